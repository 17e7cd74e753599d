"""panda_points_scalar_mul / panda_points_scalar_mul_plan: out[i] = A_i + k_i P_i over a vector of G1 points.

    k_i = d_scalars[i] (EACH), the one host scalar (ONE), c s^i (POWERS); the A_i term is optional

Expected values are Python integers through tests/pyref.py (ec_add, encode_affine; tests/points_ref.py builds the multiples of G from
them): affine points on the wire, the identity as all-zero bytes.  Output coordinates are canonical, so every comparison is byte for
byte; there is no tolerance anywhere.  Every device buffer carries a guard run behind the data, which no call may touch; the inputs of
an out-of-place call must come back unchanged.  tests/host_check/points_mul_host.cpp runs the per-thread routines under FE29_CHECK."""
import ctypes as C
import re

import numpy as np
import pytest

import field_ref as fr
import pyref
from gpu_util import assert_exported, gm, run_host_check  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm
from points_ref import CURVES, Dev, compare, enc, enc_all, enc_multiples, host_ptr, mul_g, point_bytes

NAMES = ("panda_points_scalar_mul", "panda_points_scalar_mul_plan", "panda_kzg_open_all_setup", "panda_kzg_open_all", "panda_kzg_open_all_plan")
EACH, ONE, POWERS = 0, 1, 2
MODES = (EACH, ONE, POWERS)
SIZES = (1, 2, 63, 64, 65, 130)  # a wave is 64 points, a normalisation chunk 16: a short last wave, a short last chunk, three waves
N = 130
gpu = pytest.mark.gpu


def _plan(lib, curve, mode, n):
    l, s = C.c_uint(0xDEAD), C.c_size_t(0xDEAD)
    return lib.panda_points_scalar_mul_plan(curve, mode, n, C.byref(l), C.byref(s)), l.value, s.value


def _ptr(v):
    return None if v is None else C.c_void_p(v)


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, _ = assert_exported(NAMES)
    for macro, value in (("PANDA_POINTS_MUL_EACH", "0u"), ("PANDA_POINTS_MUL_ONE", "1u"), ("PANDA_POINTS_MUL_POWERS", "2u"), ("PANDA_KZG_OPEN_ALL_MAX_LOG_N", "25")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), header)
    assert (ffi.POINTS_MUL_EACH, ffi.POINTS_MUL_ONE, ffi.POINTS_MUL_POWERS, ffi.KZG_OPEN_ALL_MAX_LOG_N) == (0, 1, 2, 25)
    import panda_amd
    assert panda_amd.panda_points_gpu_scalar_mul is pgm.panda_points_gpu_scalar_mul and panda_amd.PandaKzgOpenAll is pgm.PandaKzgOpenAll


def test_plan():
    lib = ffi.load()
    for curve in CURVES:
        point = 144 if curve == 0 else 224
        for mode in MODES:
            for n in (1, 63, 64, 65, 4096, 4097, 1 << 28):
                rc, launches, scratch = _plan(lib, curve, mode, n)
                assert rc == 0 and launches == 2, (curve, mode, n)
                assert n * point <= scratch <= n * point + 4096
    assert lib.panda_points_scalar_mul_plan(0, 0, 64, None, None) == 0
    for bad in ((3, 0, 64), (4, 0, 64), (6, 0, 64), (0xFFFFFFFF, 0, 64), (0, 3, 64), (0, 0xFFFFFFFF, 64), (0, 0, 0), (2, 1, (1 << 28) + 1), (1, 2, 1 << 63)):
        rc, launches, scratch = _plan(lib, *bad)
        assert rc == 1 and (launches, scratch) == (0xDEAD, 0xDEAD), bad


def _refusals(lib, curve, P, A, OUT, SC, n, stream, untouched):
    """every refusal of the contract over valid buffers of n points at P, A and OUT and of n scalars at SC (disjoint, at least one point
    of room on either side of each); `untouched()` says that nothing was written"""
    pb, c = point_bytes(curve), pyref.CURVES[curve]
    one, two = np.ascontiguousarray(fr.wire_one(curve, 5)), np.ascontiguousarray(np.concatenate([fr.wire_one(curve, 3), fr.wire_one(curve, 7)]))
    count = [0]

    def call(curve=curve, mode=EACH, pts=P, d_sc=SC, h_sc=None, add=A, out=OUT, n=n):
        count[0] += 1
        rc = lib.panda_points_scalar_mul(curve, mode, _ptr(pts), _ptr(d_sc), host_ptr(h_sc), _ptr(add), _ptr(out), n, stream)
        assert untouched(), "a refused call wrote to a buffer"
        return rc

    for bad_curve in (3, 4, 6, 5, 7, 0xFFFFFFFF):
        assert call(curve=bad_curve) == 1, "a G2 or unknown curve id"
    assert call(mode=3) == 1 and call(mode=0xFFFFFFFF) == 1
    assert call(n=0) == 1 and call(n=(1 << 28) + 1) == 1 and call(n=1 << 40) == 1
    assert call(pts=None) == 1 and call(out=None) == 1 and call(pts=None, add=None) == 1
    # the scalar pointer of the chosen mode missing, or the pointer of the other kind given
    assert call(d_sc=None) == 1 and call(h_sc=one) == 1 and call(d_sc=None, h_sc=one) == 1
    for mode, h in ((ONE, one), (POWERS, two)):
        assert call(mode=mode, d_sc=None, h_sc=None) == 1 and call(mode=mode, h_sc=h) == 1 and call(mode=mode, h_sc=None) == 1
    # host scalars at or above the modulus
    r_words, ones = pyref.int_to_limbs(c.r, 8), np.full(8, 0xFFFFFFFF, np.uint32)
    for bad in (r_words, ones):
        assert call(mode=ONE, d_sc=None, h_sc=np.ascontiguousarray(bad)) == 1
        assert call(mode=POWERS, d_sc=None, h_sc=np.ascontiguousarray(np.concatenate([bad, fr.wire_one(curve, 7)]))) == 1
        assert call(mode=POWERS, d_sc=None, h_sc=np.ascontiguousarray(np.concatenate([fr.wire_one(curve, 3), bad]))) == 1
    # overlaps: the output over either input other than exactly, and the two inputs over each other (exactly included)
    for off in (pb, -pb, 16, -16, n * pb - 16, -(n * pb - 16)):
        assert call(out=P + off) == 1 and call(out=A + off) == 1 and call(out=P + off, add=None) == 1, ("overlap", off)
        assert call(add=P + off) == 1 and call(mode=ONE, d_sc=None, h_sc=one, add=P + off) == 1, ("inputs overlap", off)
    assert call(add=P) == 1 and call(add=P, out=P) == 1
    return count[0]


def test_bad_arguments_are_refused_before_any_device_call():
    """also on a machine with no device: host memory stands in for the device buffers, nothing may dereference or write it"""
    lib = ffi.load()
    mem = np.full(8 << 20, 0x5A, np.uint8)
    base = (mem.ctypes.data + 4095) & ~4095
    for curve in CURVES:
        n_calls = _refusals(lib, curve, base + (1 << 20), base + (2 << 20), base + (3 << 20), base + (4 << 20), 16, ffi.PandaStream(),
                            lambda: bool((mem == 0x5A).all()))
        assert n_calls > 50


def test_host_program_checks_the_bounds_and_the_exceptional_cases(tmp_path):
    """tests/host_check/points_mul_host.cpp: scalar_bits, scalar_mul at every loop length from the scalar's own up to 256, add_affine_wire
    (A the identity, A = k P, A = -k P), scalar_from_wire and power_scalar of points_mul.h on the host under FE29_CHECK against the affine
    law in integer arithmetic of its own, for the three curves; every stored point is checked against the stored-point bounds"""
    assert run_host_check(tmp_path, "points_mul_host.cpp") >= 50000


# ------------------------------------------------------------------------------------------------- on the device
def _mode_scalars(curve, mode, ks=None, one=None, c=None, s=None):
    """(device scalars to stage or None, host scalars or None) of a call"""
    if mode == EACH:
        return fr.wire(curve, ks), None
    if mode == ONE:
        return None, np.ascontiguousarray(fr.wire_one(curve, one))
    return None, np.ascontiguousarray(np.concatenate([fr.wire_one(curve, c), fr.wire_one(curve, s)]))


def _run(gm, curve, mode, pts, d_sc, h_sc, add, n, what="", in_place=None):
    """one call over fresh guarded buffers; inputs and guards checked; returns the output words (n, 2 L).  in_place: None, "points" or
    "addend" -- the output buffer is then that input"""
    h = Dev(gm, curve)
    try:
        P = h.buffer(pts[:n])
        S = None if d_sc is None else h.buffer(d_sc[:n])
        A = None if add is None else h.buffer(add[:n])
        O = {None: None, "points": P, "addend": A}[in_place] or h.buffer(nbytes=n * point_bytes(curve))
        rc = h.lib.panda_points_scalar_mul(curve, mode, P.ptr, None if S is None else S.ptr, host_ptr(h_sc), None if A is None else A.ptr, O.ptr, n, h.stream)
        assert rc == 0, what
        for d in (P, S, A, O):
            if d is not None:
                assert h.guard_intact(d) if d is O else h.intact(d), (what, "an input or a guard changed")
        return h.get(O).reshape(n, -1)
    finally:
        h.close()


class Fixture:
    """per curve: P_i = a_i G, A_i = b_i G and the scalars of the three modes for i < N, computed once and left unchanged"""

    def __init__(self, curve):
        c = pyref.CURVES[curve]
        self.curve, self.r = curve, c.r
        self.a, self.b, self.k = (fr.random_residues(curve, 0x9A00 + 16 * curve + j, N) for j in range(3))
        self.one, self.c, self.s = fr.random_residues(curve, 0x9A80 + curve, 3)
        self.P, self.A = enc_multiples(curve, self.a), enc_multiples(curve, self.b)

    def scalars(self, mode):
        """the integers k_i of a mode"""
        if mode == EACH:
            return self.k
        if mode == ONE:
            return [self.one] * N
        return [self.c * pow(self.s, i, self.r) % self.r for i in range(N)]


_fixtures = {}


def _fixture(curve):
    if curve not in _fixtures:
        _fixtures[curve] = Fixture(curve)
    return _fixtures[curve]


@gpu
@pytest.mark.parametrize("addend", (False, True))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("curve", CURVES)
def test_definition(gm, curve, mode, addend):
    """n in SIZES, P_i = a_i G: out[i] = (b_i + k_i a_i) G, the whole output byte for byte"""
    f = _fixture(curve)
    ks = f.scalars(mode)
    want = enc_multiples(curve, [(f.b[i] if addend else 0) + ks[i] * f.a[i] for i in range(N)])
    d_sc, h_sc = _mode_scalars(curve, mode, ks=f.k, one=f.one, c=f.c, s=f.s)
    for n in SIZES:
        got = _run(gm, curve, mode, f.P, d_sc, h_sc, f.A if addend else None, n, (curve, mode, addend, n))
        compare(got, want[:n], (curve, mode, addend, n))


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_waves_with_different_loop_lengths(gm, curve):
    """EACH at n = 130: the first wave's scalars below 2^64 (one of them zero, one of them 1), the rest full length; and a wave of
    128-bit scalars between two full-length ones"""
    f = _fixture(curve)
    for first, lo, hi in ((64, 0, 64), (128, 64, 128)):
        ks = list(f.k)
        for i in range(lo, hi):
            ks[i] = f.k[i] % (1 << first)
        if lo == 0:
            ks[3], ks[17] = 0, 1
        for addend in (False, True):
            want = enc_multiples(curve, [(f.b[i] if addend else 0) + ks[i] * f.a[i] for i in range(N)])
            got = _run(gm, curve, EACH, f.P, fr.wire(curve, ks), None, f.A if addend else None, N, (curve, first, addend))
            compare(got, want, (curve, first, addend))


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_structured_inputs(gm, curve):
    """n = 130: all k_i = 0; all P_i the identity; k_i = 1; k_i = r - 1 (-P_i); A_i = -k_i P_i (all zeros); A_i = k_i P_i (2 k_i P_i);
    x == 0 with a nonzero y as the input identity; in place over d_points and over d_addend"""
    f, c = _fixture(curve), pyref.CURVES[curve]
    zero = np.zeros_like(f.P)
    each = lambda ks: fr.wire(curve, ks)
    host = lambda *vs: np.ascontiguousarray(np.concatenate([fr.wire_one(curve, v) for v in vs]))
    negP = enc_multiples(curve, [-a for a in f.a])
    # k = 0
    assert not _run(gm, curve, EACH, f.P, each([0] * N), None, None, N).any()
    assert not _run(gm, curve, ONE, f.P, None, host(0), None, N).any()
    assert not _run(gm, curve, POWERS, f.P, None, host(0, f.s), None, N).any()
    compare(_run(gm, curve, EACH, f.P, each([0] * N), None, f.A, N), f.A, "k = 0 with an addend")
    compare(_run(gm, curve, ONE, f.P, None, host(0), f.A, N), f.A, "k = 0, ONE, with an addend")
    # P the identity, as all-zero bytes and as x == 0 with a y that is not
    ident = zero.copy()
    ident[::2, c.lc_q:] = pyref.int_to_limbs(c.Rq, c.lc_q)
    assert not _run(gm, curve, EACH, ident, each(f.k), None, None, N).any()
    compare(_run(gm, curve, EACH, ident, each(f.k), None, f.A, N), f.A, "P the identity with an addend")
    compare(_run(gm, curve, POWERS, f.P, None, host(f.c, f.s), ident, N), enc_multiples(curve, [k * a for k, a in zip(f.scalars(POWERS), f.a)]), "A the identity")
    mixed, mixed_want = f.P.copy(), enc_multiples(curve, [k * a for k, a in zip(f.k, f.a)])
    mixed[5::7], mixed_want[5::7] = ident[5::7], 0
    compare(_run(gm, curve, EACH, mixed, each(f.k), None, None, N), mixed_want, "some P the identity")
    # k = 1 and k = r - 1
    compare(_run(gm, curve, EACH, f.P, each([1] * N), None, None, N), f.P, "k = 1, EACH")
    compare(_run(gm, curve, ONE, f.P, None, host(1), None, N), f.P, "k = 1, ONE")
    compare(_run(gm, curve, POWERS, f.P, None, host(1, 1), None, N), f.P, "c = s = 1")
    compare(_run(gm, curve, EACH, f.P, each([c.r - 1] * N), None, None, N), negP, "k = r - 1, EACH")
    compare(_run(gm, curve, ONE, f.P, None, host(c.r - 1), None, N), negP, "k = r - 1, ONE")
    compare(_run(gm, curve, POWERS, f.P, None, host(1, c.r - 1), None, N), np.where((np.arange(N) % 2 == 1)[:, None], negP, f.P), "s = -1")
    # the addend the negative of the product, and the product itself
    kP, minus = [k * a for k, a in zip(f.k, f.a)], enc_multiples(curve, [-k * a for k, a in zip(f.k, f.a)])
    assert not _run(gm, curve, EACH, f.P, each(f.k), None, minus, N).any(), "A = -k P"
    compare(_run(gm, curve, EACH, f.P, each(f.k), None, enc_multiples(curve, kP), N), enc_multiples(curve, [2 * v for v in kP]), "A = k P")
    assert not _run(gm, curve, ONE, f.P, None, host(c.r - 1), f.P, N).any(), "A = P, k = r - 1"
    compare(_run(gm, curve, ONE, f.P, None, host(1), f.P.copy(), N), enc_multiples(curve, [2 * a for a in f.a]), "A = P, k = 1")
    # in place
    want = enc_multiples(curve, [b + k * a for a, b, k in zip(f.a, f.b, f.k)])
    compare(_run(gm, curve, EACH, f.P, each(f.k), None, f.A, N, in_place="points"), want, "in place over d_points")
    compare(_run(gm, curve, EACH, f.P, each(f.k), None, f.A, N, in_place="addend"), want, "in place over d_addend")
    compare(_run(gm, curve, ONE, f.P, None, host(f.one), None, N, in_place="points"), enc_multiples(curve, [f.one * a for a in f.a]), "ONE in place")


N_MANY = 4099
SAMPLES = sorted([0, 4095, 4096, 4098] + [int(k) for k in np.random.default_rng(0x9A12).choice([k for k in range(1, 4098) if k not in (4095, 4096)], 60, replace=False)])


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_across_workgroups(gm, curve):
    """n = 4099: two normalisation workgroups (256 x 16 points each) and 65 multiplication workgroups.  P_i = (a + i d) G by repeated
    additions; 64 fixed outputs per mode against integers, and over the whole buffer k then k^-1 returns the input in every mode"""
    n, c = N_MANY, pyref.CURVES[curve]
    assert len(SAMPLES) == 64 and (n + 63) // 64 == 65 and (n + 15) // 16 > 256
    a, d, one, cc, s = fr.random_residues(curve, 0x9A20 + curve, 5)
    step, Q, pts = mul_g(curve, d), mul_g(curve, a), []
    for _ in range(n):
        pts.append(Q)
        Q = pyref.ec_add(c, Q, step)
    words = enc_all(curve, pts)
    ks = fr.random_residues(curve, 0x9A30 + curve, n)
    inv = lambda v: pow(v, -1, c.r)
    host = lambda *vs: np.ascontiguousarray(np.concatenate([fr.wire_one(curve, v) for v in vs]))
    cases = ((EACH, fr.wire(curve, ks), None, fr.wire(curve, [inv(k) for k in ks]), None, lambda i: ks[i]),
             (ONE, None, host(one), None, host(inv(one)), lambda i: one),
             (POWERS, None, host(cc, s), None, host(inv(cc), inv(s)), lambda i: cc * pow(s, i, c.r)))
    for mode, d_sc, h_sc, d_back, h_back, k_of in cases:
        got = _run(gm, curve, mode, words, d_sc, h_sc, None, n, (curve, mode))
        for i in SAMPLES:
            assert np.array_equal(got[i], enc(curve, mul_g(curve, k_of(i) * (a + i * d)))), (curve, mode, "output", i)
        compare(_run(gm, curve, mode, got, d_back, h_back, None, n, (curve, mode, "back")), words, (curve, mode, "k then 1 / k"))


@gpu
def test_refusals_leave_the_guarded_buffers_untouched(gm):
    from gpu_util import DeviceBuffer
    lib = ffi.load()
    for curve in CURVES:
        h = Dev(gm, curve)
        try:
            n, pb = 16, point_bytes(curve)
            f = _fixture(curve)
            rooms = [h.buffer(np.concatenate([f.P[:48]])), h.buffer(np.concatenate([f.A[:48]])), h.buffer(fr.wire(curve, f.k[:48]))]
            out = h.buffer(nbytes=48 * pb)
            P, A, SC, OUT = rooms[0].ptr.value + 16 * pb, rooms[1].ptr.value + 16 * pb, rooms[2].ptr.value + 16 * 32, out.ptr.value + 16 * pb
            untouched = lambda: all(h.intact(r) for r in rooms) and h.untouched(out)
            assert _refusals(lib, curve, P, A, OUT, SC, n, h.stream, untouched) > 50
            # a buffer of the library's allocator shorter than stated, in every role
            short = DeviceBuffer(16 * pb)
            try:
                sp = short.ptr.value
                for args in ((sp + pb, SC, A, OUT), (P, sp + 16 * pb - 256, A, OUT), (P, SC, sp + pb, OUT), (P, SC, A, sp + pb), (sp + pb, SC, None, sp + pb)):
                    rc = lib.panda_points_scalar_mul(curve, EACH, _ptr(args[0]), _ptr(args[1]), None, _ptr(args[2]), _ptr(args[3]), n, h.stream)
                    assert rc == 1 and untouched(), (curve, "short buffer", args)
                assert lib.panda_points_scalar_mul(curve, EACH, _ptr(sp), _ptr(SC), None, None, _ptr(sp), 17, h.stream) == 1 and untouched()
            finally:
                short.free()
        finally:
            h.close()


@gpu
def test_host_array_wrapper(gm):
    """panda_points_gpu_scalar_mul: host arrays in and out, the three modes"""
    curve = 0
    f = _fixture(curve)
    got = pgm.panda_points_gpu_scalar_mul(gm, f.P, fr.wire(curve, f.k), curve, addend=f.A)
    compare(got.view(np.uint32).reshape(N, -1), enc_multiples(curve, [b + k * a for a, b, k in zip(f.a, f.b, f.k)]), "EACH")
    got = pgm.panda_points_gpu_scalar_mul(gm, f.P, fr.wire_one(curve, f.one), curve, mode=ffi.POINTS_MUL_ONE)
    compare(got.view(np.uint32).reshape(N, -1), enc_multiples(curve, [f.one * a for a in f.a]), "ONE")
    got = pgm.panda_points_gpu_scalar_mul(gm, f.P, np.concatenate([fr.wire_one(curve, 1), fr.wire_one(curve, 1)]), curve, mode=ffi.POINTS_MUL_POWERS)
    compare(got.view(np.uint32).reshape(N, -1), f.P, "POWERS")
    with pytest.raises(pgm.PandaGpuError):
        pgm.panda_points_gpu_scalar_mul(gm, f.P, fr.wire(curve, f.k[:5]), curve)
