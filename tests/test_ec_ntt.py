"""panda_ec_ntt / panda_ec_ntt_plan: the discrete Fourier transform over G1 points.

    out[k] = sum_j omega^(jk) P_j        k, j < n = 2^log_n, natural order; the inverse uses omega^-1 and multiplies by 1 / n

Expected values are Python integers through tests/pyref.py (ec_add, ec_mul, the moduli): affine points, put on the wire with the
identity as all-zero bytes.  Output coordinates are canonical, so every comparison is byte for byte; there is no tolerance anywhere.
Every device buffer carries a guard run of a fixed byte pattern behind the data, which no call may touch; the input of an out-of-place
call must come back unchanged.  The host program tests/host_check/ec_ntt_host.cpp runs the per-thread routines under FE29_CHECK."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import field_ref as fr
import oracle as po
import pyref
from gpu_util import GuardedBuffers, assert_exported, gm, run_host_check  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

NAMES = ("panda_ec_ntt", "panda_ec_ntt_plan", "panda_points_to_affine", "panda_points_to_affine_plan")
CURVES = (0, 1, 2)
FORWARD, INVERSE = 0, 1
gpu = pytest.mark.gpu


def _pb(curve):
    return 64 if curve == 0 else 96


def _enc(curve, P):
    """affine point -> wire words; the identity is all-zero bytes"""
    c = pyref.CURVES[curve]
    return np.zeros(2 * c.lc_q, np.uint32) if P is None else pyref.encode_affine(c, P)


def _enc_all(curve, pts):
    return np.stack([_enc(curve, P) for P in pts])


@functools.lru_cache(maxsize=None)
def _omega_wire(curve, log_n):
    return po.root_of_unity(po.FR_OF[curve], log_n)


@functools.lru_cache(maxsize=None)
def _omega(curve, log_n):
    c = pyref.CURVES[curve]
    w = pyref.decode_scalar(c, _omega_wire(curve, log_n))
    assert pow(w, 1 << log_n, c.r) == 1 and (log_n == 0 or pow(w, 1 << (log_n - 1), c.r) == c.r - 1)
    return w


@functools.lru_cache(maxsize=None)
def _mul_g(curve, k):
    c = pyref.CURVES[curve]
    return pyref.ec_mul(c, k % c.r, c.g)


def _dft(curve, s, log_n, inverse=False, ks=None):
    """sum_j s_j w^(jk) mod r for k in ks (all k by default); w = omega, or omega^-1 with the 1 / n"""
    c, n = pyref.CURVES[curve], 1 << log_n
    w = _omega(curve, log_n)
    scale = 1
    if inverse:
        w, scale = pow(w, -1, c.r), pow(n, -1, c.r)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * w % c.r
    return [sum(s[j] * pw[j * k % n] for j in range(n)) * scale % c.r for k in (range(n) if ks is None else ks)]


def _plan(lib, curve, log_n, direction):
    l, s, u = C.c_uint(0xDEAD), C.c_size_t(0xDEAD), C.c_uint(0xDEAD)
    rc = lib.panda_ec_ntt_plan(curve, log_n, direction, C.byref(l), C.byref(s), C.byref(u))
    return rc, l.value, s.value, u.value


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, _ = assert_exported(NAMES)
    assert len(set(NAMES)) == 4 and "panda_ec_ntt_gpu" in dir(pgm) and "panda_points_gpu_to_affine" in dir(pgm)
    for macro, value in (("PANDA_EC_NTT_FORWARD", "0u"), ("PANDA_EC_NTT_INVERSE", "1u"), ("PANDA_EC_NTT_MAX_LOG_N", "26")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), header)
    assert (ffi.EC_NTT_FORWARD, ffi.EC_NTT_INVERSE, ffi.EC_NTT_MAX_LOG_N) == (0, 1, 26)
    import panda_amd
    assert panda_amd.panda_ec_ntt_gpu is pgm.panda_ec_ntt_gpu and panda_amd.panda_points_gpu_to_affine is pgm.panda_points_gpu_to_affine


def test_plan():
    lib = ffi.load()
    for curve in CURVES:
        point = 144 if curve == 0 else 224
        for log_n in list(range(0, 14)) + [20, 26]:
            n = 1 << log_n
            for direction in (FORWARD, INVERSE):
                rc, launches, scratch, uniform = _plan(lib, curve, log_n, direction)
                assert rc == 0, (curve, log_n, direction)
                stages = log_n
                assert uniform == max(0, log_n - 6), "the stages in which at least 64 butterflies share a twiddle"
                assert uniform <= stages
                assert scratch >= n * point + (n // 2) * 32
                assert scratch <= n * point + (n // 2) * 32 + 4096
                if log_n == 0:
                    assert launches == 2
                else:
                    assert launches == (1 if log_n >= 2 else 0) + stages + (1 if direction == INVERSE else 0) + 1
    assert lib.panda_ec_ntt_plan(0, 12, 0, None, None, None) == 0
    for bad in ((3, 12, 0), (4, 12, 0), (6, 12, 0), (7, 12, 0), (0xFFFFFFFF, 12, 0), (0, 27, 0), (0, 0xFFFFFFFF, 0), (0, 12, 2), (2, 12, 0xFFFFFFFF)):
        rc, launches, scratch, uniform = _plan(lib, *bad)
        assert rc == 1 and (launches, scratch, uniform) == (0xDEAD,) * 3, bad


def _refusals(lib, curve, IN, OUT, log_n, stream, untouched):
    """every refusal of the contract over valid buffers of 2^log_n points at IN and OUT (disjoint, at least one point of room on either
    side of each); `untouched()` says that nothing was written"""
    pb, n = _pb(curve), 1 << log_n
    c = pyref.CURVES[curve]
    good = np.ascontiguousarray(_omega_wire(curve, log_n))
    count = [0]

    def call(curve=curve, d_in=IN, d_out=OUT, log_n=log_n, direction=FORWARD, omega=good):
        count[0] += 1
        om = None if omega is None else C.c_void_p(np.ascontiguousarray(omega, np.uint32).ctypes.data)
        rc = lib.panda_ec_ntt(curve, None if d_in is None else C.c_void_p(d_in), None if d_out is None else C.c_void_p(d_out), log_n, direction, om, stream)
        assert untouched(), "a refused call wrote to a buffer"
        return rc

    for bad_curve in (3, 4, 6, 5, 7, 0xFFFFFFFF):
        assert call(curve=bad_curve) == 1, "a G2 or unknown curve id"
    assert call(log_n=27) == 1 and call(log_n=0xFFFFFFFF) == 1 and call(direction=2) == 1 and call(direction=0xFFFFFFFF) == 1
    assert call(d_in=None) == 1 and call(d_out=None) == 1 and call(omega=None) == 1 and call(omega=None, log_n=0) == 1
    assert call(omega=pyref.int_to_limbs(c.r, 8)) == 1 and call(omega=np.full(8, 0xFFFFFFFF, np.uint32)) == 1, "omega >= the modulus"
    w = _omega(curve, log_n)
    to_wire = lambda v: fr.wire_one(curve, v)
    assert call(omega=to_wire(w * w)) == 1, "omega^2: a root of half the order"
    assert call(omega=_omega_wire(curve, log_n + 1)) == 1, "the root of the next size up"
    assert call(omega=to_wire(1)) == 1 and call(omega=to_wire(0)) == 1 and call(omega=to_wire(c.r - 1)) == (0 if log_n == 1 else 1)
    for direction in (FORWARD, INVERSE):
        for off in (pb, -pb, 16, -16, n * pb - 16, -(n * pb - 16)):
            assert call(d_out=IN + off, direction=direction) == 1, ("overlap", off)
    return count[0]


def test_bad_arguments_are_refused_before_any_device_call():
    """also on a machine with no device: host memory stands in for the device buffers, nothing may dereference or write it"""
    lib = ffi.load()
    mem = np.full(4 << 20, 0x5A, np.uint8)
    base = (mem.ctypes.data + 4095) & ~4095
    for curve in CURVES:
        n_calls = _refusals(lib, curve, base + (1 << 20), base + (2 << 20), 4, ffi.PandaStream(), lambda: bool((mem == 0x5A).all()))
        assert n_calls > 30


def test_host_program_checks_the_bounds_and_the_exceptional_cases(tmp_path):
    """tests/host_check/ec_ntt_host.cpp: scalar_mul, butterfly, a whole transform of 8 points and normalise_chunk of ec_ntt.h on the host
    under FE29_CHECK against the affine law in integer arithmetic of its own, for the three curves: B, A and both the identity,
    w B = A, w B = -A, the twiddles 1, r - 1 and one with the top bit set, a chunk of identities only and one whose first and last
    points are identities; every stored point is checked against the stored-point bounds"""
    assert run_host_check(tmp_path, "ec_ntt_host.cpp") >= 5000


# ------------------------------------------------------------------------------------------------- on the device
class Dev(GuardedBuffers):
    """guarded device buffers, and the transform over them"""

    def __init__(self, gm, curve=0):
        super().__init__()
        self.lib, self.curve, self.stream = ffi.load(), curve, gm.exec_stream.raw

    def ntt(self, src, dst, log_n, direction=FORWARD, omega=None):
        om = np.ascontiguousarray(_omega_wire(self.curve, log_n) if omega is None else omega)
        return self.lib.panda_ec_ntt(self.curve, src.ptr, dst.ptr, log_n, direction, C.c_void_p(om.ctypes.data), self.stream)


def _transform(gm, curve, words, log_n, direction=FORWARD, what=""):
    """out of place; guards and the input checked; returns the output words (n, 2 L)"""
    h = Dev(gm, curve)
    try:
        src, dst = h.buffer(words), h.buffer(nbytes=(1 << log_n) * _pb(curve))
        assert h.ntt(src, dst, log_n, direction) == 0, what
        assert h.intact(src) and h.intact(dst), what
        return h.get(dst).reshape(1 << log_n, -1)
    finally:
        h.close()


def _compare(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, "first differing outputs", bad[:8].tolist())


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_definition(gm, curve):
    """log_n = 0 .. 4, both directions: P_j = s_j G, out[k] = (sum_j s_j omega^(jk)) G, the whole output byte for byte"""
    for log_n in range(5):
        n = 1 << log_n
        s = fr.random_residues(curve, 0xEC00 + 16 * curve + log_n, n)
        words = _enc_all(curve, [_mul_g(curve, v) for v in s])
        for direction in (FORWARD, INVERSE):
            want = _enc_all(curve, [_mul_g(curve, v) for v in _dft(curve, s, log_n, direction == INVERSE)])
            _compare(_transform(gm, curve, words, log_n, direction), want, (curve, log_n, direction))


@gpu
def test_log_n_zero_identity_and_random_half_identities(gm):
    """the lone point of log_n == 0 when it is the identity (x == 0 with a y that is not), and at log_n = 4 a random half of the inputs
    the identity, against the definition"""
    for curve in CURVES:
        c = pyref.CURVES[curve]
        ident = np.concatenate([np.zeros(c.lc_q, np.uint32), pyref.int_to_limbs(c.Rq, c.lc_q)])[None, :]
        assert not _transform(gm, curve, ident, 0).any() and not _transform(gm, curve, ident, 0, INVERSE).any()
        s = fr.random_residues(curve, 0xEC80 + curve, 16)
        hole = np.random.default_rng(0xEC90 + curve).permutation(16)[:8]
        for j in hole:
            s[j] = 0
        pts = _enc_all(curve, [_mul_g(curve, v) if v else None for v in s])
        pts[hole[0], c.lc_q:] = pyref.int_to_limbs(c.Rq, c.lc_q)  # x == 0 alone marks the identity
        for direction in (FORWARD, INVERSE):
            want = _enc_all(curve, [_mul_g(curve, v) for v in _dft(curve, s, 4, direction == INVERSE)])
            _compare(_transform(gm, curve, pts, 4, direction), want, (curve, direction))


SAMPLES_12 = sorted([0, 1, 2048, 4095] + [int(k) for k in np.random.default_rng(0xEC12).choice([k for k in range(2, 4095) if k != 2048], 60, replace=False)])


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_across_workgroups_and_both_stage_kinds(gm, curve):
    """log_n = 12: P_j = (a + j d) G built by repeated additions; 64 fixed outputs against (sum_j (a + j d) omega^(jk)) G, and
    inverse(forward(P)) == P over the whole buffer, out of place and in place"""
    log_n, n = 12, 1 << 12
    lib = ffi.load()
    rc, launches, scratch, uniform = _plan(lib, curve, log_n, FORWARD)
    assert rc == 0 and uniform >= 2 and log_n - uniform >= 2, "two uniform and two divergent stages"
    assert (n // 2) // 64 > 1, "more than one workgroup per stage (a workgroup is 64 butterflies)"
    assert len(SAMPLES_12) == 64 and {0, 1, n // 2, n - 1} <= set(SAMPLES_12)
    c = pyref.CURVES[curve]
    a, d = fr.random_residues(curve, 0xEC20 + curve, 2)
    step, P, pts = _mul_g(curve, d), _mul_g(curve, a), []
    for j in range(n):
        pts.append(P)
        P = pyref.ec_add(c, P, step)
    words = _enc_all(curve, pts)
    h = Dev(gm, curve)
    try:
        src, mid, back = h.buffer(words), h.buffer(nbytes=n * _pb(curve)), h.buffer(nbytes=n * _pb(curve))
        assert h.ntt(src, mid, log_n, FORWARD) == 0 and h.intact(src) and h.intact(mid)
        got = h.get(mid).reshape(n, -1)
        want = _dft(curve, [(a + j * d) % c.r for j in range(n)], log_n, ks=SAMPLES_12)
        for k, v in zip(SAMPLES_12, want):
            assert np.array_equal(got[k], _enc(curve, _mul_g(curve, v))), (curve, "output", k)
        assert h.ntt(mid, back, log_n, INVERSE) == 0 and h.intact(back)
        _compare(h.get(back).reshape(n, -1), words, "inverse(forward), out of place")
        assert np.array_equal(h.get(mid).reshape(n, -1), got), "the input of an out-of-place call changed"
        assert h.ntt(mid, mid, log_n, INVERSE) == 0 and h.intact(back) and h.guard_intact(mid)
        _compare(h.get(mid).reshape(n, -1), words, "inverse(forward), in place")
        assert h.ntt(mid, mid, log_n, FORWARD) == 0
        _compare(h.get(mid).reshape(n, -1), got, "forward in place equals forward out of place")
    finally:
        h.close()


@gpu
def test_random_points_at_2_to_8(gm):
    """BN254, 2^8 random s_j: 16 sampled outputs against the definition and the round trip over the whole buffer"""
    curve, log_n, n = 0, 8, 256
    s = fr.random_residues(curve, 0xEC88, n)
    words = _enc_all(curve, [_mul_g(curve, v) for v in s])
    got = _transform(gm, curve, words, log_n)
    ks = [0, 1, 2, 3, 64, 127, 128, 129, 200, 254, 255, 17, 33, 65, 99, 192]
    for k, v in zip(ks, _dft(curve, s, log_n, ks=ks)):
        assert np.array_equal(got[k], _enc(curve, _mul_g(curve, v))), k
    _compare(_transform(gm, curve, got, log_n, INVERSE), words, "round trip")


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_structured_inputs_with_closed_forms(gm, curve):
    """all P_j = P -> n P at 0, the identity elsewhere (nothing but P + P and P + (-P)); P_j = (-1)^j P -> n P at n / 2; one point at
    j in {0, 1, n - 1} -> out[k] = omega^(jk) P; all identities -> all identities.  log_n = 6 whole buffer; 12 whole buffer for the
    closed forms with one non-identity output, sampled outputs for the single point"""
    c = pyref.CURVES[curve]
    P = _mul_g(curve, fr.random_residues(curve, 0xEC60 + curve, 1)[0])
    neg = (P[0], (-P[1]) % c.p)
    w6 = _omega(curve, 6)
    table = [None] * 64  # omega_6^k P
    for k in range(64):
        table[k] = pyref.ec_mul(c, pow(w6, k, c.r), P)
    for log_n in (6, 12):
        n = 1 << log_n
        zero = np.zeros((n, 2 * c.lc_q), np.uint32)
        nP = _enc(curve, pyref.ec_mul(c, n, P))
        want = zero.copy()
        want[0] = nP
        _compare(_transform(gm, curve, np.tile(_enc(curve, P), (n, 1)), log_n), want, (log_n, "all equal"))
        want = zero.copy()
        want[n // 2] = nP
        alternating = np.stack([_enc(curve, P), _enc(curve, neg)] * (n // 2))
        _compare(_transform(gm, curve, alternating, log_n), want, (log_n, "alternating signs"))
        assert not _transform(gm, curve, zero, log_n).any(), (log_n, "all identities")
        assert not _transform(gm, curve, zero, log_n, INVERSE).any(), (log_n, "all identities, inverse")
        w = _omega(curve, log_n)
        for j in (0, 1, n - 1):
            x = zero.copy()
            x[j] = _enc(curve, P)
            got = _transform(gm, curve, x, log_n)
            if log_n == 6:
                _compare(got, _enc_all(curve, [table[j * k % 64] for k in range(64)]), (log_n, "one point at", j))
            else:  # omega_12^(64 i) = omega_6^i: the multiples of 64 reuse the table
                for k in (0, 64, 128, 2048, 4032, 1984, 3008):
                    assert np.array_equal(got[k], _enc(curve, table[(j * k // 64) % 64])), (log_n, j, k)
                for k in (1, n - 1):
                    assert np.array_equal(got[k], _enc(curve, pyref.ec_mul(c, pow(w, j * k, c.r), P))), (log_n, j, k)


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_commitment_identity_on_the_device(gm, curve):
    """Q = inverse EC-NTT of P, e = forward NTT of c:  MSM(Q, e) == MSM(P, c) for any base set P (here panda_gen_bases at 2^12)"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    log_n, n = 12, 1 << 12
    lib = ffi.load()
    c = pyref.CURVES[curve]
    d = DeviceBuffer(n * _pb(curve))
    try:
        ffi.check(lib.panda_gen_bases(curve, 0xECB0 + curve, 0, n, d.ptr, NULL_STREAM), "gen")
        P = d.to_host(np.uint32).reshape(n, -1)
    finally:
        d.free()
    om = _omega_wire(curve, log_n)
    Q = pgm.panda_ec_ntt_gpu(gm, P, om, curve, inverse=True).view(np.uint32).reshape(n, -1)
    coeffs = po.gen_scalars(po.FR_OF[curve], 0xECC0 + curve, n)
    evals = coeffs.copy()
    ntt = {0: lambda b: pgm.panda_ntt_bn254_gpu_v1(gm, b, om, log_n), 1: lambda b: pgm.panda_ntt_bls12_377_gpu_v1(gm, b, om, log_n),
           2: lambda b: pgm.panda_ntt_bls12_381_gpu_v1(gm, b, om, log_n)}[curve]
    ntt(evals)
    assert not np.array_equal(evals, coeffs)
    lhs = pyref.decode_jacobian(c, pgm.panda_msm_bn254_gpu(gm, evals, Q, curve).view(np.uint32))
    rhs = pyref.decode_jacobian(c, pgm.panda_msm_bn254_gpu(gm, coeffs, P, curve).view(np.uint32))
    assert lhs is not None and lhs == rhs


@gpu
def test_refusals_leave_the_guarded_output_untouched(gm):
    from gpu_util import DeviceBuffer
    lib = ffi.load()
    for curve in CURVES:
        h = Dev(gm, curve)
        try:
            log_n, pb = 4, _pb(curve)
            room = h.buffer(_enc_all(curve, [_mul_g(curve, j + 1) for j in range(48)]))  # IN is its middle third
            out = h.buffer(nbytes=48 * pb)
            IN, OUT = room.ptr.value + 16 * pb, out.ptr.value + 16 * pb
            untouched = lambda: h.intact(room) and h.untouched(out)
            assert _refusals(lib, curve, IN, OUT, log_n, h.stream, untouched) > 30
            # a buffer of the library's allocator shorter than stated
            short = DeviceBuffer(16 * pb)
            try:
                om = np.ascontiguousarray(_omega_wire(curve, 5))
                for d_in, d_out in ((short.ptr.value, OUT), (IN, short.ptr.value), (short.ptr.value + pb, short.ptr.value + pb)):
                    rc = lib.panda_ec_ntt(curve, C.c_void_p(d_in), C.c_void_p(d_out), 5 if d_in != d_out else 4, FORWARD,
                                          C.c_void_p((om if d_in != d_out else np.ascontiguousarray(_omega_wire(curve, 4))).ctypes.data), h.stream)
                    assert rc == 1 and untouched(), (curve, "short buffer")
            finally:
                short.free()
        finally:
            h.close()
