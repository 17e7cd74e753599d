"""panda_kzg_open_all_setup / panda_kzg_open_all / panda_kzg_open_all_plan: the KZG proofs of one polynomial at all n points of its domain.

    d_proofs[k] = the commitment to (f(X) - f(w^k)) / (X - w^k) under s_i = [tau^i]G,   w = omega2^2,  k < n = 2^log_n

The SRS comes from a known tau, s_i = (tau^i mod r) G, and the reference proof is (sum_j q_j tau^j) G with q from synthetic division in
Python integers -- not the fraction (f(tau) - f(z)) / (tau - z), so tau on the domain is legal.  Points are built through tests/pyref.py
(tests/points_ref.py); every comparison is byte for byte, every device buffer carries a guard run, inputs must come back unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import field_ref as fr
import oracle as po
import pyref
from gpu_util import assert_exported, gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm
from points_ref import CURVES, Dev, compare, enc_multiples, host_ptr, point_bytes

NAMES = ("panda_kzg_open_all_setup", "panda_kzg_open_all", "panda_kzg_open_all_plan")
gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _omega2_wire(curve, log_n):
    return np.ascontiguousarray(po.root_of_unity(po.FR_OF[curve], log_n + 1))


@functools.lru_cache(maxsize=None)
def _omega(curve, log_n):
    """the domain's generator omega2^2 as an integer"""
    c = pyref.CURVES[curve]
    w2 = pyref.decode_scalar(c, _omega2_wire(curve, log_n))
    assert pow(w2, 1 << log_n, c.r) == c.r - 1
    return w2 * w2 % c.r


def _plan(lib, curve, log_n):
    w, l = C.c_size_t(0xDEAD), C.c_uint(0xDEAD)
    return lib.panda_kzg_open_all_plan(curve, log_n, C.byref(w), C.byref(l)), w.value, l.value


def _ptr(v):
    return None if v is None else C.c_void_p(v)


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_and_plan():
    _, lib = assert_exported(NAMES)
    assert "PandaKzgOpenAll" in dir(pgm)
    u = C.c_uint
    for curve in CURVES:
        for log_n in (1, 2, 3, 4, 9, 10, 16, 17, 20, 25):
            rc, work, launches = _plan(lib, curve, log_n)
            n = 1 << log_n
            assert rc == 0 and work == (2 * n * 32 + 2 * n * point_bytes(curve) + 255) // 256 * 256, (curve, log_n)
            passes, mul, inverse, forward = u(0), u(0), u(0), u(0)
            assert lib.panda_ntt_batch_plan(log_n + 1, ffi.NTT_FORWARD, 1, C.byref(passes), None) == 0
            assert lib.panda_points_scalar_mul_plan(curve, ffi.POINTS_MUL_EACH, 2 * n, C.byref(mul), None) == 0
            assert lib.panda_ec_ntt_plan(curve, log_n + 1, ffi.EC_NTT_INVERSE, C.byref(inverse), None, None) == 0
            assert lib.panda_ec_ntt_plan(curve, log_n, ffi.EC_NTT_FORWARD, C.byref(forward), None, None) == 0
            assert launches == 1 + passes.value + mul.value + inverse.value + 1 + forward.value, "the pad, the parts, the middle copy"
    assert lib.panda_kzg_open_all_plan(0, 4, None, None) == 0
    for bad in ((3, 4), (4, 4), (6, 4), (0xFFFFFFFF, 4), (0, 0), (0, 26), (2, 0xFFFFFFFF)):
        rc, work, launches = _plan(lib, *bad)
        assert rc == 1 and (work, launches) == (0xDEAD, 0xDEAD), bad


def _refusals(lib, curve, log_n, SRS, TABLE, COEFFS, WORK, PROOFS, stream, untouched):
    """every refusal of the two calls over valid disjoint buffers with at least one point of room on either side of each"""
    pb, n, c = point_bytes(curve), 1 << log_n, pyref.CURVES[curve]
    good = _omega2_wire(curve, log_n)
    rc, work_bytes, _ = _plan(lib, curve, log_n)
    assert rc == 0
    count = [0]

    def setup(curve=curve, srs=SRS, log_n=log_n, omega2=good, table=TABLE):
        count[0] += 1
        rc = lib.panda_kzg_open_all_setup(curve, _ptr(srs), log_n, host_ptr(omega2), _ptr(table), stream)
        assert untouched(), "a refused setup wrote to a buffer"
        return rc

    def open_(curve=curve, coeffs=COEFFS, table=TABLE, log_n=log_n, omega2=good, work=WORK, wb=work_bytes, proofs=PROOFS):
        count[0] += 1
        rc = lib.panda_kzg_open_all(curve, _ptr(coeffs), _ptr(table), log_n, host_ptr(omega2), _ptr(work), wb, _ptr(proofs), stream)
        assert untouched(), "a refused open wrote to a buffer"
        return rc

    to_wire = lambda v: np.ascontiguousarray(fr.wire_one(curve, v))
    w2 = pyref.decode_scalar(c, good)
    bad_roots = (np.ascontiguousarray(pyref.int_to_limbs(c.r, 8)), np.full(8, 0xFFFFFFFF, np.uint32), to_wire(w2 * w2), to_wire(1), to_wire(0),
                 _omega2_wire(curve, log_n + 1), _omega2_wire(curve, log_n - 1) if log_n > 1 else to_wire(c.r - 1))
    for call in (setup, open_):
        for bad_curve in (3, 4, 6, 5, 0xFFFFFFFF):
            assert call(curve=bad_curve) == 1
        assert call(log_n=0) == 1 and call(log_n=26) == 1 and call(log_n=0xFFFFFFFF) == 1 and call(omega2=None) == 1 and call(table=None) == 1
        for root in bad_roots:
            assert call(omega2=root) == 1, "omega2 is not a primitive 2n-th root below the modulus"
    assert setup(srs=None) == 1 and open_(coeffs=None) == 1 and open_(work=None) == 1 and open_(proofs=None) == 1
    assert open_(wb=work_bytes - 1) == 1 and open_(wb=0) == 1
    for off in (pb, -pb, 16, -16, n * pb - 16, -(2 * n * pb - 16), 0):
        assert setup(table=SRS + off) == 1, ("setup overlap", off)
    for off in (0, 32, -32, 16, n * 32 - 16, -(n * 32 - 16)):
        assert open_(proofs=COEFFS + off) == 1 and open_(work=COEFFS + off) == 1 and open_(table=COEFFS + off) == 1, ("coeffs", off)
        assert open_(proofs=TABLE + off) == 1 and open_(work=TABLE + off) == 1 and open_(proofs=WORK + off) == 1, ("table, work", off)
    assert open_(proofs=WORK + work_bytes - 16) == 1 and open_(coeffs=WORK + work_bytes - 16) == 1
    return count[0]


def test_bad_arguments_are_refused_before_any_device_call():
    """also on a machine with no device: host memory stands in for the device buffers, nothing may dereference or write it"""
    lib = ffi.load()
    mem = np.full(8 << 20, 0x5A, np.uint8)
    base = (mem.ctypes.data + 4095) & ~4095
    for curve in CURVES:
        n_calls = _refusals(lib, curve, 3, *(base + (j << 20) for j in range(1, 6)), ffi.PandaStream(), lambda: bool((mem == 0x5A).all()))
        assert n_calls > 80


# ------------------------------------------------------------------------------------------------- on the device
def _reference(curve, f, tau, log_n):
    """the n proofs as integers e_k with proof_k = e_k G: e_k = sum_j q_j tau^j, q the quotient of f by X - omega^k (synthetic division)"""
    r, n, w = pyref.CURVES[curve].r, 1 << log_n, _omega(curve, log_n)
    tp = [pow(tau, j, r) for j in range(n)]
    out, z = [], 1
    for _ in range(n):
        S, e = 0, 0
        for j in range(n - 1, 0, -1):  # q_(j-1) = S_j = f_j + z S_(j+1)
            S = (f[j] + z * S) % r
            e += S * tp[j - 1]
        out.append(e % r)
        z = z * w % r
    return out


def _open_all(gm, curve, log_n, f, tau, what, opens=1):
    """setup and `opens` opens over guarded buffers: inputs, the table and the guards checked; returns the proofs' words (n, 2 L)"""
    n, pb, r = 1 << log_n, point_bytes(curve), pyref.CURVES[curve].r
    lib, om = ffi.load(), _omega2_wire(curve, log_n)
    rc, work_bytes, _ = _plan(lib, curve, log_n)
    assert rc == 0
    h = Dev(gm, curve)
    try:
        srs = h.buffer(enc_multiples(curve, [pow(tau, i, r) for i in range(n)]))
        table, work, proofs = h.buffer(nbytes=2 * n * pb), h.buffer(nbytes=work_bytes), h.buffer(nbytes=n * pb)
        coeffs = h.buffer(fr.wire(curve, f))
        assert lib.panda_kzg_open_all_setup(curve, srs.ptr, log_n, host_ptr(om), table.ptr, h.stream) == 0, what
        assert h.intact(srs) and h.guard_intact(table) and h.untouched(work) and h.untouched(proofs), (what, "setup")
        table.host = h.get(table)
        got = None
        for _ in range(opens):
            assert lib.panda_kzg_open_all(curve, coeffs.ptr, table.ptr, log_n, host_ptr(om), work.ptr, work_bytes, proofs.ptr, h.stream) == 0, what
            assert h.intact(coeffs) and h.intact(table) and h.intact(srs) and h.guard_intact(work) and h.guard_intact(proofs), (what, "open")
            now = h.get(proofs).reshape(n, -1)
            assert got is None or np.array_equal(got, now), (what, "a second open gave other bytes")
            got = now
        return got
    finally:
        h.close()


def _check(gm, curve, log_n, f, tau, what, opens=1):
    got = _open_all(gm, curve, log_n, f, tau, what, opens)
    compare(got, enc_multiples(curve, _reference(curve, f, tau, log_n)), what)
    return got


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_small_domains(gm, curve):
    """log_n = 1 .. 4, random f and tau, the whole output; two opens give the same bytes"""
    for log_n in (1, 2, 3, 4):
        tau, = fr.random_residues(curve, 0xF200 + 16 * curve + log_n, 1)
        f = fr.random_residues(curve, 0xF280 + 16 * curve + log_n, 1 << log_n)
        _check(gm, curve, log_n, f, tau, (curve, log_n), opens=2)


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_special_cases(gm, curve):
    """log_n = 3: tau = omega^3 (the SRS repeats, and the fraction's division by zero is not the reference's); tau = 1 (every SRS point is
    G: doublings and cancellations only); f constant (all identities); f with a zero top coefficient; f = X^(n - 1)"""
    log_n, n, r = 3, 8, pyref.CURVES[curve].r
    f = fr.random_residues(curve, 0xF300 + curve, n)
    tau, = fr.random_residues(curve, 0xF310 + curve, 1)
    _check(gm, curve, log_n, f, pow(_omega(curve, log_n), 3, r), "tau on the domain")
    _check(gm, curve, log_n, f, 1, "tau = 1")
    assert not _check(gm, curve, log_n, [f[0]] + [0] * (n - 1), tau, "f constant").any()
    assert not _check(gm, curve, log_n, [0] * n, tau, "f = 0").any()
    _check(gm, curve, log_n, f[:n - 1] + [0], tau, "zero top coefficient")
    _check(gm, curve, log_n, [0] * (n - 1) + [1], tau, "f = X^(n - 1)")


@gpu
@pytest.mark.parametrize("curve,log_n", ((0, 8), (1, 6), (2, 6)))
def test_uniform_and_divergent_stages(gm, curve, log_n):
    """the whole output at 2n = 512 on BN254 (uniform and divergent EC-NTT stages, eight multiplication waves) and 2n = 128 on the BLS curves"""
    tau, = fr.random_residues(curve, 0xF400 + curve, 1)
    _check(gm, curve, log_n, fr.random_residues(curve, 0xF410 + curve, 1 << log_n), tau, (curve, log_n))


@gpu
def test_against_division_and_msm_on_the_device(gm):
    """BN254, log_n = 10, panda_gen_bases points as an SRS of unknown tau: proofs 0, 1, 512 and 1023 equal the MSM of the quotient
    panda_poly_divide_linear forms at omega^k -- a device-against-device identity that needs no tau.  Through PandaKzgOpenAll."""
    from gpu_util import NULL_STREAM, DeviceBuffer
    curve, log_n, n = 0, 10, 1 << 10
    lib, c = ffi.load(), pyref.CURVES[0]
    d = DeviceBuffer(n * 64)
    try:
        ffi.check(lib.panda_gen_bases(curve, 0xF500, 0, n, d.ptr, NULL_STREAM), "gen")
        srs = d.to_host(np.uint32).reshape(n, -1)
    finally:
        d.free()
    coeffs = po.gen_scalars(po.FR_OF[curve], 0xF501, n)
    opener = pgm.PandaKzgOpenAll(gm, srs, _omega2_wire(curve, log_n), curve)
    try:
        proofs = opener.open(coeffs)
        again = opener.open(coeffs)
    finally:
        opener.close()
    assert proofs.shape == (n, 64) and np.array_equal(proofs, again)
    w = _omega(curve, log_n)
    for k in (0, 1, 512, 1023):
        quot, _ = pgm.panda_poly_gpu_divide(gm, [coeffs], fr.wire_one(curve, pow(w, k, c.r)), curve)
        want = pyref.decode_jacobian(c, pgm.panda_msm_bn254_gpu(gm, quot[0], srs, curve).view(np.uint32))
        assert want is not None and pyref.decode_affine(c, proofs[k].view(np.uint32)) == want, k


@gpu
def test_refusals_leave_the_guarded_buffers_untouched(gm):
    lib = ffi.load()
    for curve in CURVES:
        h = Dev(gm, curve)
        try:
            log_n, n, pb = 3, 8, point_bytes(curve)
            rc, work_bytes, _ = _plan(lib, curve, log_n)
            srs = h.buffer(enc_multiples(curve, range(1, 3 * n + 1)))
            coeffs = h.buffer(fr.wire(curve, range(7, 7 + 3 * n)))
            table, work, proofs = h.buffer(nbytes=4 * n * pb), h.buffer(nbytes=work_bytes + 2 * n * pb), h.buffer(nbytes=3 * n * pb)
            untouched = lambda: h.intact(srs) and h.intact(coeffs) and all(h.untouched(b) for b in (table, work, proofs))
            args = (srs.ptr.value + n * pb, table.ptr.value + n * pb, coeffs.ptr.value + n * 32, work.ptr.value + n * pb, proofs.ptr.value + n * pb)
            assert _refusals(lib, curve, log_n, *args, h.stream, untouched) > 80
            # a buffer of the library's allocator shorter than stated, in every role
            from gpu_util import DeviceBuffer
            short = DeviceBuffer(n * pb)
            try:
                SRS, TABLE, COEFFS, WORK, PROOFS = (_ptr(a) for a in args)
                sp, om = short.ptr.value, host_ptr(_omega2_wire(curve, log_n))
                for srs_, table_ in ((_ptr(sp + pb), TABLE), (SRS, _ptr(sp))):
                    assert lib.panda_kzg_open_all_setup(curve, srs_, log_n, om, table_, h.stream) == 1 and untouched(), (curve, "short buffer, setup")
                for c_, t_, w_, p_ in ((_ptr(sp + n * pb - 32), TABLE, WORK, PROOFS), (COEFFS, _ptr(sp), WORK, PROOFS), (COEFFS, TABLE, _ptr(sp), PROOFS),
                                       (COEFFS, TABLE, WORK, _ptr(sp + pb))):
                    assert lib.panda_kzg_open_all(curve, c_, t_, log_n, om, w_, work_bytes, p_, h.stream) == 1 and untouched(), (curve, "short buffer, open")
            finally:
                short.free()
        finally:
            h.close()
