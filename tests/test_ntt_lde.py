"""panda_ntt_execute_lde / panda_ntt_lde_plan: `batch` polynomials of n = 2^log_n coefficients to their evaluations on the coset g H_N of
the domain of N = B n points, B = 2^log_blowup.

The call runs B members of n points per polynomial (member i transforms c_j (g w_N^i)^j with root w_N^B) instead of one N-point coset
transform of the zero-padded polynomial.  Outputs are canonical field elements, so every comparison is of whole buffers, byte for byte.
The expected NATURAL-order value is the CPU oracle's N-point transform of the zero-padded coefficients scaled by g^j where that is cheap,
and the library's own zero-padded coset call at log2 N (itself pinned to the oracle by test_gpu_parity.py) where it is not; the
COSET_MAJOR order is the permutation [(i, k)] <- [i + B k] of it.  All three device buffers carry one guard member of a fixed byte
pattern behind the batch, which no call may touch; the coefficients must come back unchanged too."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import field_ref as fr
import oracle as po
import pyref
from gpu_util import GUARD, assert_exported, gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

MAX_BATCH = 4096  # PANDA_NTT_MAX_BATCH
MAX_LOG_BLOWUP = 4  # PANDA_NTT_LDE_MAX_LOG_BLOWUP
COSET_MAJOR, NATURAL = 0, 1
ORDERS = (COSET_MAJOR, NATURAL)
FIELD_NAME = ("bn254", "bls12_377", "bls12_381")
SHIFT = 5  # the coset generator, as in test_ntt_batch.py


def _plan(lib, log_n, log_blowup, batch, order):
    launches, flag = C.c_uint(99), C.c_uint(99)
    rc = lib.panda_ntt_lde_plan(log_n, log_blowup, batch, order, C.byref(launches), C.byref(flag))
    return rc, launches.value, flag.value


def _passes(lib, log_n):
    passes = C.c_uint(0)
    ffi.check(lib.panda_ntt_pass_plan(log_n, C.byref(passes), None), "plan")
    return passes.value


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, _ = assert_exported(("panda_ntt_execute_lde", "panda_ntt_lde_plan"))
    assert re.search(r"#define\s+PANDA_NTT_LDE_MAX_LOG_BLOWUP\s+%d\b" % MAX_LOG_BLOWUP, header)
    assert re.search(r"#define\s+PANDA_NTT_LDE_COSET_MAJOR\s+%du\b" % COSET_MAJOR, header)
    assert re.search(r"#define\s+PANDA_NTT_LDE_NATURAL\s+%du\b" % NATURAL, header)
    assert ffi.NTT_LDE_MAX_LOG_BLOWUP == MAX_LOG_BLOWUP
    assert (ffi.NTT_LDE_COSET_MAJOR, ffi.NTT_LDE_NATURAL) == ORDERS


def test_bad_arguments_are_refused_before_any_device_call():
    """every shape, pointer and overlap error returns 1 with the flag untouched -- also on a machine with no device"""
    lib = ffi.load()
    mem = np.zeros(3 << 20, np.uint8)  # three disjoint 1 MiB host ranges stand in for the buffers: nothing may dereference them
    base = mem.ctypes.data
    at = lambda off: C.c_void_p(base + off)
    coeffs, src, dst = at(0), at(1 << 20), at(2 << 20)
    one = np.array(pyref.int_to_limbs(1, 8), np.uint32)
    zero = np.zeros(8, np.uint32)
    g = C.c_void_p(one.ctypes.data)
    flag = C.c_uint(7)

    def run(field=0, log_n=4, log_blowup=2, batch=2, order=0, c=coeffs, s=src, d=dst, omega=g, fl=C.pointer(flag), shift=g):
        cfg = ffi.NttconfigurationV1(ffi.PandaMemPool(), ffi.PandaStream(), s, d, omega, log_n, fl)
        return lib.panda_ntt_execute_lde(field, cfg, c, log_blowup, batch, shift, order)

    assert run(field=3) == 1
    assert run(order=2) == 1
    assert run(log_blowup=0) == 1
    assert run(log_blowup=MAX_LOG_BLOWUP + 1) == 1
    assert run(batch=0) == 1
    assert run(batch=MAX_BATCH // 4 + 1) == 1                  # batch x B > PANDA_NTT_MAX_BATCH
    assert run(batch=MAX_BATCH, log_blowup=1, log_n=0) == 1
    assert run(log_n=26, log_blowup=2, batch=2) == 1           # 2 x 2^28 elements
    assert run(log_n=27, log_blowup=2, batch=1) == 1           # 2^29 elements
    assert run(log_n=17, log_blowup=4, batch=256) == 1         # 256 x 2^21 = 2^29
    assert run(log_n=29, log_blowup=1, batch=1) == 1
    assert run(log_n=0xFFFFFFFF) == 1
    assert run(c=None) == 1
    assert run(s=None) == 1
    assert run(d=None) == 1
    assert run(omega=None) == 1
    assert run(fl=C.POINTER(C.c_uint)()) == 1
    assert run(shift=None) == 1
    assert run(shift=C.c_void_p(zero.ctypes.data)) == 1
    # 2 polynomials of 2^4 coefficients are 1024 bytes, the extended buffers 4096 bytes: every way the ranges can meet
    assert run(c=src) == 1 and run(c=dst) == 1
    assert run(c=at((1 << 20) - 1)) == 1          # the coefficients' last byte is d_src's first
    assert run(c=at((1 << 20) + 4095)) == 1       # their first byte is d_src's last
    assert run(c=at((2 << 20) + 2048)) == 1       # inside d_dst
    assert run(s=at(512)) == 1                    # d_src begins inside the coefficients
    assert flag.value == 7
    for args in ((29, 1, 1, 0), (4, 0, 1, 0), (4, 5, 1, 0), (4, 2, 0, 0), (4, 2, MAX_BATCH // 4 + 1, 0), (4, 2, 1, 2), (26, 2, 2, 0), (27, 2, 1, 1)):
        assert lib.panda_ntt_lde_plan(*args, None, None) == 1


def test_lde_plan():
    lib = ffi.load()
    for log_n in range(0, 25):
        passes = _passes(lib, log_n)
        for log_blowup in range(1, MAX_LOG_BLOWUP + 1):
            for order in ORDERS:
                seen = set()
                for batch in (1, 2, 3, 64, 256):
                    if (batch << (log_n + log_blowup)) > (1 << 28):
                        assert lib.panda_ntt_lde_plan(log_n, log_blowup, batch, order, None, None) == 1
                        continue
                    rc, launches, flag = _plan(lib, log_n, log_blowup, batch, order)
                    assert rc == 0, (log_n, log_blowup, batch, order)
                    assert launches == 1 + passes + order
                    assert flag == (passes + order) & 1
                    seen.add((launches, flag))
                    assert lib.panda_ntt_lde_plan(log_n, log_blowup, batch, order, None, None) == 0  # either pointer may be NULL
                    only = C.c_uint(99)
                    assert lib.panda_ntt_lde_plan(log_n, log_blowup, batch, order, C.byref(only), None) == 0 and only.value == launches
                    assert lib.panda_ntt_lde_plan(log_n, log_blowup, batch, order, None, C.byref(only)) == 0 and only.value == flag
                assert len(seen) == 1, "neither the launches nor the flag depend on the batch"


# ------------------------------------------------------------------------------------------------- on the device
def _to_coset_major(natural, log_n, log_blowup):
    """(batch, N, 8) in the NATURAL order -> the COSET_MAJOR order: element (i, k) is element i + B k"""
    batch = natural.shape[0]
    return np.ascontiguousarray(natural.reshape(batch, 1 << log_n, 1 << log_blowup, 8).transpose(0, 2, 1, 3)).reshape(batch, -1, 8)


@functools.lru_cache(maxsize=None)
def _coeffs(field, log_n, batch, seed):
    x = po.gen_scalars(po.FR_OF[field], seed, batch << log_n).reshape(batch, 1 << log_n, 8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle_natural(field, log_n, log_blowup, batch, seed):
    """the oracle's value, computed once per shape and shared by the two orders: zero-pad to N, multiply element j by g^j, transform"""
    fid, n, log_big = po.FR_OF[field], 1 << log_n, log_n + log_blowup
    omega = po.root_of_unity(fid, log_big)
    pw = fr.shift_powers(field, n, SHIFT)
    out = []
    for c in _coeffs(field, log_n, batch, seed):
        padded = np.zeros((1 << log_big, 8), np.uint32)
        padded[:n] = po.f_vec(fid, po.OP_MUL, np.ascontiguousarray(c), pw)
        out.append(po.ntt(fid, padded, omega, log_big))
    out = np.stack(out)
    out.setflags(write=False)
    return out


class Harness:
    """the coefficient buffer and the two extended buffers, each with one guard member behind the batch"""

    def __init__(self, gm, field, log_n, log_blowup, batch):
        from gpu_util import DeviceBuffer
        self.lib, self.gm, self.field, self.log_n, self.log_blowup, self.batch = ffi.load(), gm, field, log_n, log_blowup, batch
        self.fid, self.n, self.big = po.FR_OF[field], 1 << log_n, 1 << (log_n + log_blowup)
        self.cbytes, self.bytes = self.n * 32, self.big * 32
        self.c = DeviceBuffer((batch + 1) * self.cbytes)
        self.a, self.b = DeviceBuffer((batch + 1) * self.bytes), DeviceBuffer((batch + 1) * self.bytes)
        self.omega = po.root_of_unity(self.fid, log_n + log_blowup)
        self.g = fr.wire_one(field, SHIFT)
        self.flag = C.c_uint(9)

    def cfg(self, src, dst, log_n=None, omega=None):
        omega = self.omega if omega is None else omega
        return ffi.NttconfigurationV1(self.gm.mem_pool, self.gm.exec_stream.raw, src, dst, C.c_void_p(omega.ctypes.data),
                                      self.log_n if log_n is None else log_n, C.pointer(self.flag))

    def fill(self, coeffs):
        coeffs = np.ascontiguousarray(coeffs, np.uint32).reshape(self.batch, self.n, 8)
        ffi.check(self.lib.panda_memset(self.c.ptr, GUARD, (self.batch + 1) * self.cbytes), "memset")
        ffi.check(self.lib.panda_memcpy(self.c.ptr, C.c_void_p(coeffs.ctypes.data), self.batch * self.cbytes), "memcpy")
        for d in (self.a, self.b):
            ffi.check(self.lib.panda_memset(d.ptr, GUARD, (self.batch + 1) * self.bytes), "memset")
        return coeffs

    def check_untouched(self, coeffs):
        """the coefficients and the three guard members are as fill() left them"""
        got = self.c.to_host(np.uint32, nbytes=self.batch * self.cbytes).reshape(self.batch, self.n, 8)
        assert np.array_equal(got, coeffs), "d_coeffs was written"
        assert (self.c.to_host(np.uint8, nbytes=self.cbytes, offset=self.batch * self.cbytes) == GUARD).all(), "bytes behind the coefficients were written"
        for d in (self.a, self.b):
            assert (d.to_host(np.uint8, nbytes=self.bytes, offset=self.batch * self.bytes) == GUARD).all(), "bytes behind the batch were written"

    def lde(self, coeffs, order):
        """one panda_ntt_execute_lde -> the (batch, N, 8) result; checks the flag against the plan, the guards and the coefficients"""
        coeffs = self.fill(coeffs)
        self.flag.value = 9
        ffi.check(self.lib.panda_ntt_execute_lde(self.field, self.cfg(self.a.ptr, self.b.ptr), self.c.ptr, self.log_blowup, self.batch,
                                                 C.c_void_p(self.g.ctypes.data), order), "lde")
        rc, launches, flag = _plan(self.lib, self.log_n, self.log_blowup, self.batch, order)
        assert rc == 0 and self.flag.value == flag
        assert launches == 1 + _passes(self.lib, self.log_n) + order
        self.check_untouched(coeffs)
        res = self.b if self.flag.value else self.a
        return res.to_host(np.uint32, nbytes=self.batch * self.bytes).reshape(self.batch, self.big, 8)

    def padded_coset_calls(self, coeffs):
        """today's route, polynomial by polynomial: zero-pad to N, the single coset call at log2 N -> (batch, N, 8) in the NATURAL order"""
        from gpu_util import DeviceBuffer
        fn = getattr(self.lib, "panda_ntt_execute_" + FIELD_NAME[self.field] + "_coset")
        sa, sb = DeviceBuffer(self.bytes), DeviceBuffer(self.bytes)
        out = []
        try:
            for c in np.ascontiguousarray(coeffs, np.uint32).reshape(self.batch, self.n, 8):
                ffi.check(self.lib.panda_memset(sa.ptr, 0, self.bytes), "memset")
                ffi.check(self.lib.panda_memcpy(sa.ptr, C.c_void_p(c.ctypes.data), self.cbytes), "memcpy")
                self.flag.value = 9
                ffi.check(fn(self.cfg(sa.ptr, sb.ptr, log_n=self.log_n + self.log_blowup), C.c_void_p(self.g.ctypes.data)), "coset")
                out.append((sb if self.flag.value else sa).to_host(np.uint32).reshape(self.big, 8))
        finally:
            sa.free()
            sb.free()
        return np.stack(out)

    def close(self):
        for d in (self.c, self.a, self.b):
            d.free()


def _check_order(h, coeffs, natural, order):
    got = h.lde(coeffs, order)
    want = natural if order == NATURAL else _to_coset_major(natural, h.log_n, h.log_blowup)
    assert np.array_equal(got, want), (h.field, h.log_n, h.log_blowup, h.batch, order)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("log_n,log_blowup,batch", [(0, 1, 3), (1, 2, 5), (3, 4, 64), (5, 3, 7), (8, 1, 5), (9, 2, 3), (10, 3, 2), (11, 2, 3),
                                                    (12, 1, 3), (13, 3, 1)])
def test_bn254_vs_oracle(gm, log_n, log_blowup, batch, order):
    """expand only; members sharing workgroups, full and ragged; one and two passes; either side of the one-member-per-workgroup
    boundary; k_ntt_pass8 with a short last pass"""
    seed = 0x6E00 + 64 * log_n + log_blowup
    h = Harness(gm, 0, log_n, log_blowup, batch)
    try:
        _check_order(h, _coeffs(0, log_n, batch, seed), _oracle_natural(0, log_n, log_blowup, batch, seed), order)
    finally:
        h.close()


@functools.lru_cache(maxsize=None)
def _padded_reference(gm, log_n, log_blowup, batch, seed):
    h = Harness(gm, 0, log_n, log_blowup, batch)
    try:
        ref = h.padded_coset_calls(_coeffs(0, log_n, batch, seed))
    finally:
        h.close()
    ref.setflags(write=False)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("log_n,log_blowup,batch", [(16, 3, 2), (17, 2, 1), (18, 1, 1), pytest.param(20, 3, 2, marks=pytest.mark.gpu_soak),
                                                    pytest.param(22, 2, 1, marks=pytest.mark.gpu_soak)])
def test_bn254_vs_zero_padded_coset_call(gm, log_n, log_blowup, batch, order):
    """the sizes whose oracle transform costs seconds, against the library's own coset call on the zero-padded polynomial at log2 N:
    the last size with j >> 16 == 0 (2 passes against 3); second-level power tables for both g and w_N with a radix-512 pass; 2^18; under
    gpu_soak the three-pass members of 2^20 and 2^22 coefficients"""
    seed = 0x6F00 + log_n
    h = Harness(gm, 0, log_n, log_blowup, batch)
    try:
        _check_order(h, _coeffs(0, log_n, batch, seed), _padded_reference(gm, log_n, log_blowup, batch, seed), order)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("log_n,log_blowup,batch", [(9, 2, 3), (12, 3, 2)])
@pytest.mark.parametrize("field", [1, 2])
def test_other_fields_vs_oracle(gm, field, log_n, log_blowup, batch, order):
    seed = 0x7000 + 32 * field + log_n
    h = Harness(gm, field, log_n, log_blowup, batch)
    try:
        _check_order(h, _coeffs(field, log_n, batch, seed), _oracle_natural(field, log_n, log_blowup, batch, seed), order)
    finally:
        h.close()


def _builds(lib):
    builds = C.c_uint64(0)
    ffi.check(lib.panda_ntt_table_builds(C.byref(builds)), "builds")
    return builds.value


@pytest.mark.gpu
def test_table_cache_is_shared_with_the_single_call(gm):
    """the members run under the single call's key for (log_n, forward, w_N^B): a _v1 call at 2^12 with root w_N^4 after an extension
    builds nothing, and neither does a second identical extension"""
    from gpu_util import DeviceBuffer
    log_n, log_blowup, batch, seed = 12, 2, 3, 0x7100
    h = Harness(gm, 0, log_n, log_blowup, batch)
    sa, sb = DeviceBuffer(h.cbytes), DeviceBuffer(h.cbytes)
    try:
        x = _coeffs(0, log_n, batch, seed)
        natural = _oracle_natural(0, log_n, log_blowup, batch, seed)
        _check_order(h, x, natural, COSET_MAJOR)
        b0 = _builds(h.lib)
        member_root = h.omega.reshape(1, 8)
        for _ in range(log_blowup):
            member_root = po.f_vec(h.fid, po.OP_SQR, member_root)
        member_root = np.ascontiguousarray(member_root.reshape(8))
        ffi.check(h.lib.panda_memcpy(sa.ptr, C.c_void_p(np.ascontiguousarray(x[0]).ctypes.data), h.cbytes), "memcpy")
        ffi.check(h.lib.panda_ntt_execute_bn254_v1(h.cfg(sa.ptr, sb.ptr, omega=member_root)), "single")
        assert _builds(h.lib) == b0, "a single call with the members' root after an extension builds nothing"
        single = (sb if h.flag.value else sa).to_host(np.uint32).reshape(h.n, 8)
        assert np.array_equal(single, po.ntt(h.fid, np.ascontiguousarray(x[0]), member_root, log_n))
        _check_order(h, x, natural, COSET_MAJOR)
        _check_order(h, x, natural, NATURAL)
        assert _builds(h.lib) == b0, "a repeated extension builds nothing"
    finally:
        sa.free()
        sb.free()
        h.close()


@pytest.mark.gpu
def test_streamed_table_fallback_applies_to_the_members(gm):
    """under the allocation-failure hook an extension of 2^17 coefficients still matches the zero-padded coset call"""
    log_n, log_blowup, batch, seed = 17, 1, 2, 0x7200
    h = Harness(gm, 0, log_n, log_blowup, batch)
    try:
        x = _coeffs(0, log_n, batch, seed)
        ref = h.padded_coset_calls(x)
        ffi.check(h.lib.panda_ntt_set_streamed_tables(3), "option")
        for order in ORDERS:
            _check_order(h, x, ref, order)
    finally:
        h.lib.panda_ntt_set_streamed_tables(0xFFFFFFFF)
        h.close()


@pytest.mark.gpu
def test_short_device_buffers_are_refused(gm):
    from gpu_util import DeviceBuffer
    log_n, log_blowup, batch, seed = 9, 2, 3, 0x7300
    h = Harness(gm, 0, log_n, log_blowup, batch)
    short_c, short_big = DeviceBuffer((batch - 1) * h.cbytes), DeviceBuffer(batch * h.bytes - h.cbytes)  # each one member of n elements short
    try:
        x = h.fill(_coeffs(0, log_n, batch, seed))
        g = C.c_void_p(h.g.ctypes.data)
        h.flag.value = 9
        assert h.lib.panda_ntt_execute_lde(0, h.cfg(short_big.ptr, h.b.ptr), h.c.ptr, log_blowup, batch, g, COSET_MAJOR) == 1
        assert h.lib.panda_ntt_execute_lde(0, h.cfg(h.a.ptr, short_big.ptr), h.c.ptr, log_blowup, batch, g, COSET_MAJOR) == 1
        assert h.lib.panda_ntt_execute_lde(0, h.cfg(h.a.ptr, h.b.ptr), short_c.ptr, log_blowup, batch, g, NATURAL) == 1
        assert h.flag.value == 9
        h.check_untouched(x)
        for d in (h.a, h.b):
            assert (d.to_host(np.uint8) == GUARD).all(), "a refused call wrote to a buffer"
        _check_order(h, x, _oracle_natural(0, log_n, log_blowup, batch, seed), NATURAL)
    finally:
        short_c.free()
        short_big.free()
        h.close()


@pytest.mark.gpu
def test_gpu_manager_helper(gm):
    log_n, log_blowup, batch, seed = 8, 2, 3, 0x7400
    x = _coeffs(0, log_n, batch, seed)
    natural = _oracle_natural(0, log_n, log_blowup, batch, seed)
    omega = po.root_of_unity(po.F_BN254_FR, log_n + log_blowup)
    polys = [np.array(c) for c in x]
    for order, want in ((ffi.NTT_LDE_COSET_MAJOR, _to_coset_major(natural, log_n, log_blowup)), (ffi.NTT_LDE_NATURAL, natural)):
        got = pgm.panda_ntt_gpu_lde(gm, polys, omega, log_n, log_blowup, fr.wire_one(0, SHIFT), order=order)
        assert len(got) == batch
        for j in range(batch):
            assert got[j].shape == (1 << (log_n + log_blowup), 8) and np.array_equal(got[j], want[j])
            assert np.array_equal(polys[j], x[j]), "the helper changed its input"
    assert pgm.panda_ntt_gpu_lde(gm, [], omega, log_n, log_blowup, fr.wire_one(0, SHIFT)) == []
