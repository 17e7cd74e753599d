"""panda_ntt_execute_batch / panda_ntt_batch_plan: many transforms of one size, field, kind and root in one call.

Every pass is launched once over all members (a member dimension in the grid of the pass kernels; members below 2^10 points share a
workgroup), with the single call's table set and one synchronisation.  NTT outputs are canonical field elements, so every comparison
is of whole buffers, byte for byte: against the CPU oracle where it is cheap, against the library's own single call (itself pinned to
the oracle by test_gpu_parity.py) where it is not.  Both device buffers carry one guard member behind the batch, which no call may touch."""
import ctypes as C
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
FORWARD, INVERSE, BITREV_OUT, INVERSE_BITREV_IN, COSET, COSET_INVERSE = range(6)
KINDS = (FORWARD, INVERSE, BITREV_OUT, INVERSE_BITREV_IN, COSET, COSET_INVERSE)
FIELD_NAME = ("bn254", "bls12_377", "bls12_381")
KIND_SUFFIX = ("_v1", "_inverse", "_bitrev_out", "_inverse_bitrev_in", "_coset", "_coset_inverse")
SHIFT = 5  # the coset generator of the tests


def _plan(lib, log_n, kind, batch):
    launches, mpw = C.c_uint(99), C.c_uint(99)
    rc = lib.panda_ntt_batch_plan(log_n, kind, batch, C.byref(launches), C.byref(mpw))
    return rc, launches.value, mpw.value


def _single_passes(lib, log_n):
    passes = C.c_uint(0)
    ffi.check(lib.panda_ntt_pass_plan(log_n, C.byref(passes), None), "plan")
    return passes.value


def _kind_passes(lib, log_n, kind):
    """passes of the plan a kind runs: the bit-reversed orderings keep the eight-bit plan at 2^18 / 2^27"""
    if kind in (BITREV_OUT, INVERSE_BITREV_IN) and log_n in (18, 27):
        return (log_n + 7) // 8
    return _single_passes(lib, log_n)


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, _ = assert_exported(("panda_ntt_execute_batch", "panda_ntt_batch_plan"))
    assert re.search(r"#define\s+PANDA_NTT_MAX_BATCH\s+%d\b" % MAX_BATCH, header)
    assert ffi.NTT_MAX_BATCH == MAX_BATCH
    assert (ffi.NTT_FORWARD, ffi.NTT_INVERSE, ffi.NTT_BITREV_OUT, ffi.NTT_INVERSE_BITREV_IN, ffi.NTT_COSET, ffi.NTT_COSET_INVERSE) == KINDS


def test_bad_arguments_are_refused_before_any_device_call():
    """every shape and pointer error returns 1 -- also on a machine with no device"""
    lib = ffi.load()
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    one = np.array(pyref.int_to_limbs(1, 8), np.uint32)
    zero = np.zeros(8, np.uint32)
    g = C.c_void_p(one.ctypes.data)
    flag = C.c_uint(7)

    def run(field=0, kind=FORWARD, batch=2, log_n=4, src=p, dst=p, omega=p, fl=C.pointer(flag), shift=None):
        cfg = ffi.NttconfigurationV1(ffi.PandaMemPool(), ffi.PandaStream(), src, dst, omega, log_n, fl)
        return lib.panda_ntt_execute_batch(field, kind, cfg, batch, shift)

    assert run(field=3) == 1
    assert run(kind=6) == 1
    assert run(batch=0) == 1
    assert run(batch=MAX_BATCH + 1) == 1
    assert run(log_n=29) == 1
    assert run(log_n=28, batch=2) == 1        # 2 x 2^28 elements
    assert run(log_n=17, batch=MAX_BATCH) == 1  # 4096 x 2^17 = 2^29
    assert run(src=None) == 1
    assert run(dst=None) == 1
    assert run(omega=None) == 1
    assert run(fl=C.POINTER(C.c_uint)()) == 1
    for kind in (COSET, COSET_INVERSE):
        assert run(kind=kind, shift=None) == 1
        assert run(kind=kind, shift=C.c_void_p(zero.ctypes.data)) == 1
        assert run(kind=kind, field=3, shift=g) == 1
    assert flag.value == 7
    for args in ((29, 0, 1), (4, 6, 1), (4, 0, 0), (4, 0, MAX_BATCH + 1), (28, 0, 2), (17, 0, MAX_BATCH)):
        assert lib.panda_ntt_batch_plan(*args, None, None) == 1


def test_batch_plan():
    lib = ffi.load()
    for log_n in range(0, 29):
        for kind in KINDS:
            seen = set()
            for batch in (1, 2, 3, 64, 4096):
                if (batch << log_n) > (1 << 28):
                    assert lib.panda_ntt_batch_plan(log_n, kind, batch, None, None) == 1
                    continue
                rc, launches, mpw = _plan(lib, log_n, kind, batch)
                assert rc == 0, (log_n, kind, batch)
                seen.add(launches)
                base = kind - 4 if kind >= COSET else kind
                assert launches == _kind_passes(lib, log_n, base) + (1 if kind >= COSET else 0), (log_n, kind, batch)
                if log_n < 10:
                    assert (mpw << log_n) >= 1024
                if log_n >= 11:
                    assert mpw == 1
                assert lib.panda_ntt_batch_plan(log_n, kind, batch, None, None) == 0  # either pointer may be NULL
            assert len(seen) == 1, "the launches of a batch do not depend on its size"
    assert _plan(lib, 8, FORWARD, 64)[2] == 4 and _plan(lib, 5, FORWARD, 64)[2] == 32


# ------------------------------------------------------------------------------------------------- on the device
def _perm(log_n):
    return np.array([int(format(k, f"0{log_n}b")[::-1], 2) if log_n else 0 for k in range(1 << log_n)])


class Harness:
    """two device buffers of batch + 1 members (the last one a guard), two of one member for the single calls"""

    def __init__(self, gm, field, log_n, batch):
        from gpu_util import DeviceBuffer
        self.lib, self.gm, self.field, self.log_n, self.batch, self.n = ffi.load(), gm, field, log_n, batch, 1 << log_n
        self.fid = po.FR_OF[field]
        self.mbytes = self.n * 32
        self.a, self.b = DeviceBuffer((batch + 1) * self.mbytes), DeviceBuffer((batch + 1) * self.mbytes)
        self.sa, self.sb = DeviceBuffer(self.mbytes), DeviceBuffer(self.mbytes)
        self.omega = po.root_of_unity(self.fid, log_n)
        self.g = fr.wire_one(field, SHIFT)
        self.flag = C.c_uint(9)

    def cfg(self, src, dst, log_n=None):
        return ffi.NttconfigurationV1(self.gm.mem_pool, self.gm.exec_stream.raw, src, dst, C.c_void_p(self.omega.ctypes.data),
                                      self.log_n if log_n is None else log_n, C.pointer(self.flag))

    def shift_ptr(self, kind):
        return C.c_void_p(self.g.ctypes.data) if kind >= COSET else None

    def batch_call(self, kind, data, batch=None):
        """one panda_ntt_execute_batch over `data` (batch, n, 8) -> (flag, outputs); checks that neither guard member was touched"""
        batch = self.batch if batch is None else batch
        data = np.ascontiguousarray(data, np.uint32).reshape(batch, self.n, 8)
        total = (self.batch + 1) * self.mbytes
        ffi.check(self.lib.panda_memset(self.a.ptr, GUARD, total), "memset")
        ffi.check(self.lib.panda_memset(self.b.ptr, GUARD, total), "memset")
        ffi.check(self.lib.panda_memcpy(self.a.ptr, C.c_void_p(data.ctypes.data), batch * self.mbytes), "memcpy")
        self.flag.value = 9
        ffi.check(self.lib.panda_ntt_execute_batch(self.field, kind, self.cfg(self.a.ptr, self.b.ptr), batch, self.shift_ptr(kind)), "batch")
        assert self.flag.value in (0, 1)
        for d in (self.a, self.b):
            guard = d.to_host(np.uint8, nbytes=total - batch * self.mbytes, offset=batch * self.mbytes)
            assert (guard == GUARD).all(), "bytes behind the batch were written"
        res = self.b if self.flag.value else self.a
        return self.flag.value, res.to_host(np.uint32, nbytes=batch * self.mbytes).reshape(batch, self.n, 8)

    def single_call(self, kind, member):
        """the single call of `kind` on one member -> (flag, output)"""
        member = np.ascontiguousarray(member, np.uint32)
        ffi.check(self.lib.panda_memcpy(self.sa.ptr, C.c_void_p(member.ctypes.data), self.mbytes), "memcpy")
        fn = getattr(self.lib, "panda_ntt_execute_" + FIELD_NAME[self.field] + KIND_SUFFIX[kind])
        cfg = self.cfg(self.sa.ptr, self.sb.ptr)
        self.flag.value = 9
        ffi.check(fn(cfg, self.shift_ptr(kind)) if kind >= COSET else fn(cfg), "single")
        res = self.sb if self.flag.value else self.sa
        return self.flag.value, res.to_host(np.uint32).reshape(self.n, 8)

    def random(self, seed, batch=None):
        batch = self.batch if batch is None else batch
        return po.gen_scalars(self.fid, seed, batch * self.n).reshape(batch, self.n, 8)

    def oracle(self, x):
        return np.stack([po.ntt(self.fid, np.ascontiguousarray(m), self.omega, self.log_n) for m in x])

    def expected_flag(self, kind):
        base = kind - 4 if kind >= COSET else kind
        return _kind_passes(self.lib, self.log_n, base) & 1

    def close(self):
        for d in (self.a, self.b, self.sa, self.sb):
            d.free()


def _forward_inverse_vs_oracle(h, seed):
    x = h.random(seed)
    want = h.oracle(x)
    flag, got = h.batch_call(FORWARD, x)
    assert flag == h.expected_flag(FORWARD)
    assert np.array_equal(got, want)
    flag, back = h.batch_call(INVERSE, got)
    assert flag == h.expected_flag(INVERSE)
    assert np.array_equal(back, x)


def _vs_single_calls(h, kind, data):
    flag, got = h.batch_call(kind, data)
    for j in range(h.batch):
        sflag, want = h.single_call(kind, data[j])
        assert flag == sflag
        assert np.array_equal(got[j], want), (h.field, h.log_n, kind, j)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,batch", [(0, 5), (1, 7), (3, 4096), (5, 33), (8, 64), (8, 5), (9, 33), (10, 33), (11, 8), (12, 13), (13, 5)])
def test_bn254_vs_oracle(gm, log_n, batch):
    """packed members with full and ragged last workgroups, the two-pass plans below 2^11, k_ntt_pass8 with a short last pass, the
    maximum batch; the plan's launch count does not depend on the batch"""
    h = Harness(gm, 0, log_n, batch)
    try:
        rc, launches, mpw = _plan(h.lib, log_n, FORWARD, batch)
        assert rc == 0 and launches == _single_passes(h.lib, log_n)
        _forward_inverse_vs_oracle(h, 0x4E00 + 64 * log_n + batch % 61)
    finally:
        h.close()


_soak = pytest.mark.gpu_soak


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,batch", [(16, 13), (17, 5), (18, 4), pytest.param(19, 3, marks=_soak), pytest.param(20, 3, marks=_soak),
                                         pytest.param(22, 2, marks=_soak)])
def test_bn254_vs_single_calls(gm, log_n, batch):
    """the sizes whose oracle transform costs seconds: every member equals the single call on it, forward and inverse"""
    h = Harness(gm, 0, log_n, batch)
    try:
        x = h.random(0x5100 + log_n)
        y = _vs_single_calls(h, FORWARD, x)
        if log_n == 16:
            assert np.array_equal(y[0], po.ntt(h.fid, np.ascontiguousarray(x[0]), h.omega, log_n))
        back = _vs_single_calls(h, INVERSE, y)
        assert np.array_equal(back, x)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field,log_n,batch,oracle", [(1, 12, 5, True), (2, 12, 5, True), (2, 9, 8, True), (1, 17, 3, False),
                                                       pytest.param(2, 20, 2, False, marks=_soak)])
def test_other_fields(gm, field, log_n, batch, oracle):
    h = Harness(gm, field, log_n, batch)
    try:
        if oracle:
            _forward_inverse_vs_oracle(h, 0x5200 + 32 * field + log_n)
        else:
            x = h.random(0x5300 + 32 * field + log_n)
            y = _vs_single_calls(h, FORWARD, x)
            assert np.array_equal(_vs_single_calls(h, INVERSE, y), x)
    finally:
        h.close()


def _other_kinds_vs_oracle(h, seed):
    x = h.random(seed)
    want = h.oracle(x)
    perm = _perm(h.log_n)
    flag, got = h.batch_call(BITREV_OUT, x)
    assert flag == h.expected_flag(BITREV_OUT)
    assert np.array_equal(got[:, perm], want)  # got[bitrev(k)] = y[k]
    flag, back = h.batch_call(INVERSE_BITREV_IN, got)
    assert flag == h.expected_flag(INVERSE_BITREV_IN)
    assert np.array_equal(back, x)
    pw = fr.shift_powers(h.field, h.n, SHIFT)
    scaled = np.stack([po.f_vec(h.fid, po.OP_MUL, np.ascontiguousarray(m), pw) for m in x])
    cwant = h.oracle(scaled)
    flag, got = h.batch_call(COSET, x)
    assert flag == h.expected_flag(COSET)
    assert np.array_equal(got, cwant)
    flag, back = h.batch_call(COSET_INVERSE, got)
    assert flag == h.expected_flag(COSET_INVERSE)
    assert np.array_equal(back, x)


@pytest.mark.gpu
@pytest.mark.parametrize("field,log_n,batch", [(0, 5, 33), (0, 9, 8), (0, 12, 5), (1, 9, 8), (2, 9, 8)])
def test_other_kinds_vs_oracle(gm, field, log_n, batch):
    """bit-reversed output = the oracle's output permuted; inverse from bit-reversed input returns the coefficients; coset forward = the
    oracle's transform of the input scaled by g^j; coset inverse returns the input"""
    h = Harness(gm, field, log_n, batch)
    try:
        _other_kinds_vs_oracle(h, 0x5400 + 32 * field + log_n)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,batch", [(17, 3), (18, 2)])
def test_other_kinds_vs_single_calls(gm, log_n, batch):
    """2^17 / 2^18: the bit-reversed kinds run other plans (radix-512 passes last, the eight-bit plan) than the natural order"""
    h = Harness(gm, 0, log_n, batch)
    try:
        x = h.random(0x5500 + log_n)
        for fwd, inv in ((BITREV_OUT, INVERSE_BITREV_IN), (COSET, COSET_INVERSE)):
            y = _vs_single_calls(h, fwd, x)
            assert h.flag.value == h.expected_flag(fwd)
            assert np.array_equal(_vs_single_calls(h, inv, y), x)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [12, 8])
def test_members_do_not_leak(gm, log_n):
    """a member of zeros, a delta member, two identical members among random ones; batch = 1 equals the single call (the guard member
    behind the batch is checked by every batch_call of this file)"""
    h = Harness(gm, 0, log_n, 8)
    try:
        x = h.random(0x5600 + log_n).copy()
        v = x[0, 3].copy()
        x[1] = 0
        x[3] = 0
        x[3, 0] = v
        x[6] = x[2]
        flag, got = h.batch_call(FORWARD, x)
        assert not got[1].any()
        assert (got[3] == v).all()
        assert np.array_equal(got[6], got[2])
        for j in (0, 2, 4, 5, 7):
            assert np.array_equal(got[j], po.ntt(h.fid, np.ascontiguousarray(x[j]), h.omega, log_n)), j
        flag1, one = h.batch_call(FORWARD, x[5:6], batch=1)
        sflag, want = h.single_call(FORWARD, x[5])
        assert flag1 == sflag and np.array_equal(one[0], want)
    finally:
        h.close()


def _builds(lib):
    builds = C.c_uint64(0)
    ffi.check(lib.panda_ntt_table_builds(C.byref(builds)), "builds")
    return builds.value


@pytest.mark.gpu
def test_table_cache_is_shared_with_the_single_call(gm):
    h = Harness(gm, 0, 14, 7)
    h2 = Harness(gm, 0, 13, 7)
    try:
        x = h.random(0x5700)
        h.single_call(FORWARD, x[0])  # whatever was cached before, this size and root now is
        b0 = _builds(h.lib)
        _, got = h.batch_call(FORWARD, x)
        assert _builds(h.lib) == b0, "a batch after a single call of the same key builds nothing"
        x2 = h2.random(0x5701)
        h2.batch_call(FORWARD, x2)
        assert _builds(h.lib) == b0 + 1, "a batch at a new size builds one table set, whatever its size"
        h2.batch_call(FORWARD, x2)
        assert _builds(h.lib) == b0 + 1
        _, want = h2.single_call(FORWARD, x2[0])
        assert _builds(h.lib) == b0 + 1, "a single call after a batch of the same key builds nothing"
        assert np.array_equal(got[0], h.single_call(FORWARD, x[0])[1])
    finally:
        h.close()
        h2.close()


@pytest.mark.gpu
def test_streamed_table_fallback_applies_to_a_batch(gm):
    """under the allocation-failure hook a batch of 2 at 2^19 (whose middle pass takes a streamed table by default) succeeds with the
    two small tables and equals the single calls"""
    h = Harness(gm, 0, 19, 2)
    try:
        x = h.random(0x5800)
        ffi.check(h.lib.panda_ntt_set_streamed_tables(3), "option")
        _vs_single_calls(h, FORWARD, x)
    finally:
        h.lib.panda_ntt_set_streamed_tables(0xFFFFFFFF)
        h.close()


@pytest.mark.gpu
def test_short_device_buffers_are_refused(gm):
    from gpu_util import DeviceBuffer
    h = Harness(gm, 0, 12, 4)
    short = DeviceBuffer(3 * h.mbytes)
    try:
        x = h.random(0x5900)
        assert h.lib.panda_ntt_execute_batch(0, FORWARD, h.cfg(short.ptr, h.b.ptr), 4, None) == 1
        assert h.lib.panda_ntt_execute_batch(0, FORWARD, h.cfg(h.a.ptr, short.ptr), 4, None) == 1
        _, got = h.batch_call(FORWARD, x)
        assert np.array_equal(got, h.oracle(x))
    finally:
        short.free()
        h.close()


@pytest.mark.gpu
def test_gpu_manager_helper(gm):
    fid, log_n = po.F_BN254_FR, 12
    om = po.root_of_unity(fid, log_n)
    polys = [po.gen_scalars(fid, 0x5A00 + j, 1 << log_n) for j in range(5)]
    want = [p.copy() for p in polys]
    flags = {pgm.panda_ntt_bn254_gpu_v1(gm, w, om, log_n) for w in want}
    flag = pgm.panda_ntt_gpu_batch(gm, polys, om, log_n)
    assert flags == {flag}
    for p, w in zip(polys, want):
        assert np.array_equal(p, w)
    back = pgm.panda_ntt_gpu_batch(gm, polys, om, log_n, kind=ffi.NTT_INVERSE)
    assert back == flag
    for j, p in enumerate(polys):
        assert np.array_equal(p, po.gen_scalars(fid, 0x5A00 + j, 1 << log_n))
    assert pgm.panda_ntt_gpu_batch(gm, [], om, log_n) == 0
