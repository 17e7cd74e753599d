"""panda_msm_execute_batch / panda_msm_batch_plan: many scalar vectors over one base set in one call.

With precomputed tables a group of 2^g members runs as ONE MSM of 2^g n scalars whose bucket id carries the member index (one sort, one
accumulation, one reduction that emits 2^g results); without tables the members run one after the other.  Expected values are the
linearity identity sum s_i m_i G over panda_gen_bases seeds (O(n) on the CPU); results are compared as affine points, never as raw bytes
(Jacobian / homogeneous coordinates are representatives, and bucket order follows wave scheduling)."""
import ctypes as C
import re

import numpy as np
import pytest

import field_ref as fr
import oracle as po
import pyref
import pyref_bls377_g2 as g377
import pyref_bls381_g2 as g381
from gpu_util import assert_exported, gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

MAX_BATCH = 1024  # PANDA_MSM_MAX_BATCH
CURVES = (0, 1, 2, 3, 4, 6)
# curve id -> single-call entry point, affine base bytes, result bytes, oracle curve of the scalar field's linear combination, scalar field id
INFO = {
    0: ("panda_msm_execute_bn254", 64, 96, po.BN254, po.F_BN254_FR),
    1: ("panda_msm_execute_bls12_377", 96, 144, po.BLS12_377, po.F_BLS377_FR),
    2: ("panda_msm_execute_bls12_381", 96, 144, po.BLS12_381, po.F_BLS381_FR),
    3: ("panda_msm_execute_bn254_g2", 128, 192, po.BN254, po.F_BN254_FR),
    4: ("panda_msm_execute_bls12_381_g2", 192, 288, po.BLS12_381, po.F_BLS381_FR),
    6: ("panda_msm_execute_bls12_377_g2", 192, 288, po.BLS12_377, po.F_BLS377_FR),
}


def _plan(lib, curve, log_n, window_bits, batch):
    gl, seq = C.c_uint(99), C.c_uint(99)
    rc = lib.panda_msm_batch_plan(curve, log_n, window_bits, batch, C.byref(gl), C.byref(seq))
    return rc, gl.value, seq.value


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, _ = assert_exported(("panda_msm_execute_batch", "panda_msm_batch_plan"))
    assert re.search(r"#define\s+PANDA_MSM_MAX_BATCH\s+%d\b" % MAX_BATCH, header)


def test_bad_arguments_are_refused_before_any_device_call():
    """batch == 0, the unused curve id 5, curve 7 and NULL buffers return 1 -- also on a machine with no device"""
    lib = ffi.load()
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    mk = lambda b, s, r: ffi.MSMConfiguration(ffi.PandaMemPool(), ffi.PandaStream(), b, s, r, 2, pgm.JACOBIAN)
    assert lib.panda_msm_execute_batch(0, mk(p, p, p), 0) == 1
    assert lib.panda_msm_execute_batch(5, mk(p, p, p), 2) == 1
    assert lib.panda_msm_execute_batch(7, mk(p, p, p), 2) == 1
    assert lib.panda_msm_execute_batch(0, mk(None, p, p), 2) == 1
    assert lib.panda_msm_execute_batch(0, mk(p, None, p), 2) == 1
    assert lib.panda_msm_execute_batch(0, mk(p, p, None), 2) == 1
    assert lib.panda_msm_execute_batch(0, mk(p, p, p), MAX_BATCH + 1) == 1
    for args in ((5, 16, 0, 4), (7, 16, 0, 4), (0, 27, 0, 4), (0, 16, 0, 0), (0, 16, 0, MAX_BATCH + 1), (0, 16, 3, 4), (0, 16, 25, 4)):
        assert lib.panda_msm_batch_plan(*args, None, None) == 1


def test_batch_plan_is_consistent_and_fuses_where_it_matters():
    lib = ffi.load()
    batches = (1, 2, 3, 5, 13, 16, 64, 1000)
    fused_somewhere = 0
    for curve in CURVES:
        for log_n in range(10, 27):
            for wb in (0, 12, 16, 20):
                prev = 0
                for batch in batches:
                    rc, gl, seq = _plan(lib, curve, log_n, wb, batch)
                    assert rc == 0, (curve, log_n, wb, batch)
                    assert log_n + gl <= 26
                    assert (1 << gl) <= batch
                    assert -(-batch // (1 << gl)) <= seq <= batch
                    if batch == 1:
                        assert (gl, seq) == (0, 1)
                    if gl == 0:
                        assert seq == batch
                    assert gl >= prev, "a larger batch must never get a smaller group"
                    prev = gl
                    fused_somewhere += gl > 0
    assert fused_somewhere
    # the sizes the feature is for: a PLONK / halo2 round of 2^16-point commitments
    assert _plan(lib, 0, 16, 0, 64)[1] >= 4
    assert _plan(lib, 4, 16, 0, 16)[1] >= 4
    # 13 members in power-of-two groups of at most 2^gl
    rc, gl, seq = _plan(lib, 0, 16, 0, 13)
    assert rc == 0 and gl == 3 and seq == 3  # 8 + 4 + 1
    assert lib.panda_msm_batch_plan(0, 16, 0, 13, None, None) == 0  # either pointer may be NULL


# ------------------------------------------------------------------------------------------------- on the device
def _decode(curve, raw, coord=pgm.JACOBIAN):
    """a result of the C ABI as a comparable affine point"""
    proj = coord == pgm.PROJECTIVE
    w = np.ascontiguousarray(raw).view(np.uint32)
    if curve <= 2:
        return (po.hom_to_affine(curve, w) if proj else po.to_affine(curve, w)).tobytes()
    if curve == 3:
        return pyref.g2_decode_homogeneous(w) if proj else pyref.g2_decode_jacobian(w)
    return (g381 if curve == 4 else g377).decode(raw, proj)


def _expected(curve, seed_b, scalars):
    lin = INFO[curve][3]
    if curve <= 2:
        return po.expected_from_linearity(curve, seed_b, scalars).tobytes()
    k = pyref.limbs_to_int(po.linear_combination(lin, seed_b, scalars))
    if curve == 3:
        return pyref.g2_mul(k, pyref.G2_GEN)
    g2 = g381 if curve == 4 else g377
    return g2.mul(k, g2.GEN)


class Batch:
    """device bases of `curve` (seed -> panda_gen_bases), `batch` scalar vectors in one device buffer, a results buffer"""

    def __init__(self, gm, curve, k, batch, seed, tables=True, window_bits=0):
        from gpu_util import NULL_STREAM, DeviceBuffer
        self.lib, self.gm, self.curve, self.k, self.n, self.batch, self.seed = ffi.load(), gm, curve, k, 1 << k, batch, seed
        self.entry, self.aff, self.res = INFO[curve][:3]
        self.db, self.ds = DeviceBuffer(self.n * self.aff), DeviceBuffer(batch * self.n * 32)
        self.dr, self.dr1 = DeviceBuffer(batch * self.res), DeviceBuffer(self.res)
        ffi.check(self.lib.panda_gen_bases(curve, seed, 0, self.n, self.db.ptr, NULL_STREAM), "gen")
        ffi.check(self.lib.panda_gen_scalars(curve, seed + 1, 0, batch * self.n, self.ds.ptr, NULL_STREAM), "gen")
        if tables is True:
            ffi.check(self.lib.panda_msm_precompute_bases(curve, self.db.ptr, k, window_bits, gm.exec_stream.raw), "precompute")
        elif tables is False:
            ffi.check(self.lib.panda_msm_register_bases(curve, self.db.ptr, k, gm.exec_stream.raw), "register")
        self.scalars = np.ascontiguousarray(self.ds.to_host().reshape(batch, self.n, 8))

    def set_member(self, j, rows):
        self.scalars[j] = rows
        ffi.check(self.lib.panda_memcpy(C.c_void_p(self.ds.ptr.value + j * self.n * 32), C.c_void_p(self.scalars[j].ctypes.data), self.n * 32), "memcpy")

    def window_bits(self):
        tables, bits = C.c_uint(0), C.c_uint(0)
        ffi.check(self.lib.panda_msm_registered_info(self.db.ptr, C.byref(tables), C.byref(bits), None), "info")
        return tables.value, bits.value

    def group_log(self):
        rc, gl, seq = _plan(self.lib, self.curve, self.k, self.window_bits()[1], self.batch)
        assert rc == 0
        return gl, seq

    def cfg(self, results, coord=pgm.JACOBIAN, scalars=None):
        return ffi.MSMConfiguration(self.gm.mem_pool, self.gm.exec_stream.raw, self.db.ptr, scalars or self.ds.ptr, results, self.k, coord)

    def run(self, coord=pgm.JACOBIAN):
        ffi.check(self.lib.panda_memset(self.dr.ptr, 0xA5, self.batch * self.res), "memset")
        ffi.check(self.lib.panda_msm_execute_batch(self.curve, self.cfg(self.dr.ptr, coord), self.batch), "batch")
        raw = self.dr.to_host(np.uint8).reshape(self.batch, self.res)
        return [_decode(self.curve, raw[j], coord) for j in range(self.batch)], raw

    def single(self, j, coord=pgm.JACOBIAN):
        cfg = self.cfg(self.dr1.ptr, coord, C.c_void_p(self.ds.ptr.value + j * self.n * 32))
        ffi.check(getattr(self.lib, self.entry)(cfg), "msm")
        return _decode(self.curve, self.dr1.to_host(np.uint8), coord)

    def expected(self, j):
        return _expected(self.curve, self.seed, self.scalars[j])

    def close(self):
        self.lib.panda_msm_unregister_bases(self.db.ptr)
        for d in (self.db, self.ds, self.dr, self.dr1):
            d.free()


def _check_all(b, coords=(pgm.JACOBIAN, pgm.PROJECTIVE), singles=True):
    want = [b.expected(j) for j in range(b.batch)]
    for coord in coords:
        got, _ = b.run(coord)
        for j in range(b.batch):
            assert got[j] == want[j], (b.curve, b.k, b.batch, coord, j)
    if singles:
        for j in range(b.batch):
            assert b.single(j) == want[j]
    assert (b.ds.to_host().reshape(b.batch, b.n, 8) == b.scalars).all()  # the scalars are never modified


_soak = pytest.mark.gpu_soak


@pytest.mark.gpu
@pytest.mark.parametrize("k,batch", [(14, 13), (16, 8), pytest.param(14, 1, marks=_soak), pytest.param(14, 2, marks=_soak), pytest.param(14, 3, marks=_soak),
                                     pytest.param(14, 8, marks=_soak), pytest.param(16, 1, marks=_soak), pytest.param(16, 2, marks=_soak),
                                     pytest.param(16, 3, marks=_soak), pytest.param(16, 13, marks=_soak)])
def test_fused_bn254(gm, k, batch):
    """tables, both coordinate types: every member equals the linearity value and the single call on that member; the plan says the
    batch IS fused (a silent loop of single calls cannot pass), and 13 members run as 8 + 4 + 1"""
    b = Batch(gm, 0, k, batch, 0xBA00 + 16 * k + batch)
    try:
        tables, bits = b.window_bits()
        assert tables >= 2 and bits > 0
        gl, seq = b.group_log()
        if batch >= 2:
            assert gl >= 1 and seq < batch
        else:
            assert (gl, seq) == (0, 1)
        _check_all(b)
        if batch >= 2:  # observable difference to a loop of single calls: a fused batch reports its last group's device time only
            ffi.check(b.lib.panda_msm_set_phase_timing(2), "timing")
            try:
                b.run()
                ms = (C.c_float * 8)()
                ffi.check(b.lib.panda_msm_last_phase_ms(ms), "phase")
                assert ms[7] > 0 and ms[3] == 0
            finally:
                b.lib.panda_msm_set_phase_timing(0)
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("curve,k", [(1, 14), (4, 12), (6, 12), pytest.param(2, 14, marks=_soak), pytest.param(3, 14, marks=_soak),
                                     pytest.param(4, 16, marks=_soak), pytest.param(6, 16, marks=_soak)])
def test_fused_other_curves(gm, curve, k):
    """the 14-limb field (curve 1) and the Ext2 curves (4, 6), batch 5 = 4 + 1"""
    b = Batch(gm, curve, k, 5, 0xBB00 + 32 * curve + k)
    try:
        gl, seq = b.group_log()
        assert gl == 2 and seq == 2
        _check_all(b)
    finally:
        b.close()


@pytest.mark.gpu
def test_members_that_stress_the_sort(gm):
    """an all-zero vector (identity, Z == 0), all-equal scalars (one long bucket per window), all r - 1, two identical members, a vector
    with only its last scalar non-zero -- among ordinary random members of the same group: a member's buckets must not leak"""
    k, batch = 14, 8
    b = Batch(gm, 0, k, batch, 0xBC00)
    try:
        assert b.group_log() == (3, 1)
        n = b.n
        b.set_member(1, np.zeros((n, 8), np.uint32))
        b.set_member(3, np.tile(b.scalars[0][5], (n, 1)))
        b.set_member(4, np.tile(fr.wire_one(0, -1), (n, 1)))
        b.set_member(5, b.scalars[0])
        last = np.zeros((n, 8), np.uint32)
        last[n - 1] = b.scalars[2][7]
        b.set_member(6, last)
        want = [b.expected(j) for j in range(batch)]
        for coord in (pgm.JACOBIAN, pgm.PROJECTIVE):
            got, raw = b.run(coord)
            words = raw.view(np.uint32).reshape(batch, 24)
            assert not words[1, 16:24].any()  # Z == 0: the identity
            for j in range(batch):
                if j != 1:
                    assert words[j, 16:24].any() and got[j] == want[j], (coord, j)
            assert got[5] == got[0]
        for j in (3, 4, 6):
            assert b.single(j) == want[j]
    finally:
        b.close()


@pytest.mark.gpu
def test_more_than_one_group_in_order(gm):
    """a batch larger than the largest group: results stay in member order across the group boundaries"""
    lib = ffi.load()
    k = 16
    top = _plan(lib, 0, k, 0, MAX_BATCH)[1]
    batch = (1 << top) + 5  # one full group, then 4 + 1
    b = Batch(gm, 0, k, batch, 0xBD00)
    try:
        gl, seq = b.group_log()
        assert gl == top and seq == 3
        _check_all(b, coords=(pgm.JACOBIAN,), singles=False)
    finally:
        b.close()


@pytest.mark.gpu
def test_results_to_device_pinned_and_pageable_memory(gm):
    k, batch = 14, 3
    b = Batch(gm, 0, k, batch, 0xBE00)
    host = C.c_void_p()
    try:
        want = [b.expected(j) for j in range(batch)]
        assert b.run()[0] == want  # device memory
        ffi.check(b.lib.panda_malloc_host(C.byref(host), batch * 96), "malloc_host")
        C.memset(host, 0xA5, batch * 96)
        ffi.check(b.lib.panda_msm_execute_batch(0, b.cfg(host), batch), "batch")
        raw = np.frombuffer((C.c_uint8 * (batch * 96)).from_address(host.value), dtype=np.uint8).copy().reshape(batch, 96)
        assert [_decode(0, raw[j]) for j in range(batch)] == want
        out = np.full(batch * 96, 0xA5, np.uint8)  # pageable
        ffi.check(b.lib.panda_msm_execute_batch(0, b.cfg(C.c_void_p(out.ctypes.data)), batch), "batch")
        assert [_decode(0, out.reshape(batch, 96)[j]) for j in range(batch)] == want
    finally:
        if host:
            b.lib.panda_free_host(host)
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [None, False])
def test_unfused_paths(gm, tables):
    """unregistered bases, and bases registered without tables: the members run one after the other -- correct results, and the phase
    timers read like a single call's (a fused batch reports a total only)"""
    k, batch = 12, 3
    b = Batch(gm, 0, k, batch, 0xBF00, tables=tables)
    try:
        if tables is None:
            assert b.lib.panda_msm_registered_info(b.db.ptr, None, None, None) != 0
        else:
            assert b.window_bits() == (1, 0)  # the converted copy only: nothing to fuse
        ffi.check(b.lib.panda_msm_set_phase_timing(2), "timing")
        try:
            _check_all(b)
            ms = (C.c_float * 8)()
            ffi.check(b.lib.panda_msm_last_phase_ms(ms), "phase")
            assert ms[3] > 0  # "accumulate" of the last member's own call
        finally:
            b.lib.panda_msm_set_phase_timing(0)
    finally:
        b.close()


@pytest.mark.gpu
def test_stale_registration_is_dropped_and_the_batch_answered_from_the_buffer(gm):
    from gpu_util import NULL_STREAM
    k, batch = 14, 4
    b = Batch(gm, 0, k, batch, 0xC000)
    try:
        assert b.group_log()[0] == 2
        assert b.run()[0] == [b.expected(j) for j in range(batch)]
        new_seed = 0xC0FF
        ffi.check(b.lib.panda_gen_bases(0, new_seed, 0, b.n, b.db.ptr, NULL_STREAM), "gen")  # other bases in the registered buffer
        got, _ = b.run()
        assert got == [_expected(0, new_seed, b.scalars[j]) for j in range(batch)]
        assert b.lib.panda_msm_registered_info(b.db.ptr, None, None, None) != 0  # the registration is gone
    finally:
        b.close()


@pytest.mark.gpu
def test_bad_arguments_on_the_device(gm):
    from gpu_util import DeviceBuffer
    k, batch = 12, 4
    b = Batch(gm, 0, k, batch, 0xC100)
    short_s, short_r, big = DeviceBuffer((batch - 1) * b.n * 32), DeviceBuffer((batch - 1) * 96), DeviceBuffer(MAX_BATCH * 96 + 96)
    try:
        lib = b.lib
        mk = lambda s, r, log_n=k: ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, b.db.ptr, s, r, log_n, pgm.JACOBIAN)
        assert lib.panda_msm_execute_batch(0, mk(b.ds.ptr, b.dr.ptr, 27), batch) == 1
        assert lib.panda_msm_execute_batch(0, mk(short_s.ptr, b.dr.ptr), batch) == 1   # scalars one member short
        assert lib.panda_msm_execute_batch(0, mk(b.ds.ptr, short_r.ptr), batch) == 1   # results one member short
        assert lib.panda_msm_execute_batch(0, mk(b.ds.ptr, big.ptr), MAX_BATCH + 1) == 1
        assert lib.panda_msm_execute_batch(0, mk(b.ds.ptr, b.dr.ptr), 0) == 1
        assert b.run()[0] == [b.expected(j) for j in range(batch)]  # and the next valid call is still correct
    finally:
        for d in (short_s, short_r, big):
            d.free()
        b.close()


@pytest.mark.gpu
def test_gpu_manager_batch_helper(gm):
    """panda_msm_gpu_batch_with_cached_bases (one library call) against the existing helper that issues one call per vector"""
    k = 14
    n = 1 << k
    bases = po.gen_bases(po.BN254, 0xC200, n)
    vectors = [po.gen_scalars(po.F_BN254_FR, 0xC201 + j, n) for j in range(5)]
    idx = gm.add_cached_bases(bases)
    gm.precompute_cached_bases(idx)
    one_call = pgm.panda_msm_gpu_batch_with_cached_bases(gm, vectors, idx)
    per_vector = pgm.panda_msm_bn254_gpu_with_cached_bases_batched(gm, vectors, idx)
    assert len(one_call) == len(per_vector) == 5
    for j in range(5):
        assert one_call[j].size == 96
        assert _decode(0, one_call[j]) == _decode(0, per_vector[j]) == po.expected_from_linearity(po.BN254, 0xC200, vectors[j]).tobytes()
    assert pgm.panda_msm_gpu_batch_with_cached_bases(gm, [], idx) == []
