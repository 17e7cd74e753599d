"""The tabled MSM around its bucket accumulation, on the shapes at which the placement and scheduling of those kernels can go wrong.

  remap      the scatter kernels of the bucket sort take their tile from xcd_remap (panda_amd/csrc/xcd_remap.h) instead of their workgroup
             id: a map that is not a bijection sorts one tile twice and another never.  Checked on the host for every grid size, then on
             the device at 2, 4 and 16 level-1 tiles per window (fewer than 8 workgroups, not a multiple of 8, two rounds of 8); level 2's
             ragged tile counts take the remainder branch as well.
  level 3    one size for every class of cell the launch code of k3_merge distinguishes: cells that fit the ordinary variant, the dense
             half of a two-width plan that takes the wide variant, cells beyond either (the two-pass path).  The class a size reaches is
             worked out on the host from the plan panda_msm_registered_info reports, and asserted.
  fix-up     the kernels behind the accumulation as the sort hands its list to them: every bucket in several pieces, a bucket on the long
             queue, no bucket at all, and a call in point ranges, whose later ranges take the merging fix-up.
  templates  the 14-limb field, the per-window (registered-only) path that shares the level-1 column scan and the reduction, and G2.

Expected values are the linearity identity sum s_i m_i G over panda_gen_bases seeds, compared as affine points (test_msm_sort_shapes)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as po
import pyref
from gpu_util import gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm
from test_msm_sort_shapes import Problem, _scalar_set

HERE = os.path.dirname(os.path.abspath(__file__))
gpu = pytest.mark.gpu


# ------------------------------------------------------------------ the tile map, on the host

def test_xcd_remap_is_a_bijection(tmp_path):
    """the device's formula, built for the host: a bijection of [0, nwg) for every nwg from 1 to 4096, and the workgroups of one class
    (id mod 8) take consecutive tiles in the order of their ids"""
    so = str(tmp_path / "libxcd_remap_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_check", "xcd_remap_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.xcd_remap_host.argtypes = [C.c_uint, C.c_uint]
    lib.xcd_remap_host.restype = C.c_uint
    lib.xcd_remap_check.argtypes = [C.c_uint, C.c_void_p]
    lib.xcd_remap_check.restype = C.c_uint
    seen = np.zeros(4096, np.uint8)
    for nwg in range(1, 4097):
        assert lib.xcd_remap_check(nwg, seen.ctypes.data) == 0, nwg
        assert seen[:nwg].all()
    # spelled out once: 11 workgroups, classes 0..2 hold two of them, 3..7 one
    assert [lib.xcd_remap_host(i, 11) for i in range(11)] == [0, 2, 4, 6, 7, 8, 9, 10, 1, 3, 5]
    assert [lib.xcd_remap_host(i, 5) for i in range(5)] == [0, 1, 2, 3, 4]
    assert [lib.xcd_remap_host(i, 16) for i in range(16)] == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15]


# ------------------------------------------------------------------ device cases

class Tabled(Problem):
    """Problem with the window width of the tables chosen by the test (0: the library's)"""

    def __init__(self, gm, curve, k, seed, window_bits=0):
        from gpu_util import NULL_STREAM, DeviceBuffer
        from test_msm_sort_shapes import INFO
        self.lib, self.gm, self.curve, self.k, self.n, self.members, self.seed = ffi.load(), gm, curve, k, 1 << k, 1, seed
        self.entry, aff, self.res, fr = INFO[curve]
        self.db, self.ds, self.dr = DeviceBuffer(self.n * aff), DeviceBuffer(self.n * 32), DeviceBuffer(self.res)
        ffi.check(self.lib.panda_gen_bases(curve, seed, 0, self.n, self.db.ptr, NULL_STREAM), "gen")
        ffi.check(self.lib.panda_msm_precompute_bases(curve, self.db.ptr, k, window_bits, gm.exec_stream.raw), "precompute")
        tables, bits = C.c_uint(0), C.c_uint(0)
        ffi.check(self.lib.panda_msm_registered_info(self.db.ptr, C.byref(tables), C.byref(bits), None), "info")
        assert tables.value >= 2 and bits.value >= 9, "the call must take the tabled path"
        self.tables, self.window_bits = tables.value, bits.value
        self.random = po.gen_scalars(fr, seed + 1, self.n)


def _check(p, names, calls=2):
    for name in names:
        rows = _scalar_set(p.curve, name, p.random, p.window_bits)
        p.upload(0, rows)
        got = [p.single() for _ in range(calls)]
        assert got[0] == p.expected(name, rows), (p.curve, p.k, name)
        assert all(g == got[0] for g in got), (p.curve, p.k, name)


@gpu
@pytest.mark.parametrize("k", [14, 15, 17])
def test_remapped_tiles(gm, k):
    """2, 4 and 16 level-1 tiles per window"""
    p = Tabled(gm, 0, k, 0x7A10 + k)
    try:
        assert (p.n + 8191) // 8192 == {14: 2, 15: 4, 17: 16}[k]
        _check(p, ("equal", "alternating", "last_three", "uniform"))
    finally:
        p.close()


K3_CAP = 16384  # entries a 1024-thread workgroup of k3_merge reads at once (16 per thread); the wide variant reads twice that


def _level3_geometry(log_n, tables, window_bits, total_bits=255):
    """What msm_sort.hip's tabled_geom and sort3 make of a BN254 plan (254 scalar bits and one for the signed digits' carry): the mean
    entries of a level-3 cell in the dense and in the sparse half of the bucket space for uniform scalars, and whether the dense half
    is merged by the wide variant."""
    W = -(-total_bits // window_bits)
    base, rem = divmod(total_bits, W)
    widths = [base + 1] * rem + [base] * (W - rem)
    assert W == tables and widths[0] == window_bits, "the plan the library reports is not the one this test models"
    B = window_bits - 1
    b3 = min(7, 31 - log_n, B)
    while b3 > 3 and ((W << log_n) >> (B - b3)) > K3_CAP * 4 // 5:
        b3 -= 1
    n = 1 << log_n
    dense = sum(n / 2.0 ** (w - 1) for w in widths) * 2 ** b3
    sparse = sum(n / 2.0 ** (w - 1) for w in widths if w == window_bits) * 2 ** b3
    two_widths = min(widths) + 1 == window_bits
    wide = two_widths and K3_CAP * 0.8 < dense <= 2 * K3_CAP * 0.8
    return dense, sparse, wide, 1 << (B - b3)


@gpu
@pytest.mark.parametrize("k,wbits,want", [(17, 16, "fits"), (16, 11, "wide"), (18, 14, "wide_launch_small_cells"), (18, 12, "oversized"), (17, 10, "oversized_both_halves")])
def test_level3_cell_classes(gm, k, wbits, want):
    """fits: every cell at most 16 Ki entries, the ordinary variant.  wide: the dense half holds 16 Ki .. 32 Ki entries per cell and takes
    the wide variant (64 cells: fewer than the chip has compute units), the sparse half the ordinary one.  wide_launch_small_cells: 256
    cells through the wide variant, of just under 16 Ki entries.  oversized: 31 Ki entries per dense cell in a plan the wide variant is
    not chosen for -- the two-pass path of the ordinary variant.  oversized_both_halves: cells of 62 Ki entries, beyond both."""
    p = Tabled(gm, 0, k, 0x7B00 + 32 * k + wbits, window_bits=wbits)
    try:
        dense, sparse, wide, cells = _level3_geometry(k, p.tables, p.window_bits)
        sd = 3 * dense ** 0.5  # the counts of uniform scalars are Poisson: three standard deviations
        reached = {
            "fits": not wide and dense + sd <= K3_CAP,
            "wide": wide and K3_CAP < dense - sd and dense + sd <= 2 * K3_CAP and sparse + sd <= K3_CAP and cells // 2 < 256,
            "wide_launch_small_cells": wide and dense + sd <= K3_CAP and cells // 2 >= 256,
            "oversized": not wide and K3_CAP < dense - sd,
            "oversized_both_halves": not wide and 2 * K3_CAP < sparse - sd,
        }
        assert reached[want], (want, dense, sparse, wide, cells)
        _check(p, ("uniform", "equal"))
    finally:
        p.close()


@gpu
def test_fixup_every_bucket_in_pieces(gm):
    """chunks of 16 entries at 2^13 points: a bucket of the uniform set that holds more than a few entries is cut into pieces, the equal
    set's one bucket per window into 512 (the long queue)"""
    p = Tabled(gm, 0, 13, 0x7C10)
    try:
        ffi.check(p.lib.panda_msm_set_chunk_entries(16), "chunk")
        _check(p, ("uniform", "alternating", "equal", "one_window"))
    finally:
        p.lib.panda_msm_set_chunk_entries(0)
        p.close()


@gpu
def test_fixup_long_queue_and_empty_buckets(gm):
    """equal: 2^16 entries in one bucket per window, hundreds of chunks -- the long queue;
    last_three: a handful of buckets among empty ones;  zero: every bucket empty, the identity must come out"""
    p = Tabled(gm, 0, 16, 0x7C20)
    try:
        _check(p, ("equal", "last_three", "zero"))
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("k", [15, 18])
def test_fixup_beside_point_ranges(gm, k):
    """panda_msm_execute_from_host with three ranges.  2^15: the library runs ranges of at least 2^16 points, so this is one range through
    the pipeline's entry;  2^18: 2^16 + 2^16 + 2^17 points, the later ranges merged into the first one's buckets by k_fixup<MERGE>.
    The same point as the single call either way."""
    p = Tabled(gm, 0, k, 0x7C30 + k)
    try:
        rows = p.random.copy()
        rows[p.n // 3:p.n // 3 + 3000] = rows[5]  # a run of equal scalars: a bucket of thousands of entries inside one range
        rows[::7] = 0
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        want = p.expected("mixed", rows)
        p.upload(0, rows)
        assert p.single() == want
        ffi.check(p.lib.panda_memset(p.ds.ptr, 0xEE, p.n * 32), "memset")
        ffi.check(p.lib.panda_memset(p.dr.ptr, 0xA5, p.res), "memset")
        ffi.check(p.lib.panda_msm_execute_from_host(0, p._cfg(), C.c_void_p(rows.ctypes.data), 3, gm.h2d_stream.raw), "from host")
        assert p._results()[0] == want
        assert p.single() == want  # the scalars the call uploaded
    finally:
        p.close()


@gpu
def test_14_limb_curve(gm):
    p = Tabled(gm, 1, 14, 0x7D10)
    try:
        _check(p, ("uniform", "equal", "last_three", "zero"))
    finally:
        p.close()


@gpu
def test_registered_only_per_window_path(gm):
    """BN254 at 2^16 with converted bases and no tables: a list per window -- the level-1 column scan and the reduction over several lists"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    lib = ffi.load()
    k, seed = 16, 0x7D20
    n = 1 << k
    db, ds, dr = DeviceBuffer(n * 64), DeviceBuffer(n * 32), DeviceBuffer(96)
    try:
        ffi.check(lib.panda_gen_bases(0, seed, 0, n, db.ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_msm_register_bases(0, db.ptr, k, gm.exec_stream.raw), "register")
        tables = C.c_uint(99)
        ffi.check(lib.panda_msm_registered_info(db.ptr, C.byref(tables), None, None), "info")
        assert tables.value <= 1, "registered without tables"
        random = po.gen_scalars(po.F_BN254_FR, seed + 1, n)
        cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, db.ptr, ds.ptr, dr.ptr, k, pgm.JACOBIAN)
        for name in ("uniform", "equal", "last_three"):
            rows = np.ascontiguousarray(_scalar_set(0, name, random, 16), dtype=np.uint32)
            ffi.check(lib.panda_memcpy(ds.ptr, C.c_void_p(rows.ctypes.data), n * 32), "memcpy")
            ffi.check(lib.panda_memset(dr.ptr, 0xA5, 96), "memset")
            ffi.check(lib.panda_msm_execute_bn254(cfg), "msm")
            assert (po.to_affine(0, dr.to_host()) == po.expected_from_linearity(0, seed, rows)).all(), name
    finally:
        lib.panda_msm_unregister_bases(db.ptr)
        for d in (db, ds, dr):
            d.free()


@gpu
def test_bn254_g2_tabled(gm):
    """2^12 G2 points with tables: the Fq2 instance of the same kernels"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    lib = ffi.load()
    k, seed = 12, 0x7D30
    n = 1 << k
    db, ds, dr = DeviceBuffer(n * 128), DeviceBuffer(n * 32), DeviceBuffer(192)
    try:
        ffi.check(lib.panda_gen_bases(3, seed, 0, n, db.ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_msm_precompute_bases(3, db.ptr, k, 0, gm.exec_stream.raw), "precompute")
        tables = C.c_uint(0)
        ffi.check(lib.panda_msm_registered_info(db.ptr, C.byref(tables), None, None), "info")
        assert tables.value >= 2
        random = po.gen_scalars(po.F_BN254_FR, seed + 1, n)
        cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, db.ptr, ds.ptr, dr.ptr, k, pgm.JACOBIAN)
        for name in ("uniform", "equal"):
            rows = np.ascontiguousarray(_scalar_set(0, name, random, 12), dtype=np.uint32)
            ffi.check(lib.panda_memcpy(ds.ptr, C.c_void_p(rows.ctypes.data), n * 32), "memcpy")
            ffi.check(lib.panda_memset(dr.ptr, 0xA5, 192), "memset")
            ffi.check(lib.panda_msm_execute_bn254_g2(cfg), "msm")
            k_sum = pyref.limbs_to_int(po.linear_combination(0, seed, rows))
            assert pyref.g2_decode_jacobian(dr.to_host().view(np.uint32)) == pyref.g2_mul(k_sum, pyref.G2_GEN), name
    finally:
        lib.panda_msm_unregister_bases(db.ptr)
        for d in (db, ds, dr):
            d.free()
