"""The tabled (precomputed window tables) MSM on the shapes its three-level bucket sort is most likely to get wrong.

The sort's scatter kernels stage a tile in LDS grouped by partition and write it out as runs; what breaks first when those kernels change is
a ragged last tile, a run that covers a whole tile (every entry in one partition: the longest runs and the worst same-address ranking),
runs of a few entries (bytes written singly at the ends of a run, as dwords inside it), empty tiles and empty cells.  So: sizes from a
fraction of one tile to many tiles per window, and scalar sets from "everything in one bucket" to uniform.  Expected values are the
linearity identity sum s_i m_i G over panda_gen_bases seeds (O(n) on the CPU oracle); results are compared as affine points -- the raw
Jacobian bytes are one representative of many and the order inside a bucket follows wave scheduling, so they get no assertion."""
import ctypes as C

import numpy as np
import pytest

import field_ref as fr
import oracle as po
from gpu_util import gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

pytestmark = pytest.mark.gpu

# curve id -> single-call entry point, affine base bytes, result bytes, scalar field id
INFO = {
    0: ("panda_msm_execute_bn254", 64, 96, po.F_BN254_FR),
    1: ("panda_msm_execute_bls12_377", 96, 144, po.F_BLS377_FR),
}
SETS = ("equal", "one_window", "zero", "r_minus_1", "alternating", "last_three", "uniform")


def _scalar_set(curve, name, random_rows, window_bits):
    """(n, 8) wire-form scalars of set `name`; random_rows are uniform scalars of the same shape"""
    n = random_rows.shape[0]
    if name == "uniform":
        return random_rows.copy()
    if name == "equal":
        return np.tile(random_rows[5 % n], (n, 1))
    if name == "zero":
        return np.zeros((n, 8), np.uint32)
    if name == "r_minus_1":
        return np.tile(fr.wire_one(curve, -1), (n, 1))
    if name == "alternating":
        out = np.empty((n, 8), np.uint32)
        out[0::2] = random_rows[1 % n]
        out[1::2] = random_rows[2 % n]
        return out
    if name == "last_three":
        out = np.zeros((n, 8), np.uint32)
        out[n - 3:] = random_rows[n - 3:]
        return out
    assert name == "one_window"
    # a digit below 2^7 at bit offsets a window apart: below half of any window of a plan of window_bits >= 9 bits (its windows are that
    # wide or one bit narrower), so the signed recoding neither carries nor borrows -- one non-zero window per scalar (two where the digit
    # straddles a boundary of a plan with two widths), every window in turn
    windows = 248 // window_bits
    palette = np.stack([fr.wire_one(curve, (1 + (37 * j) % 100) << (window_bits * (j % windows))) for j in range(8 * windows)])
    return palette[np.arange(n) % len(palette)]


class Problem:
    """device bases of `curve` (seed -> panda_gen_bases) with precomputed tables, `members` scalar vectors in one device buffer"""

    def __init__(self, gm, curve, k, seed, members=1):
        from gpu_util import NULL_STREAM, DeviceBuffer
        self.lib, self.gm, self.curve, self.k, self.n, self.members, self.seed = ffi.load(), gm, curve, k, 1 << k, members, seed
        self.entry, aff, self.res, fid = INFO[curve]
        self.db, self.ds, self.dr = DeviceBuffer(self.n * aff), DeviceBuffer(members * self.n * 32), DeviceBuffer(members * self.res)
        ffi.check(self.lib.panda_gen_bases(curve, seed, 0, self.n, self.db.ptr, NULL_STREAM), "gen")
        ffi.check(self.lib.panda_msm_precompute_bases(curve, self.db.ptr, k, 0, gm.exec_stream.raw), "precompute")
        tables, bits = C.c_uint(0), C.c_uint(0)
        ffi.check(self.lib.panda_msm_registered_info(self.db.ptr, C.byref(tables), C.byref(bits), None), "info")
        assert tables.value >= 2 and bits.value >= 9, "the call must take the tabled path"
        self.window_bits = bits.value
        self.random = po.gen_scalars(fid, seed + 1, self.n)

    def upload(self, member, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        ffi.check(self.lib.panda_memcpy(C.c_void_p(self.ds.ptr.value + member * self.n * 32), C.c_void_p(rows.ctypes.data), self.n * 32), "memcpy")

    def _cfg(self):
        return ffi.MSMConfiguration(self.gm.mem_pool, self.gm.exec_stream.raw, self.db.ptr, self.ds.ptr, self.dr.ptr, self.k, pgm.JACOBIAN)

    def _results(self):
        raw = self.dr.to_host(np.uint8).reshape(self.members, self.res)
        out = []
        for j in range(self.members):
            w = np.ascontiguousarray(raw[j]).view(np.uint32)
            z = w[2 * w.size // 3:]
            out.append(b"identity" if not z.any() else po.to_affine(self.curve, w).tobytes())
        return out

    def single(self):
        ffi.check(self.lib.panda_memset(self.dr.ptr, 0xA5, self.members * self.res), "memset")
        ffi.check(getattr(self.lib, self.entry)(self._cfg()), "msm")
        return self._results()[0]

    def batch(self):
        ffi.check(self.lib.panda_memset(self.dr.ptr, 0xA5, self.members * self.res), "memset")
        ffi.check(self.lib.panda_msm_execute_batch(self.curve, self._cfg(), self.members), "batch")
        return self._results()

    def expected(self, name, rows):
        if name == "zero":
            return b"identity"
        return po.expected_from_linearity(self.curve, self.seed, rows).tobytes()

    def close(self):
        self.lib.panda_msm_unregister_bases(self.db.ptr)
        for d in (self.db, self.ds, self.dr):
            d.free()


def _check_single_calls(gm, curve, k, seed, sets=SETS):
    p = Problem(gm, curve, k, seed)
    try:
        for name in sets:
            rows = _scalar_set(curve, name, p.random, p.window_bits)
            p.upload(0, rows)
            got = [p.single() for _ in range(3)]  # repeated calls on identical inputs: the same point
            assert got[0] == p.expected(name, rows), (curve, k, name)
            assert got[1] == got[0] and got[2] == got[0], (curve, k, name)
    finally:
        p.close()


@pytest.mark.parametrize("k", [10, 13, 16, 18])
def test_bn254_tabled(gm, k):
    """2^10: a fraction of one tile per window; 2^13: exactly one; 2^16 and 2^18: many, with ragged level-2 tiles and level-3 cells of
    every class (empty, sparse, dense)"""
    _check_single_calls(gm, 0, k, 0x50A0 + k)


def test_bn254_tabled_fused_digits(gm):
    """2^22: the size from which the digits and the level-1 histogram are one kernel"""
    _check_single_calls(gm, 0, 22, 0x50C0, sets=("equal", "uniform"))


def test_14_limb_curve_tabled(gm):
    _check_single_calls(gm, 1, 16, 0x50D0)


def test_batch_group_of_four(gm):
    """one panda_msm_execute_batch call is one sort over the group's scalars: every scalar set next to three others"""
    k = 14
    p = Problem(gm, 0, k, 0x50E0, members=4)
    try:
        gl = C.c_uint(99)
        assert p.lib.panda_msm_batch_plan(0, k, p.window_bits, 4, C.byref(gl), None) == 0 and gl.value == 2
        for names in (SETS[:4], SETS[3:]):
            want = []
            for j, name in enumerate(names):
                rows = _scalar_set(0, name, np.roll(p.random, j, axis=0), p.window_bits)
                p.upload(j, rows)
                want.append(p.expected(name, rows))
            got = [p.batch() for _ in range(3)]
            assert got[0] == want, names
            assert got[1] == got[0] and got[2] == got[0], names
    finally:
        p.close()
