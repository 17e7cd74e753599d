"""k_accumulate's addition on signed limbs (ACC_ITEM_SIGNED_DIFF: xyzz_madd_core_s) and the converting loads of the kernels behind
it (load_xyzz_stored in k_fixup, k_fixup_long, k_sum_lines).  BN254 against the CPU oracle's affine result at sizes where the kernel
can still go wrong: 2^8, 2^10 and 2^12 points over window tables, 2^10 over registered-only bases and through the plain entry point;
each at the library's own chunk size and with chunks of 16 entries forced, so that nearly every bucket of more than a few entries is
cut into pieces and goes through the fix-up's loads of marked, signed accumulators.

Scalar sets: random; all equal (one bucket per window holds everything; over a base set of equal rows every addition in it is P + P,
the doubling path, whose unsigned result goes back into the signed addition); every base twice with s and r - s (P + (-P): identity
accumulators in the middle of a run); all zero; all r - 1; every digit negative (every y is p - y, taken on the packed words).
One base set has identity rows among the points.  One case each goes through panda_msm_execute_batch (two members) and through the
point ranges of panda_msm_execute_from_host (k_fixup<MERGE>, k_fixup_long adding into the total)."""
import ctypes as C

import numpy as np
import pytest

import oracle as po
import pyref
from gpu_util import NULL_STREAM, DeviceBuffer, gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

pytestmark = pytest.mark.gpu

CURVE = pyref.CURVES[0]
SEED = 0x51D
KINDS = ["random", "all_equal", "opposite_pairs", "zero", "r_minus_1", "negative_digits"]


@pytest.fixture(autouse=True)
def _built_in_policies():
    def reset():
        lib = ffi.load()
        lib.panda_msm_set_window_bits(0)
        lib.panda_msm_set_accumulate_variant(0)
        lib.panda_msm_set_chunk_entries(0)

    reset()
    yield
    reset()


def _mont(v):
    return pyref.int_to_limbs(v % CURVE.r * CURVE.Rr % CURVE.r, 8)


def _scalars(kind, n, c):
    rng = np.random.default_rng(0x5167 + n)
    rand = lambda: int.from_bytes(rng.bytes(40), "little") % CURVE.r
    if kind == "random":
        vals = [rand() for _ in range(n)]
    elif kind == "all_equal":
        vals = [rand()] * n
    elif kind == "opposite_pairs":  # rows 2i and 2i + 1 hold the same point (_bases("pairs")): s P + (r - s) P
        vals = []
        for _ in range(n // 2):
            s = rand()
            vals += [s, CURVE.r - s]
    elif kind == "zero":
        vals = [0] * n
    elif kind == "r_minus_1":
        vals = [CURVE.r - 1] * n
    else:  # every full c-bit chunk above 2^(c-1) and not all ones: a negative digit and a carry in every window
        half = 1 << (c - 1)
        vals = [sum(int(rng.integers(half + 2, 2 * half - 2)) << (c * j) for j in range(253 // c)) for _ in range(n)]
    return np.stack([_mont(v) for v in vals])


_BASES, _WANT = {}, {}


def _bases(shape, k):
    """one seeded stream of points m_i * G; shapes edit it.  Built once, never changed."""
    if (shape, k) not in _BASES:
        b = po.gen_bases(0, SEED, 1 << k)
        if shape == "pairs":
            b[1::2] = b[0::2]
        elif shape == "equal_rows":
            b[:] = b[0]
        elif shape == "identity_rows":
            b[::5, :8] = 0
            b[(1 << k) // 2:(1 << k) // 2 + 6, :8] = 0
        _BASES[(shape, k)] = b
    return _BASES[(shape, k)]


def _want(shape, k, kind, c, scalars):
    key = (shape, k, kind, c)
    if key not in _WANT:
        _WANT[key] = po.msm_affine(0, _bases(shape, k), scalars, window_bits=9)
    return _WANT[key]


# (scalar set, base set): what each pair is there for is in the module's docstring
CASES = [("random", "generated"), ("all_equal", "generated"), ("all_equal", "equal_rows"), ("opposite_pairs", "pairs"), ("zero", "generated"),
         ("r_minus_1", "generated"), ("negative_digits", "generated"), ("random", "identity_rows"), ("negative_digits", "identity_rows")]


@pytest.mark.parametrize("chunk", [0, 16], ids=["default_chunks", "chunks_of_16"])
@pytest.mark.parametrize("k,path", [(8, "tables"), (10, "tables"), (12, "tables"), (10, "registered"), (10, "plain")])
def test_signed_accumulate_against_the_oracle(gm, k, path, chunk):
    lib = ffi.load()
    n = 1 << k
    c = 10
    ffi.check(lib.panda_msm_set_chunk_entries(chunk), "cfg")
    for shape in sorted({s for _, s in CASES}):
        bases = _bases(shape, k)
        width = c
        idx = None
        if path != "plain":
            idx = gm.add_cached_bases(bases)
            if path == "tables":
                _, width, _ = gm.precompute_cached_bases(idx, curve=0, window_bits=c)
            else:
                gm.register_cached_bases(idx, curve=0)
        if path != "tables":
            ffi.check(lib.panda_msm_set_window_bits(c), "cfg")
        for kind in [kd for kd, s in CASES if s == shape]:
            scalars = _scalars(kind, n, width)
            if idx is None:
                out = pgm.panda_msm_bn254_gpu(gm, scalars, bases)
            else:
                out = pgm.panda_msm_bn254_gpu_with_cached_bases(gm, scalars, idx)
            got = po.to_affine(0, np.asarray(out).view(np.uint32))
            assert (got == _want(shape, k, kind, width, scalars)).all(), (shape, kind)


class _Device:
    """bases with window tables and `members` scalar vectors in device buffers, for the entry points that take a configuration"""

    def __init__(self, gm, k, shape, members):
        self.lib, self.gm, self.k, self.n, self.members = ffi.load(), gm, k, 1 << k, members
        self.bases = _bases(shape, k)
        self.db, self.ds, self.dr = DeviceBuffer.from_host(self.bases), DeviceBuffer(members * self.n * 32), DeviceBuffer(members * 96)
        ffi.check(self.lib.panda_msm_precompute_bases(0, self.db.ptr, k, 0, gm.exec_stream.raw), "precompute")
        bits = C.c_uint(0)
        ffi.check(self.lib.panda_msm_registered_info(self.db.ptr, None, C.byref(bits), None), "info")
        self.width = bits.value

    def cfg(self):
        return ffi.MSMConfiguration(self.gm.mem_pool, self.gm.exec_stream.raw, self.db.ptr, self.ds.ptr, self.dr.ptr, self.k, pgm.JACOBIAN)

    def results(self):
        raw = self.dr.to_host(np.uint8).reshape(self.members, 96)
        return [po.to_affine(0, np.ascontiguousarray(r).view(np.uint32)) for r in raw]

    def close(self):
        self.lib.panda_msm_unregister_bases(self.db.ptr)
        for d in (self.db, self.ds, self.dr):
            d.free()


@pytest.mark.parametrize("chunk", [0, 16], ids=["default_chunks", "chunks_of_16"])
def test_batch_of_two_members(gm, chunk):
    """panda_msm_execute_batch: one sort and one accumulate launch over both members' lists, then one fix-up and one line sum per member"""
    lib = ffi.load()
    ffi.check(lib.panda_msm_set_chunk_entries(chunk), "cfg")
    d = _Device(gm, 10, "identity_rows", 2)
    try:
        sets = [_scalars("negative_digits", d.n, d.width), _scalars("all_equal", d.n, d.width)]
        both = np.ascontiguousarray(np.concatenate(sets), dtype=np.uint32)
        ffi.check(lib.panda_memcpy(d.ds.ptr, C.c_void_p(both.ctypes.data), both.nbytes), "memcpy")
        ffi.check(lib.panda_memset(d.dr.ptr, 0xA5, 2 * 96), "memset")
        ffi.check(lib.panda_msm_execute_batch(0, d.cfg(), 2), "batch")
        for got, scalars in zip(d.results(), sets):
            assert (got == po.msm_affine(0, d.bases, scalars, window_bits=9)).all()
    finally:
        d.close()


@pytest.mark.parametrize("chunk", [0, 16], ids=["default_chunks", "chunks_of_16"])
@pytest.mark.parametrize("kind,shape", [("random", "identity_rows"), ("all_equal", "equal_rows")])
def test_point_ranges_from_host(gm, kind, shape, chunk):
    """panda_msm_execute_from_host in three ranges: the first range's buckets stay as k_accumulate and k_fixup left them -- marked and
    unmarked side by side -- and the later ranges' fix-ups load them again and add to them"""
    lib = ffi.load()
    ffi.check(lib.panda_msm_set_chunk_entries(chunk), "cfg")
    d = _Device(gm, 10, shape, 1)
    try:
        scalars = np.ascontiguousarray(_scalars(kind, d.n, d.width), dtype=np.uint32)
        ffi.check(lib.panda_memset(d.ds.ptr, 0, d.n * 32), "memset")
        ffi.check(lib.panda_memset(d.dr.ptr, 0xA5, 96), "memset")
        ffi.check(lib.panda_msm_execute_from_host(0, d.cfg(), C.c_void_p(scalars.ctypes.data), 3, gm.h2d_stream.raw), "msm")
        assert (d.results()[0] == po.msm_affine(0, d.bases, scalars, window_bits=9)).all()
    finally:
        d.close()
