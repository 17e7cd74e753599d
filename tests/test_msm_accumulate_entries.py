"""k_accumulate entry by entry: the code around the addition in the hot loop of the MSM -- the negation of y under a negative digit, the
identity test of a row, the walk through the sorted words (quads, 64-byte sectors through LDS), the "accumulator is the identity" flag and
the run-boundary path -- on scalar sets built to steer the loop's branches.  BN254 over precomputed window tables and over
registered-only bases, at 2^8, 2^10 and 2^12 points, each result compared as an affine point with the CPU oracle.  At these sizes the
library's own chunk is 16 entries -- one 64-byte sector, so chunk and quad boundaries occur but a chunk never enters a second sector:
test_chunks_of_several_sectors forces longer chunks (panda_msm_set_chunk_entries) to reach the transfer of the next sector, the
explicit waits in front of a newly entered sector's first read and the second LDS buffer.

What the sets establish: the scalars are built so that digits of the wanted sign, runs of the wanted shape and identity rows at the
wanted places must occur if the library cuts windows as described below; nothing reads back from the device that they did.  The
tables path may settle on a narrower window than asked for, and the scalars are then built for the width it reports.  Whatever
branches are reached, the result is checked against the independent CPU oracle.

Digits: a scalar is cut into windows of c bits and recoded to signed digits; a c-bit chunk (plus the carry of the chunk below) above
2^(c-1) becomes a negative digit and carries one into the next window.  The sets below choose every full chunk of every scalar inside
the open halves (1, 2^(c-1) - 1) or (2^(c-1) + 1, 2^c - 2), so the sign of every digit but the carry at the very top is decided
whatever side the recoding puts the boundary values on."""

import numpy as np
import pytest

import oracle as po
import pyref
from gpu_util import NULL_STREAM, DeviceBuffer, gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

pytestmark = pytest.mark.gpu

CURVE = pyref.CURVES[0]
SEED = 0xACC0


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
    return pyref.int_to_limbs(v * CURVE.Rr % CURVE.r, 8)


def _from_chunks(c, pick):
    """the scalar whose j-th full c-bit chunk is pick(j); it stays below 2^253 < r"""
    v = 0
    for j in range(253 // c):
        v |= pick(j) << (c * j)
    return v


_SCALARS = {}


def _scalars(kind, n, c):
    key = (kind, n, c)
    if key not in _SCALARS:
        _SCALARS[key] = _make_scalars(kind, n, c)
    return _SCALARS[key].copy()


def _make_scalars(kind, n, c):
    rng = np.random.default_rng(0xD161 + n)
    half = 1 << (c - 1)
    pos = lambda: int(rng.integers(2, half - 1))          # chunk (+ carry) stays below 2^(c-1): a positive digit
    neg = lambda: int(rng.integers(half + 2, 2 * half - 2))  # above 2^(c-1) and not all ones: a negative digit, carry 1
    if kind == "negative":
        vals = [_from_chunks(c, lambda j: neg()) for _ in range(n)]
    elif kind == "positive":
        vals = [_from_chunks(c, lambda j: pos()) for _ in range(n)]
    elif kind == "alternating":  # by window and by point: neighbours in a window's list and in a lane's stretch differ in sign
        vals = [_from_chunks(c, lambda j: neg() if (i + j) & 1 else pos()) for i in range(n)]
    elif kind == "all_equal":  # one bucket per window holds every entry: one long run, no boundary inside any chunk but the first
        v = _from_chunks(c, lambda j: neg() if j & 1 else pos())
        vals = [v] * n
    elif kind == "few_buckets":  # three scalars over all points: three buckets per window, runs that span sectors and chunks
        three = [_from_chunks(c, lambda j: neg() if (t + j) & 1 else pos()) for t in range(3)]
        vals = [three[int(t)] for t in rng.integers(0, 3, n)]
    elif kind == "counting":  # 1, 2, 3, ...: in the lowest window every bucket has one entry, every trip is a boundary
        vals = list(range(1, n + 1))
    else:
        raise ValueError(kind)
    return np.stack([_mont(v) for v in vals])


KINDS = ["negative", "positive", "alternating", "all_equal", "counting"]


def _run(gm, make_scalars, bases, tabled, c):
    """BN254 through the cached-bases entry point: window tables of (at most) c-bit windows, or registered-only bases with the window
    width set to c.  make_scalars(width) builds the scalars for the window width the library settled on.  Returns (affine result, scalars)."""
    lib = ffi.load()
    idx = gm.add_cached_bases(bases)
    if tabled:
        _, c, _ = gm.precompute_cached_bases(idx, curve=0, window_bits=c)
    else:
        gm.register_cached_bases(idx, curve=0)
        ffi.check(lib.panda_msm_set_window_bits(c), "cfg")
    scalars = make_scalars(c)
    try:
        out = pgm.panda_msm_bn254_gpu_with_cached_bases(gm, scalars, idx)
    finally:
        lib.panda_msm_set_window_bits(0)
    return po.to_affine(0, np.asarray(out).view(np.uint32)), scalars


@pytest.fixture(scope="module")
def generated_bases():
    """bases m_i * G of one seeded stream, shared by every test that does not edit them (expected values come by linearity)"""
    return {k: po.gen_bases(0, SEED, 1 << k) for k in (8, 10, 12)}


@pytest.mark.parametrize("tabled", [True, False], ids=["tables", "registered"])
@pytest.mark.parametrize("k", [8, 10, 12])
@pytest.mark.parametrize("kind", KINDS)
def test_digit_sign_and_run_shapes(gm, generated_bases, kind, k, tabled):
    n = 1 << k
    c = max(k + 1, 10)  # 2^(c-1) >= n: the counting scalars stay positive digits of distinct buckets
    got, scalars = _run(gm, lambda width: _scalars(kind, n, width), generated_bases[k], tabled, c)
    assert (got == po.expected_from_linearity(0, SEED, scalars)).all()


@pytest.mark.parametrize("tabled", [True, False], ids=["tables", "registered"])
def test_list_lengths_off_the_quad_and_sector_grid(gm, generated_bases, tabled):
    """2^10 - 3 points (the entry points take powers of two: the last three scalars are zero and leave no entry in any list), so the
    lists end inside a quad and inside a sector"""
    n = 1 << 10
    def make(width):
        scalars = _scalars("alternating", n, width)
        scalars[n - 3:] = 0
        return scalars

    got, scalars = _run(gm, make, generated_bases[10], tabled, 11)
    assert (got == po.expected_from_linearity(0, SEED, scalars)).all()


@pytest.mark.parametrize("k", [0, 1, 3])
def test_tiny_lists_off_sixteen_and_sixty_four_bytes(gm, k):
    """1, 2 and 8 points through the plain entry point: the lists of the windows above the first start off a 16-byte (1, 2 points) or a
    64-byte boundary (8), the loop's single-word and 16-byte-load fallbacks"""
    n = 1 << k
    bases = po.gen_bases(0, SEED + 1, n)
    scalars = _scalars("alternating", n, 10)
    out = pgm.panda_msm_bn254_gpu(gm, scalars, bases)
    assert (po.to_affine(0, np.asarray(out).view(np.uint32)) == po.expected_from_linearity(0, SEED + 1, scalars)).all()


@pytest.mark.parametrize("tabled", [True, False], ids=["tables", "registered"])
@pytest.mark.parametrize("kind", ["alternating", "few_buckets"])
@pytest.mark.parametrize("k", [10, 12])
@pytest.mark.parametrize("chunk", [24, 32, 48, 64, 128])
def test_chunks_of_several_sectors(gm, generated_bases, chunk, k, kind, tabled):
    """Forced chunks of 32, 48, 64 and 128 entries (two to eight 64-byte sectors: the sector kernel sends sector s + 1 to LDS when it
    enters sector s, waits for sector s by count and alternates between its two buffers) and of 24 (no multiple of 16: the kernel
    that loads its quads from memory).  The last 37 scalars are zero and leave no entry, so every list ends inside a chunk, a sector
    and a quad: in the wave that holds the list's last chunk some lanes still have a next sector to send when the last lane has none,
    and both of the waits run.  Identity rows and P, -P pairs ride along so that those paths cross sector boundaries too."""
    n = 1 << k
    bases = generated_bases[k].copy()
    bases[7::11, :8] = 0
    pairs = range(5, n // 2, 64)
    for i in pairs:
        bases[i + 1] = _negated(bases[i:i + 1])[0]

    def make(width):
        scalars = _scalars(kind, n, width)
        for i in pairs:
            scalars[i + 1] = scalars[i]
        scalars[n - 37:] = 0
        return scalars

    ffi.check(ffi.load().panda_msm_set_chunk_entries(chunk), "cfg")
    try:
        got, scalars = _run(gm, make, bases, tabled, 10)
    finally:
        ffi.load().panda_msm_set_chunk_entries(0)
    assert (got == po.msm_affine(0, bases, scalars, window_bits=9)).all()


def _negated(points):
    out = points.copy()
    out[:, 8:] = po.f_vec(0, po.OP_SUB, np.zeros_like(points[:, 8:]), points[:, 8:])
    return out


@pytest.mark.parametrize("tabled", [True, False], ids=["tables", "registered"])
@pytest.mark.parametrize("k", [8, 10, 12])
def test_identity_rows_at_every_position(gm, generated_bases, k, tabled):
    """Identity rows (wire x = 0) under digits of both signs.  Where a row falls in the sorted lists is the sort's business, so there
    are many: every fifth base, under random digits in about 25 windows -- each of first-in-a-chunk, last-in-a-chunk (one in sixteen
    entries or more each) and first-in-a-run (most entries, at one entry a bucket) is hit hundreds of times even at 2^8; and a block of
    identity rows that share one scalar with their neighbours, so that an identity row also opens, continues and ends a longer run."""
    n = 1 << k
    c = 10
    bases = generated_bases[k].copy()
    bases[::5, :8] = 0
    lo = n // 2
    bases[lo:lo + 24:3, :8] = 0
    bases[lo + 23, :8] = 0

    def make(width):
        scalars = _scalars("alternating", n, width)
        scalars[lo:lo + 24] = scalars[lo]
        return scalars

    got, scalars = _run(gm, make, bases, tabled, c)
    assert (got == po.msm_affine(0, bases, scalars, window_bits=9)).all()


@pytest.mark.parametrize("tabled", [True, False], ids=["tables", "registered"])
@pytest.mark.parametrize("k", [8, 10, 12])
def test_same_point_and_opposite_point_in_one_bucket(gm, generated_bases, k, tabled):
    """P then P (the doubling branch) and P then -P (the sum is the identity: the accumulator's identity flag is set in the middle of
    a run, and the next row of the run must become the accumulator) under equal scalars, so the pair meets in one bucket of every
    window; triples P, -P, Q and P, -P, -P, P, P go through identity and back."""
    n = 1 << k
    c = 10
    bases = generated_bases[k].copy()
    groups = range(0, n // 2, 16)  # 8 pairs and triples at 2^8, 128 at 2^12
    for i in groups:
        kind = (i // 16) % 4
        if kind == 0:    # P, P
            bases[i + 1] = bases[i]
        elif kind in (1, 2):  # P, -P  and  P, -P, Q
            bases[i + 1] = _negated(bases[i:i + 1])[0]
        else:            # P, -P, -P, P, P
            bases[i + 1] = bases[i + 2] = _negated(bases[i:i + 1])[0]
            bases[i + 3] = bases[i + 4] = bases[i]

    def make(width):
        scalars = _scalars("alternating", n, width)
        for i in groups:
            scalars[i + 1:i + (2, 2, 3, 5)[(i // 16) % 4]] = scalars[i]
        return scalars

    got, scalars = _run(gm, make, bases, tabled, c)
    assert (got == po.msm_affine(0, bases, scalars, window_bits=9)).all()


def _g2_expected(seed_b, scalars):
    return pyref.g2_mul(pyref.limbs_to_int(po.linear_combination(0, seed_b, scalars, 0)), pyref.G2_GEN)


@pytest.mark.parametrize("cid", [1, 3], ids=["bls12_377", "bn254_g2"])
def test_curves_that_keep_the_former_loop(gm, cid):
    """BLS12-377 (14-limb Fq) and BN254 G2 (Fq2) at 2^10 over window tables: their accumulate kernels take none of the slimmed code"""
    lib = ffi.load()
    k = 10
    n = 1 << k
    pt, res = {1: (96, 144), 3: (128, 192)}[cid]
    fn = {1: lib.panda_msm_execute_bls12_377, 3: lib.panda_msm_execute_bn254_g2}[cid]
    db, ds, dr = DeviceBuffer(n * pt), DeviceBuffer(n * 32), DeviceBuffer(res)
    seed_b = SEED + 16 + cid
    try:
        ffi.check(lib.panda_gen_bases(cid, seed_b, 0, n, db.ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_gen_scalars(cid, seed_b + 1, 0, n, ds.ptr, NULL_STREAM), "gen")
        scalars = ds.to_host().reshape(n, 8)
        ffi.check(lib.panda_msm_precompute_bases(cid, db.ptr, k, 0, gm.exec_stream.raw), "precompute")
        cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, db.ptr, ds.ptr, dr.ptr, k, pgm.JACOBIAN)
        ffi.check(lib.panda_memset(dr.ptr, 0, res), "memset")
        ffi.check(fn(cfg), "msm")
        if cid == 3:
            assert pyref.g2_decode_jacobian(dr.to_host().view(np.uint32)) == _g2_expected(seed_b, scalars)
        else:
            assert (po.to_affine(cid, dr.to_host()) == po.expected_from_linearity(cid, seed_b, scalars)).all()
    finally:
        lib.panda_msm_unregister_bases(db.ptr)
        for d in (db, ds, dr):
            d.free()
