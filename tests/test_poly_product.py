"""panda_field_batch_inverse / panda_poly_grand_product / panda_poly_product_plan: the inverse of every element of a vector (zero for
zero) and the exclusive running products Z_0 = 1, Z_i = prod_{j < i} num_j / den_j of `batch` vectors with their totals, on elements
resident on the device -- the permutation argument's grand product and the vector inversions of a PLONK / halo2 prover.

A wire residue is w = x W mod r (W = 2^256), so on the integers of the wire the inverse is W^2 / w and one step of the running product is
Z_(i+1) = Z_i num_i / den_i with Z_0 = W (a missing denominator is the wire's one, W).  Expected values are Python integers (pow(w, -1, r),
running products; moduli from po.field_info) up to a few tiles; above that the CPU oracle's vector products check the complete
characterisations -- out_i in_i = one where in_i != 0 and out_i = 0 where in_i = 0; out_0 = one, out_(i+1) den_i = out_i num_i for
i < n - 1 and totals den_(n-1) = out_(n-1) num_(n-1), which determine the output when no denominator is zero.  Outputs are canonical and
every comparison is byte for byte.  Every boundary size comes from panda_poly_product_plan.  Each device buffer carries a guard run of a
fixed byte pattern behind the data, which no call may touch; inputs must come back unchanged unless they are the output."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import field_ref as fr
import oracle as po
from gpu_util import GUARD, ROOT, GuardedBuffers, assert_exported, free_bytes, gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_poly_product as mpp  # noqa: E402

MAX_ELEMS = 1 << 28
NAMES = ("panda_field_batch_inverse", "panda_poly_grand_product", "panda_poly_product_plan")


def _plan(lib, n, batch):
    ti, tp, chunk, launches = C.c_uint(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
    rc = lib.panda_poly_product_plan(n, batch, C.byref(ti), C.byref(tp), C.byref(chunk), C.byref(launches))
    return rc, ti.value, tp.value, chunk.value, launches.value


@functools.lru_cache(maxsize=None)
def _shape():
    """(tile_inverse, tile_product, carry_chunk) of the library"""
    rc, ti, tp, chunk, _ = _plan(ffi.load(), 1, 1)
    assert rc == 0
    return ti, tp, chunk


def _no_zero(a):
    """no element of the (..., 8) array is zero"""
    return bool(np.any(np.asarray(a).reshape(-1, 8), axis=1).all())


def _zero_rows(a):
    return set(np.flatnonzero(~np.any(np.asarray(a).reshape(-1, 8), axis=1)).tolist())


def _inverse_expected(field, x):
    r = fr.modulus(field)
    w2 = fr.W * fr.W % r
    return fr.words([pow(w, -1, r) * w2 % r if w else 0 for w in fr.ints(x)])


def _product_expected(field, num, den):
    """(Z words (n, 8), total words (8,)) of one vector; den None: the running product of num; a zero denominator: all zero"""
    r = fr.modulus(field)
    nw = fr.ints(num)
    dw = [fr.W % r] * len(nw) if den is None else fr.ints(den)
    if 0 in dw:
        return np.zeros((len(nw), 8), np.uint32), np.zeros(8, np.uint32)
    z, acc = [], fr.W % r
    for a, b in zip(nw, dw):
        z.append(acc)
        acc = acc * a % r * pow(b, -1, r) % r
    return fr.words(z), fr.words([acc])[0]


def _is_inverse(field, x, out):
    fid = po.FR_OF[field]
    zero = ~np.any(x, axis=1)
    want = np.where(zero[:, None], np.uint32(0), fr.wire_one(field, 1)[None, :]).astype(np.uint32)
    return np.array_equal(po.f_vec(fid, po.OP_MUL, out, x), want) and not out[zero].any()


def _is_product(field, num, den, out, total):
    """the complete characterisation for a vector without a zero denominator (den None: the wire's one)"""
    fid = po.FR_OF[field]
    n = len(num)
    one = fr.wire_one(field, 1)
    if den is None:
        den = np.broadcast_to(one, (n, 8))
    if not np.array_equal(out[0], one):
        return False
    step = po.f_vec(fid, po.OP_MUL, out, num)  # out_i num_i
    nxt = np.concatenate([out[1:], total.reshape(1, 8)])  # out_(i+1), and the total behind the last
    return np.array_equal(po.f_vec(fid, po.OP_MUL, nxt, np.ascontiguousarray(den)), step)


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    _, lib = assert_exported(NAMES)
    assert lib.panda_field_batch_inverse.argtypes[3] is C.c_uint64 and lib.panda_poly_grand_product.argtypes[4] is C.c_uint64
    assert lib.panda_poly_product_plan.argtypes[0] is C.c_uint64


def test_bad_arguments_are_refused_before_any_device_call():
    """every shape, pointer and overlap error returns 1 with the host output untouched -- also on a machine with no device"""
    lib = ffi.load()
    mem = np.zeros(3 << 20, np.uint8)  # three disjoint 1 MiB host ranges stand in for the device buffers: nothing may dereference them
    base = mem.ctypes.data
    at = lambda off: C.c_void_p(base + off)
    A, B, O = 0, 1 << 20, 2 << 20
    stream = ffi.PandaStream()
    out = np.full((4, 8), 0x5A5A5A5A, np.uint32)
    outp = C.c_void_p(out.ctypes.data)

    def inv(f=0, i=at(A), o=at(O), n=32):
        return lib.panda_field_batch_inverse(f, i, o, n, stream)

    def gp(f=0, num=at(A), den=at(B), o=at(O), n=16, batch=2, tot=outp):
        return lib.panda_poly_grand_product(f, num, den, o, n, batch, tot, stream)

    assert inv(f=3) == 1 and gp(f=3) == 1
    assert inv(n=0) == 1 and gp(n=0) == 1 and gp(batch=0) == 1
    assert inv(n=MAX_ELEMS + 1) == 1 and gp(n=MAX_ELEMS + 1, batch=1) == 1
    assert gp(n=(MAX_ELEMS >> 1) + 1, batch=2) == 1 and gp(n=1, batch=MAX_ELEMS + 1) == 1
    assert inv(n=1 << 63) == 1 and inv(n=(1 << 64) - 1) == 1 and gp(n=1 << 63, batch=2) == 1 and gp(n=1 << 32, batch=1 << 31) == 1
    assert inv(i=None) == 1 and inv(o=None) == 1
    assert gp(num=None) == 1 and gp(o=None) == 1 and gp(num=None, den=None) == 1
    # 32 elements / 2 vectors of 16 are 1024 bytes: every way two ranges can meet without being equal
    for off in (1023, 32, -32, -1023):
        assert inv(o=at(A + off + 4096), i=at(A + 4096)) == 1
        assert gp(o=at(A + 4096 + off), num=at(A + 4096)) == 1                      # out against num
        assert gp(o=at(B + 4096 + off), den=at(B + 4096)) == 1                      # out against den
        assert gp(num=at(A + 4096), den=at(A + 4096 + off)) == 1                    # num against den
        assert gp(num=at(A + 4096), den=at(A + 4096 + off), o=at(A + 4096)) == 1    # in place on num, den shifted
        assert gp(num=at(A + 4096), den=None, o=at(A + 4096 + off)) == 1            # no denominators: out against num
    assert (out == 0x5A5A5A5A).all(), "a refused call wrote to totals"
    assert lib.panda_poly_product_plan(16, 2, None, None, None, None) == 0
    for n, batch in ((0, 1), (1, 0), (MAX_ELEMS + 1, 1), ((MAX_ELEMS >> 1) + 1, 2), (1, MAX_ELEMS + 1), (1 << 63, 2), ((1 << 64) - 1, 1), (1 << 32, 1 << 31)):
        assert lib.panda_poly_product_plan(n, batch, None, None, None, None) == 1, (n, batch)


def test_product_plan():
    lib = ffi.load()
    for n in (1, 2, 3, 63, 64, 65, 1000, 2047, 2048, 2049, (1 << 16) + 3, (1 << 20) + 2, 1 << 24, (1 << 27) + 1, 1 << 28):
        seen = set()
        for batch in (1, 2, 3, 16, 256, 1 << 20, 1 << 28):
            if n * batch > MAX_ELEMS:
                assert lib.panda_poly_product_plan(n, batch, None, None, None, None) == 1
                continue
            rc, ti, tp, chunk, launches = _plan(lib, n, batch)
            assert rc == 0 and ti >= 1 and tp >= 1 and chunk >= 1 and launches >= 1, (n, batch)
            seen.add((ti, tp, chunk, launches))
            for i in range(4):  # every out pointer may be NULL, singly
                outs = [C.c_uint(0xDEAD) for _ in range(4)]
                args = [C.byref(o) if j != i else None for j, o in enumerate(outs)]
                assert lib.panda_poly_product_plan(n, batch, *args) == 0
                assert [o.value for j, o in enumerate(outs) if j != i] == [v for j, v in enumerate((ti, tp, chunk, launches)) if j != i]
        assert len(seen) == 1, "none of the four depends on the batch"


def _runs(tile):
    """(thread run, wave run) of a kernel with this tile (the model's constants mirror csrc/poly_product.hip)"""
    e = tile // (mpp.WAVE * mpp.WAVES)
    return e, mpp.WAVE * e


def _boundary_sizes(tile):
    e, we = _runs(tile)
    sizes = {1, 2, 3, 63, 64, 65, e - 1, e + 1, we - 1, we + 1, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile - 7}
    return sorted(s for s in sizes if s >= 1)


def _second_level_sizes(tile):
    chunk = _shape()[2]
    return tile * chunk + 1, 2 * tile * chunk + tile + 5


def test_model_agrees_with_the_plain_definitions():
    """tools/model_poly_product.py -- the three launches' index maps over exact integers -- with the library's tiles and carry chunk, at
    every size the device tests use, out of place and in place, with planted zeros; and a scaled-down shape at every n through three
    carry chunks"""
    ti, tp, chunk = _shape()
    for tile in sorted({ti, tp}):
        sh = mpp.Shape.from_plan(tile, chunk)
        assert (sh.tile, sh.chunk) == (tile, chunk)
        for n in _boundary_sizes(tile) + [s for s in _second_level_sizes(tile) if s <= 1 << 23]:
            assert mpp.check(sh, n)
        n = 2 * tile + 1
        e, we = _runs(tile)
        for zeros in ((0,), (n - 1,), tuple(range(3 * e, 4 * e)), tuple(range(we, 2 * we)), tuple(range(tile, 2 * tile)), tuple(range(n))):
            assert mpp.check(sh, n, zeros=zeros)
        for den_zeros in ((0,), (tile + tile // 2,), (n - 1,)):
            assert mpp.check(sh, n, den_zeros=den_zeros)
    small = mpp.Shape(e=3, wave=4, waves=2, ce=2)
    for n in range(1, 2 * small.tile * small.chunk + small.tile + 6):
        assert mpp.check(small, n)
    n = 2 * small.tile * small.chunk + 7
    assert mpp.check(small, n, zeros=(5,), den_zeros=(n - 1,)) and mpp.check(small, n, zeros=tuple(range(n)))


# ------------------------------------------------------------------------------------------------- on the device
@functools.lru_cache(maxsize=None)
def _vectors(field, n, batch, seed):
    """(batch, n, 8) random scalars without a zero among them"""
    x = po.gen_scalars(po.FR_OF[field], seed, batch * n).reshape(batch, n, 8)
    assert _no_zero(x), "the random data holds a zero"
    x.setflags(write=False)
    return x


class Harness(GuardedBuffers):
    """three guarded device buffers of batch x n elements (a, b, o)"""

    def __init__(self, gm, field, n, batch=1):
        super().__init__()
        self.lib, self.field, self.n, self.batch = ffi.load(), field, n, batch
        self.bytes = batch * n * 32
        self.a, self.b, self.o = (self.buffer(nbytes=self.bytes) for _ in range(3))
        self.stream = gm.exec_stream.raw

    def load(self, a, b=None):
        """the three buffers afresh, with batch x n elements in a and, if given, in b"""
        assert all(x is None or np.asarray(x).nbytes == self.bytes for x in (a, b))
        self.fill(self.a, a)
        self.fill(self.b, b)
        self.fill(self.o)

    def rows(self, d):
        return self.get(d).reshape(self.batch, self.n, 8)

    def inverse(self, x, in_place=False):
        """one panda_field_batch_inverse over the batch x n elements end to end -> (batch, n, 8); checks guards and the input"""
        self.load(x)
        dst = self.a if in_place else self.o
        ffi.check(self.lib.panda_field_batch_inverse(self.field, self.a.ptr, dst.ptr, self.batch * self.n, self.stream), "inverse")
        assert self.guard_intact(self.a) and self.guard_intact(self.o) and self.untouched(self.b), "bytes outside the output were written"
        if in_place:
            assert self.untouched(self.o)
        else:
            assert self.intact(self.a), "d_in was written"
        return self.rows(dst)

    def product(self, num, den, where="o", totals=True, den_is_num=False):
        """one panda_poly_grand_product -> (out (batch, n, 8), totals (batch, 8) or None); where: the buffer d_out is ("o", "a" = d_num,
        "b" = d_den); den None: d_den == NULL; den_is_num: d_den is d_num's pointer"""
        if den_is_num:
            den = None
        self.load(num, den)
        dst = {"o": self.o, "a": self.a, "b": self.b}[where]
        d_den = self.a.ptr if den_is_num else (self.b.ptr if den is not None else None)
        tot = np.full((self.batch, 8), 0x77777777, np.uint32) if totals else None
        ffi.check(self.lib.panda_poly_grand_product(self.field, self.a.ptr, d_den, dst.ptr, self.n, self.batch, C.c_void_p(tot.ctypes.data) if totals else None,
                                                    self.stream), "grand_product")
        assert all(self.guard_intact(d) for d in (self.a, self.b, self.o)), "bytes behind the batch were written"
        if where != "a":
            assert self.intact(self.a), "d_num was written"
        if where != "b":
            assert self.untouched(self.b) if den is None else self.intact(self.b), "d_den was written"
        if where != "o":
            assert self.untouched(self.o), "the third buffer was written by a call in place"
        return self.rows(dst), tot


def _check_product(h, num, den, out, tot, by_identity=False):
    for p in range(h.batch):
        dp = None if den is None else den[p]
        if by_identity:
            assert _is_product(h.field, num[p], dp, out[p], tot[p]), (h.field, h.n, p)
        else:
            want, want_t = _product_expected(h.field, num[p], dp)
            assert np.array_equal(out[p], want), (h.field, h.n, p)
            assert tot is None or np.array_equal(tot[p], want_t), (h.field, h.n, p)


@pytest.mark.gpu
def test_inverse_bn254_at_the_boundary_sizes(gm):
    """n around the thread run, the wave's run, the tile, several tiles with a ragged tail (from the plan, so walked inside one test)"""
    for n in _boundary_sizes(_shape()[0]):
        x = _vectors(0, n, 1, 0x1A000 + n)
        h = Harness(gm, 0, n)
        try:
            assert np.array_equal(h.inverse(x)[0], _inverse_expected(0, x[0])), n
        finally:
            h.close()


@pytest.mark.gpu
def test_product_bn254_at_the_boundary_sizes(gm):
    for n in _boundary_sizes(_shape()[1]):
        num, den = _vectors(0, n, 3, 0x1B000 + n), _vectors(0, n, 3, 0x1C000 + n)
        h = Harness(gm, 0, n, 3)
        try:
            out, tot = h.product(num, den)
            _check_product(h, num, den, out, tot)
        finally:
            h.close()


def _second_level_n(tile, which):
    n = _second_level_sizes(tile)[which]
    if n > 1 << 23:
        pytest.skip("tile x carry_chunk exceeds 2^23 elements for this plan")
    return n


def _second_level_inverse(gm, field, which, in_place=False):
    n = _second_level_n(_shape()[0], which)
    x = _vectors(field, n, 1, 0x2A000 + which)
    h = Harness(gm, field, n)
    try:
        out = h.inverse(x, in_place=in_place)
        assert _is_inverse(field, x[0], out[0])
        return out
    finally:
        h.close()


def _second_level_product(gm, field, which, batch, where="o"):
    n = _second_level_n(_shape()[1], which)
    num, den = _vectors(field, n, batch, 0x2B000 + which), _vectors(field, n, batch, 0x2C000 + which)
    h = Harness(gm, field, n, batch)
    try:
        out, tot = h.product(num, den, where=where)
        _check_product(h, num, den, out, tot, by_identity=True)
        return out, tot
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_inverse_second_level(gm, which):
    """more tile totals than one step of the seed kernel takes: one chunk and one total, and two chunks and a ragged third"""
    _second_level_inverse(gm, 0, which)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("which", [0, 1])
def test_product_second_level(gm, which, batch):
    _second_level_product(gm, 0, which, batch)


@pytest.mark.gpu
@pytest.mark.gpu_soak
def test_2_24(gm):
    n = 1 << 24
    x, den = _vectors(0, n, 1, 0x2D024), _vectors(0, n, 1, 0x2E024)
    h = Harness(gm, 0, n)
    try:
        assert _is_inverse(0, x[0], h.inverse(x)[0])
        out, tot = h.product(x, den)
        _check_product(h, x, den, out, tot, by_identity=True)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["first", "last", "thread_run", "wave", "tile", "all"])
def test_inverse_with_planted_zeros(gm, case):
    tile = _shape()[0]
    e, we = _runs(tile)
    n = 2 * tile + 1
    where = {"first": [0], "last": [n - 1], "thread_run": range(3 * e, 4 * e), "wave": range(we, 2 * we), "tile": range(tile, 2 * tile), "all": range(n)}[case]
    x = np.array(_vectors(0, n, 1, 0x3A000))
    x[0, list(where)] = 0
    assert _zero_rows(x) == set(where)
    h = Harness(gm, 0, n)
    try:
        out = h.inverse(x)[0]
        assert _zero_rows(out) == set(where), "zeros go to zeros and nothing else does"
        assert np.array_equal(out, _inverse_expected(0, x[0]))
    finally:
        h.close()


@pytest.mark.gpu
def test_product_with_planted_zeros(gm):
    """batch 3, the zero in vector 1 only: a zero numerator is ordinary arithmetic, a zero denominator zeroes the vector and its total;
    vectors 0 and 2 are byte-identical to a run without the zero"""
    tile = _shape()[1]
    n, batch, at = 2 * tile + 1, 3, tile + tile // 2
    num, den = _vectors(0, n, batch, 0x3B000), _vectors(0, n, batch, 0x3C000)
    h = Harness(gm, 0, n, batch)
    try:
        clean, clean_t = h.product(num, den)
        _check_product(h, num, den, clean, clean_t)
        num0 = np.array(num)
        num0[1, at] = 0
        assert _zero_rows(num0) == {n + at} and _no_zero(den)
        out, tot = h.product(num0, den)
        assert np.array_equal(out[1, :at + 1], clean[1, :at + 1]) and not out[1, at + 1:].any() and not tot[1].any()
        assert _no_zero(out[1, :at + 1])
        assert np.array_equal(out[[0, 2]], clean[[0, 2]]) and np.array_equal(tot[[0, 2]], clean_t[[0, 2]])
        for pos in (0, at, n - 1):
            den0 = np.array(den)
            den0[1, pos] = 0
            assert _zero_rows(den0) == {n + pos} and _no_zero(num)
            out, tot = h.product(num, den0)
            assert not out[1].any() and not tot[1].any(), "a zero denominator zeroes the whole vector, element 0 included, and its total"
            assert np.array_equal(out[[0, 2]], clean[[0, 2]]) and np.array_equal(tot[[0, 2]], clean_t[[0, 2]])
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ones", "minus_ones", "num_is_den_one_pointer", "num_is_den_two_buffers"])
def test_edge_values(gm, case):
    tile = max(_shape()[:2])
    n, batch, r = tile + 2, 2, fr.modulus(0)
    one, m1 = fr.wire_one(0, 1), fr.wire_one(0, r - 1)
    h = Harness(gm, 0, n, batch)
    try:
        if case in ("ones", "minus_ones"):
            v = np.broadcast_to(one if case == "ones" else m1, (batch, n, 8))
            inv = h.inverse(v)
            assert np.array_equal(inv, v), "one and -1 are their own inverses"
            out, tot = h.product(v, None)  # the running product: 1, v, v^2, ...
            want = np.where((np.arange(n) % 2 == 1)[None, :, None] & (case == "minus_ones"), m1, one)
            assert np.array_equal(out, np.broadcast_to(want, (batch, n, 8)))
            assert np.array_equal(tot, np.broadcast_to(m1 if (case == "minus_ones" and n % 2) else one, (batch, 8)))
            out, tot = h.product(v, v)
            assert np.array_equal(out, np.broadcast_to(one, (batch, n, 8))) and np.array_equal(tot, np.broadcast_to(one, (batch, 8)))
            _check_product(h, v, None, *h.product(v, None))
        else:
            x = _vectors(0, n, batch, 0x4A000)
            out, tot = h.product(x, x, den_is_num=True) if case == "num_is_den_one_pointer" else h.product(x, x)
            assert np.array_equal(out, np.broadcast_to(one, (batch, n, 8))) and np.array_equal(tot, np.broadcast_to(one, (batch, 8)))
    finally:
        h.close()


@pytest.mark.gpu
def test_the_permutation_argument(gm):
    """den random, num the same multiset under a fixed permutation: Z closes, totals == one"""
    tile = _shape()[1]
    n, batch = 3 * tile + 5, 2
    den = _vectors(0, n, batch, 0x5A000)
    perm = np.random.default_rng(5).permutation(n)
    num = np.ascontiguousarray(den[:, perm])
    h = Harness(gm, 0, n, batch)
    try:
        out, tot = h.product(num, den)
        assert np.array_equal(tot, np.broadcast_to(fr.wire_one(0, 1), (batch, 8)))
        _check_product(h, num, den, out, tot)
    finally:
        h.close()


@pytest.mark.gpu
def test_running_product_without_denominators(gm):
    tile = _shape()[1]
    for n in (1, tile - 1, 2 * tile + 1):
        num = _vectors(0, n, 2, 0x5B000 + n)
        h = Harness(gm, 0, n, 2)
        try:
            out, tot = h.product(num, None)
            _check_product(h, num, None, out, tot)
            out2, tot2 = h.product(num, None, where="a")
            assert np.array_equal(out, out2) and np.array_equal(tot, tot2)
        finally:
            h.close()


@pytest.mark.gpu
def test_the_two_calls_agree(gm):
    """grand_product(num, den) is the running product of num_i * batch_inverse(den)_i"""
    tile = max(_shape()[:2])
    n, batch = 2 * tile + 3, 2
    num, den = _vectors(0, n, batch, 0x5C000), _vectors(0, n, batch, 0x5D000)
    h = Harness(gm, 0, n, batch)
    try:
        out, tot = h.product(num, den)
        inv = h.inverse(den)
        ratio = po.f_vec(po.FR_OF[0], po.OP_MUL, num.reshape(-1, 8), inv.reshape(-1, 8)).reshape(batch, n, 8)
        out2, tot2 = h.product(ratio, None)
        assert np.array_equal(out, out2) and np.array_equal(tot, tot2)
    finally:
        h.close()


@pytest.mark.gpu
def test_in_place_equals_out_of_place(gm):
    tile = max(_shape()[:2])
    n, batch = 2 * tile + 1, 3
    num, den = _vectors(0, n, batch, 0x6A000), _vectors(0, n, batch, 0x6B000)
    h = Harness(gm, 0, n, batch)
    try:
        inv = h.inverse(num)
        assert np.array_equal(inv.reshape(-1, 8), _inverse_expected(0, num.reshape(-1, 8)))
        assert np.array_equal(h.inverse(num, in_place=True), inv)
        out, tot = h.product(num, den)
        _check_product(h, num, den, out, tot)
        for where in ("a", "b"):
            out2, tot2 = h.product(num, den, where=where)
            assert np.array_equal(out, out2) and np.array_equal(tot, tot2), where
    finally:
        h.close()


@pytest.mark.gpu
def test_in_place_at_the_second_level(gm):
    assert np.array_equal(_second_level_inverse(gm, 0, 0), _second_level_inverse(gm, 0, 0, in_place=True))
    out, tot = _second_level_product(gm, 0, 0, 1)
    for where in ("a", "b"):
        out2, tot2 = _second_level_product(gm, 0, 0, 1, where=where)
        assert np.array_equal(out, out2) and np.array_equal(tot, tot2), where


@pytest.mark.gpu
def test_partial_overlaps_and_short_buffers_are_refused(gm):
    from gpu_util import DeviceBuffer
    tile = max(_shape()[:2])
    n, batch = tile + 1, 2
    num, den = _vectors(0, n, batch, 0x7A000), _vectors(0, n, batch, 0x7B000)
    h = Harness(gm, 0, n, batch)
    short = DeviceBuffer(h.bytes - 32)  # one element short
    try:
        h.load(num, den)
        ffi.check(h.lib.panda_memset(short.ptr, GUARD, h.bytes - 32), "memset")
        tot = np.full((batch, 8), 0x77777777, np.uint32)
        tp = C.c_void_p(tot.ctypes.data)
        off = lambda d, k: C.c_void_p(d.ptr.value + k)
        gp = lambda a, b, o: h.lib.panda_poly_grand_product(0, a, b, o, n, batch, tp, h.stream)
        iv = lambda a, o: h.lib.panda_field_batch_inverse(0, a, o, batch * n, h.stream)
        for k in (32, h.bytes - 32):
            assert iv(h.a.ptr, off(h.a, k)) == 1 and iv(off(h.a, k), h.a.ptr) == 1
            assert gp(h.a.ptr, h.b.ptr, off(h.a, k)) == 1 and gp(off(h.a, k), h.b.ptr, h.a.ptr) == 1
            assert gp(h.a.ptr, h.b.ptr, off(h.b, k)) == 1 and gp(h.a.ptr, off(h.b, k), h.b.ptr) == 1
            assert gp(h.a.ptr, off(h.a, k), h.o.ptr) == 1 and gp(h.a.ptr, None, off(h.a, k)) == 1
        assert iv(short.ptr, h.o.ptr) == 1 and iv(h.a.ptr, short.ptr) == 1 and iv(short.ptr, short.ptr) == 1
        assert gp(short.ptr, h.b.ptr, h.o.ptr) == 1 and gp(h.a.ptr, short.ptr, h.o.ptr) == 1 and gp(h.a.ptr, h.b.ptr, short.ptr) == 1
        assert gp(short.ptr, None, short.ptr) == 1
        assert (tot == 0x77777777).all()
        assert (short.to_host(np.uint8) == GUARD).all() and h.untouched(h.o) and h.intact(h.a) and h.intact(h.b), "a refused call wrote to a buffer"
        _check_product(h, num, den, *h.product(num, den))
    finally:
        short.free()
        h.close()


@pytest.mark.gpu
def test_without_totals(gm):
    tile = _shape()[1]
    n, batch = 2 * tile + 1, 3
    num, den = _vectors(0, n, batch, 0x8A000), _vectors(0, n, batch, 0x8B000)
    h = Harness(gm, 0, n, batch)
    try:
        out, tot = h.product(num, den, totals=False)
        assert tot is None
        _check_product(h, num, den, out, None)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_other_fields_at_one_tile_and_one(gm, field):
    ti, tp, _ = _shape()
    x = _vectors(field, ti + 1, 1, 0x9A000 + field)
    h = Harness(gm, field, ti + 1)
    try:
        assert np.array_equal(h.inverse(x)[0], _inverse_expected(field, x[0]))
    finally:
        h.close()
    n, batch = tp + 1, 2
    num, den = _vectors(field, n, batch, 0x9B000 + field), _vectors(field, n, batch, 0x9C000 + field)
    h = Harness(gm, field, n, batch)
    try:
        _check_product(h, num, den, *h.product(num, den))
        _check_product(h, num, None, *h.product(num, None))
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_other_fields_at_the_second_level(gm, field):
    _second_level_inverse(gm, field, 0)
    _second_level_product(gm, field, 0, 2)


@pytest.mark.gpu
def test_scratch_is_reused_and_released(gm):
    tile = _shape()[1]
    n, batch = 5 * tile - 7, 4
    num, den = _vectors(0, n, batch, 0xAA000), _vectors(0, n, batch, 0xAB000)
    h = Harness(gm, 0, n, batch)
    try:
        h.product(num, den)  # whatever the runtime keeps from a kernel's first launch is there before the baseline is read
        h.inverse(num)
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        before = free_bytes(h.lib)
        o1, t1 = h.product(num, den)
        first = free_bytes(h.lib)
        o2, t2 = h.product(num, den)
        assert free_bytes(h.lib) == first, "a repeated identical call allocated"
        h.inverse(num)  # batch x n elements: needs no more scratch than the product
        assert free_bytes(h.lib) == first
        assert np.array_equal(o1, o2) and np.array_equal(t1, t2)
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        assert free_bytes(h.lib) == before, "panda_ntt_tear_down releases the scratch"
    finally:
        h.close()


@pytest.mark.gpu
def test_gpu_manager_helpers(gm):
    tile = max(_shape()[:2])
    n, batch = tile + 3, 3
    num, den = _vectors(0, n, batch, 0xBA000), _vectors(0, n, batch, 0xBB000)
    nums, dens = [np.array(v) for v in num], [np.array(v) for v in den]
    inv = pgm.panda_field_gpu_batch_inverse(gm, nums)
    prods, totals = pgm.panda_poly_gpu_grand_product(gm, nums, dens)
    runs, run_totals = pgm.panda_poly_gpu_grand_product(gm, nums, None)
    assert len(inv) == len(prods) == len(runs) == batch and totals.shape == run_totals.shape == (batch, 8) and totals.dtype == np.uint32
    for p in range(batch):
        assert inv[p].shape == (n, 8) and np.array_equal(inv[p], _inverse_expected(0, num[p]))
        want, want_t = _product_expected(0, num[p], den[p])
        assert prods[p].shape == (n, 8) and np.array_equal(prods[p], want) and np.array_equal(totals[p], want_t)
        want, want_t = _product_expected(0, num[p], None)
        assert np.array_equal(runs[p], want) and np.array_equal(run_totals[p], want_t)
        assert np.array_equal(nums[p], num[p]) and np.array_equal(dens[p], den[p]), "a helper changed its input"
    assert pgm.panda_field_gpu_batch_inverse(gm, []) == []
    p0, t0 = pgm.panda_poly_gpu_grand_product(gm, [], [])
    assert p0 == [] and t0.shape == (0, 8)
    p0, t0 = pgm.panda_poly_gpu_grand_product(gm, [], None)
    assert p0 == [] and t0.shape == (0, 8)
