"""panda_poly_sum_of_products / panda_poly_sum_of_products_plan: for vector p < batch and index i < n

    out[p][i] = s(p, i) * sum_t coeff_t * prod_{f < degree_t} column[c_tf][p][(i + r_tf) mod n]

over columns resident on the device -- the gate, the permutation check and the quotient of a PLONK / halo2 / Groth16 prover's round.

Expected values are Python integers with the moduli of tests/pyref.py: a wire residue is w = x W mod r (W = 2^256), the definition is
evaluated on the x and put back on the wire.  Outputs are canonical, so every comparison is byte for byte; there is no tolerance
anywhere.  T, the elements one workgroup covers, comes from the plan call.  Every device buffer carries a guard run of a fixed byte
pattern behind the data, which no call may touch; inputs must come back unchanged unless they are the output."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import field_ref as fr
import oracle as po
from gpu_util import GUARD, GuardedBuffers, assert_exported, free_bytes, gm, run_host_check  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

MAX_ELEMS = 1 << 28
NAMES = ("panda_poly_sum_of_products", "panda_poly_sum_of_products_plan")


def _plan(lib, n, batch):
    tile, launches = C.c_uint(0), C.c_uint(0)
    rc = lib.panda_poly_sum_of_products_plan(n, batch, C.byref(tile), C.byref(launches))
    return rc, tile.value, launches.value


@functools.lru_cache(maxsize=None)
def _tile():
    rc, tile, _ = _plan(ffi.load(), 1, 1)
    assert rc == 0 and tile >= 1
    return tile


def _col_words(field, col):
    """(batch, n) plain residues -> (batch, n, 8) wire words"""
    return fr.wire(field, [v for row in col for v in row]).reshape(len(col), len(col[0]), 8)


def _expected(field, cols, terms, scales=None, mode=0):
    """the definition over plain residues; cols[c][p][i], terms = [(coeff, [(column, rotation), ...]), ...] -> (batch, n, 8) wire words"""
    r = fr.modulus(field)
    batch, n = len(cols[0]), len(cols[0][0])
    out = []
    for p in range(batch):
        for i in range(n):
            acc = 0
            for k, fs in terms:
                t = k
                for c, rot in fs:
                    t = t * cols[c][p][(i + rot) % n] % r
                acc += t
            s = 1 if mode == 0 else scales[(p if mode == 1 else i) % len(scales)]
            out.append(acc * s % r)
    return fr.wire(field, out).reshape(batch, n, 8)


GATE = [(1, [(0, 0), (5, 0)]), (1, [(1, 0), (6, 0)]), (1, [(2, 0), (5, 0), (6, 0)]), (1, [(3, 0), (7, 0)]), (1, [(4, 0)])]  # q_L q_R q_M q_O q_C a b c


class Expression:
    """the ctypes arrays of one panda_sop_expression; they stay alive with the object"""

    def __init__(self, field, ptrs, terms, scales=None, mode=0, n_scales=None, wire_coeffs=None):
        self.ptrs = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        self.coeffs = np.ascontiguousarray(wire_coeffs if wire_coeffs is not None else fr.wire(field, [k for k, _ in terms]))
        self.degrees = (C.c_uint * max(len(terms), 1))(*[len(fs) for _, fs in terms])
        flat = [f for _, fs in terms for f in fs]
        self.factors = (ffi.SopFactor * max(len(flat), 1))(*[ffi.SopFactor(c, rot) for c, rot in flat])
        self.scales = None if scales is None else np.ascontiguousarray(fr.wire(field, scales))
        self.expr = ffi.SopExpression(self.ptrs, C.c_void_p(self.coeffs.ctypes.data), self.degrees, self.factors,
                                      None if self.scales is None else C.c_void_p(self.scales.ctypes.data), len(ptrs), len(terms),
                                      (0 if scales is None else len(scales)) if n_scales is None else n_scales, mode)

    def snapshot(self):
        return (bytes(self.ptrs), self.coeffs.tobytes(), bytes(self.degrees), bytes(self.factors), None if self.scales is None else self.scales.tobytes(),
                bytes(self.expr))


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, lib = assert_exported(NAMES)
    assert lib.panda_poly_sum_of_products.argtypes[3] is C.c_uint64 and lib.panda_poly_sum_of_products_plan.argtypes[0] is C.c_uint64
    for macro, value in (("MAX_COLUMNS", ffi.SOP_MAX_COLUMNS), ("MAX_TERMS", ffi.SOP_MAX_TERMS), ("MAX_FACTORS", ffi.SOP_MAX_FACTORS),
                         ("MAX_SCALES", ffi.SOP_MAX_SCALES), ("SCALE_NONE", ffi.SOP_SCALE_NONE), ("SCALE_PER_VECTOR", ffi.SOP_SCALE_PER_VECTOR),
                         ("SCALE_CYCLIC", ffi.SOP_SCALE_CYCLIC)):
        assert int(re.search(r"#define\s+PANDA_SOP_%s\s+(\d+)" % macro, header).group(1)) == value
    assert C.sizeof(ffi.SopFactor) == 8 and C.sizeof(ffi.SopExpression) == 5 * C.sizeof(C.c_void_p) + 16
    assert ffi.SopExpression.n_columns.offset == 5 * C.sizeof(C.c_void_p) and ffi.SopFactor.rotation.offset == 4


def test_plan():
    lib = ffi.load()
    for n in (1, 2, 3, 255, 256, 257, 1000, (1 << 16) + 3, 1 << 24, (1 << 27) + 1, 1 << 28):
        seen = set()
        for batch in (1, 2, 3, 16, 1 << 20, 1 << 28):
            if n * batch > MAX_ELEMS:
                assert lib.panda_poly_sum_of_products_plan(n, batch, None, None) == 1
                continue
            rc, tile, launches = _plan(lib, n, batch)
            assert rc == 0 and tile >= 1 and launches == 1, (n, batch)
            seen.add((tile, launches))
            t, l = C.c_uint(0xDEAD), C.c_uint(0xDEAD)
            assert lib.panda_poly_sum_of_products_plan(n, batch, C.byref(t), None) == 0 and t.value == tile
            assert lib.panda_poly_sum_of_products_plan(n, batch, None, C.byref(l)) == 0 and l.value == launches
        assert len(seen) == 1, "neither value depends on the batch"
    assert lib.panda_poly_sum_of_products_plan(MAX_ELEMS, 1, None, None) == 0 and lib.panda_poly_sum_of_products_plan(1, MAX_ELEMS, None, None) == 0
    for n, batch in ((0, 1), (1, 0), (MAX_ELEMS + 1, 1), ((MAX_ELEMS >> 1) + 1, 2), (1, MAX_ELEMS + 1), (1 << 63, 2), ((1 << 64) - 1, 1), (1 << 32, 1 << 31)):
        tile = C.c_uint(0xDEAD)
        assert lib.panda_poly_sum_of_products_plan(n, batch, C.byref(tile), None) == 1 and tile.value == 0xDEAD, (n, batch)


def test_bad_arguments_are_refused_before_any_device_call():
    """every refusal of the contract returns 1 with the output stand-in and the program arrays untouched -- also on a machine with no
    device.  Host memory stands in for the device buffers: nothing may dereference it."""
    lib = ffi.load()
    n, batch = 16, 2
    nbytes = batch * n * 32  # 1024
    mem = np.full(4 << 20, 0x5A, np.uint8)  # four disjoint 1 MiB ranges
    base = mem.ctypes.data
    A, B, D, O = (base + (k << 20) + 4096 for k in range(4))
    stream = ffi.PandaStream()
    one_term = [(1, [(0, 0), (1, 0)])]
    made = []

    def call(field=0, ptrs=(A, B, D), terms=one_term, out=O, n=n, batch=batch, scales=None, mode=0, n_scales=None, wire_coeffs=None, patch=None, expr_null=False):
        x = Expression(min(field, 2), list(ptrs), terms, scales, mode, n_scales, wire_coeffs)
        if patch:
            patch(x.expr)
        before = x.snapshot()
        made.append((x, before))
        rc = lib.panda_poly_sum_of_products(field, None if expr_null else C.byref(x.expr), None if out is None else C.c_void_p(out), n, batch, stream)
        assert x.snapshot() == before, "a refused call changed the program arrays"
        return rc

    def null(member):
        def patch(e):
            setattr(e, member, None)
        return patch

    # shapes
    assert call(field=3) == 1 and call(n=0) == 1 and call(batch=0) == 1
    assert call(n=MAX_ELEMS + 1, batch=1) == 1 and call(n=(MAX_ELEMS >> 1) + 1, batch=2) == 1 and call(n=1, batch=MAX_ELEMS + 1) == 1
    assert call(n=1 << 63, batch=2) == 1 and call(n=(1 << 64) - 1, batch=1) == 1 and call(n=1 << 32, batch=1 << 31) == 1
    # pointers
    assert call(expr_null=True) == 1 and call(out=None) == 1
    assert call(patch=null("columns")) == 1 and call(patch=null("coeffs")) == 1 and call(patch=null("degrees")) == 1 and call(patch=null("factors")) == 1
    for k in range(3):
        assert call(ptrs=[None if j == k else q for j, q in enumerate((A, B, D))]) == 1, "a NULL column pointer"
    # counts: each cap at exactly the cap + 1
    def count(member, value):
        def patch(e):
            setattr(e, member, value)
        return patch
    many = [(1, [(0, 0)])] * (ffi.SOP_MAX_TERMS + 1)
    assert call(patch=count("n_columns", 0)) == 1 and call(ptrs=[A] * (ffi.SOP_MAX_COLUMNS + 1), terms=[(1, [(0, 0)])]) == 1
    assert call(terms=many, patch=count("n_terms", 0)) == 1 and call(terms=many) == 1
    assert call(terms=[(1, [(0, 0)] * (ffi.SOP_MAX_FACTORS + 1))]) == 1
    assert call(terms=[(1, [(0, 0)] * 4)] * (ffi.SOP_MAX_TERMS - 1) + [(1, [(0, 0)] * 5)]) == 1, "63 x 4 + 5 = 257 factors"

    def degrees(*values):
        def patch(e):
            for t, v in enumerate(values):
                e.degrees[t] = v
        return patch
    assert call(terms=[(1, [(0, 0)]), (1, [(1, 0)])], patch=degrees(0x80000000, 0x80000000)) == 1, "degrees whose sum wraps"
    assert call(terms=[(1, [(0, 0)])], patch=degrees(0xFFFFFFFF)) == 1
    # factors
    assert call(terms=[(1, [(0, 0), (3, 0)])]) == 1, "column index == n_columns"
    assert call(ptrs=(A,), terms=[(1, [(1, 0)])]) == 1 and call(terms=[(1, [(0xFFFFFFFF, 0)])]) == 1
    # scales
    assert call(mode=3) == 1 and call(mode=3, scales=[1, 2]) == 1 and call(mode=0xFFFFFFFF) == 1
    for mode in (1, 2):
        assert call(mode=mode) == 1, "scales NULL"
        assert call(mode=mode, scales=[1, 2], n_scales=0) == 1
        assert call(mode=mode, scales=[1] * (ffi.SOP_MAX_SCALES + 1)) == 1
    # constants at and above the modulus, per field
    for field in (0, 1, 2):
        r = fr.modulus(field)
        for bad in (r, r + 1, fr.W - 1):
            assert call(field=field, wire_coeffs=fr.words([bad])) == 1
            assert call(field=field, terms=[(1, [(0, 0)]), (1, [(1, 0)])], wire_coeffs=fr.words([1, bad])) == 1

            def bad_scale(e, bad=bad):
                C.memmove(e.scales + 32, int(bad).to_bytes(32, "little"), 32)
            assert call(field=field, mode=1, scales=[1, 2, 3], patch=bad_scale) == 1
    # overlaps of d_out with a column
    for off in (32, -32, nbytes - 1, -(nbytes - 1)):
        for k in range(3):
            assert call(ptrs=[O + off if j == k else q for j, q in enumerate((A, B, D))]) == 1, ("partial overlap", off, k)
        assert call(ptrs=(A, B, D, O + off), terms=one_term) == 1, "a column no factor names still may not overlap d_out partly"
    for rot in (1, -1, n + 1, n - 1, -(1 << 31) + 1):
        assert call(ptrs=(O, B, D), terms=[(1, [(0, rot)])]) == 1, ("in place with a rotated factor", rot)
        assert call(ptrs=(A, O, D), terms=[(1, [(0, 0), (1, 0)]), (1, [(1, rot)])]) == 1
        assert call(ptrs=(O, O, D), terms=[(1, [(0, 0)]), (1, [(1, rot)])]) == 1, "the same buffer under a second column index"
    assert (mem == 0x5A).all(), "a refused call wrote to a buffer"
    assert len(made) > 90


def test_host_program_checks_the_bounds(tmp_path):
    """tests/host_check/poly_terms_host.cpp: the program builder and the per-element routine the kernel runs, on the host under FE29_CHECK,
    against 256-bit arithmetic of its own -- every operand p - 1, 64 terms of degree 4, one term of degree 256, coefficients 0 and p - 1,
    the three fields"""
    assert run_host_check(tmp_path, "poly_terms_host.cpp") >= 1000


# ------------------------------------------------------------------------------------------------- on the device
class Harness(GuardedBuffers):
    """one guarded device buffer per column and one for the output, of batch x n elements"""

    def __init__(self, gm, field, n, batch=1):
        super().__init__()
        self.lib, self.field, self.n, self.batch = ffi.load(), field, n, batch
        self.bytes = batch * n * 32
        self.stream = gm.exec_stream.raw

    def call(self, ptrs, terms, out_ptr, scales=None, mode=0):
        x = Expression(self.field, ptrs, terms, scales, mode)
        return self.lib.panda_poly_sum_of_products(self.field, C.byref(x.expr), C.c_void_p(out_ptr), self.n, self.batch, self.stream)

    def run(self, cols, terms, scales=None, mode=0, in_place=None):
        """cols: (batch, n, 8) word arrays, one device buffer each -> the output words (batch, n, 8); in_place: the column d_out is.
        Checks the return code, the guards and that no input but the output changed."""
        ds = [self.buffer(c) for c in cols]
        assert all(d.data_bytes == self.bytes for d in ds)
        out = ds[in_place] if in_place is not None else self.buffer(nbytes=self.bytes)
        rc = self.call([d.ptr.value for d in ds], terms, out.ptr.value, scales, mode)
        assert rc == 0, rc
        for k, d in enumerate(ds):
            assert self.guard_intact(d) if k == in_place else self.intact(d), "a column or the bytes behind the batch were written"
        assert self.guard_intact(out)
        return self.get(out).reshape(self.batch, self.n, 8)


def _check(gm, field, cols, terms, scales=None, mode=0, in_place=None):
    """run the expression on plain-residue columns and compare with the definition"""
    batch, n = len(cols[0]), len(cols[0][0])
    h = Harness(gm, field, n, batch)
    try:
        got = h.run([_col_words(field, c) for c in cols], terms, scales, mode, in_place)
    finally:
        h.close()
    want = _expected(field, cols, terms, scales, mode)
    assert np.array_equal(got, want), (field, n, batch, np.flatnonzero((got != want).any(axis=2).reshape(-1))[:8])
    return got


def _gate_columns(field, seed, batch, n, planted=False):
    r = fr.modulus(field)
    cols = [fr.random_rows(field, seed + k, batch, n, nonzero=(k == 3)) for k in range(8)]
    if planted:  # c = -(q_L a + q_R b + q_M a b + q_C) / q_O
        ql, qr, qm, qo, qc, a, b, _ = cols
        cols[7] = [[-(ql[p][i] * a[p][i] + qr[p][i] * b[p][i] + qm[p][i] * a[p][i] * b[p][i] + qc[p][i]) * pow(qo[p][i], -1, r) % r for i in range(n)]
                   for p in range(batch)]
    return cols


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 3])
def test_gate_at_the_boundary_sizes(gm, batch):
    T = _tile()
    for n in (1, 2, 3, T - 1, T, T + 1, 2 * T + 5):
        _check(gm, 0, _gate_columns(0, 0x1A000 + n, batch, n), GATE)
        zero = _check(gm, 0, _gate_columns(0, 0x1B000 + n, batch, n, planted=True), GATE)
        assert not zero.any(), "a satisfied gate evaluates to zero everywhere"


@pytest.mark.gpu
def test_rotations_wrap_inside_their_vector(gm):
    T = _tile()
    for n in (3, T + 1):
        x = fr.random_rows(0, 0x2A000 + n, 2, n)
        assert x[0] != x[1]
        xw = _col_words(0, x)
        for rot in (1, -1, n - 1, n, n + 1, -n, -(1 << 31)):
            got = _check(gm, 0, [x], [(1, [(0, rot)])])
            shift = rot % n
            for p in range(2):
                assert np.array_equal(got[p], np.roll(xw[p], -shift, axis=0)), (n, rot, p)


@pytest.mark.gpu
def test_the_grand_product_closes(gm):
    """Z from panda_poly_grand_product on a permuted multiset: Z[i+1] den[i] - Z[i] num[i] is zero at every i, at i = n - 1 because Z closes"""
    n = 3 * _tile() + 5
    r = fr.modulus(0)
    den = fr.random_rows(0, 0x3A000, 1, n, nonzero=True)
    perm = np.random.default_rng(3).permutation(n)
    num = [[den[0][j] for j in perm]]
    zs, totals = pgm.panda_poly_gpu_grand_product(gm, [_col_words(0, num)[0]], [_col_words(0, den)[0]])
    assert np.array_equal(totals[0], fr.wire(0, [1])[0])
    z = [fr.plain(0, zs[0])]
    got = _check(gm, 0, [z, den, num], [(1, [(0, 1), (1, 0)]), (r - 1, [(0, 0), (2, 0)])])
    assert not got.any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fill", "copy", "coefficient_zero", "square", "all_minus_one_64x4", "degree_256", "columns_32"])
def test_edge_expressions(gm, case):
    n, batch, r = _tile() + 1, 2, fr.modulus(0)
    x, y = fr.random_rows(0, 0x4A000, batch, n), fr.random_rows(0, 0x4B000, batch, n)
    if case == "fill":
        got = _check(gm, 0, [x], [(12345, [])])
        assert np.array_equal(got, np.broadcast_to(fr.wire(0, [12345])[0], (batch, n, 8)))
    elif case == "copy":
        got = _check(gm, 0, [x], [(1, [(0, 0)])])
        assert np.array_equal(got, _col_words(0, x))
    elif case == "coefficient_zero":
        got = _check(gm, 0, [x, y], [(0, [(0, 0), (1, 0)]), (1, [(1, 0)]), (0, [])])
        assert np.array_equal(got, _col_words(0, y))
        assert not _check(gm, 0, [x], [(0, [(0, 0)])]).any()
    elif case == "square":
        _check(gm, 0, [x], [(1, [(0, 0), (0, 0)])])
        _check(gm, 0, [x], [(r - 1, [(0, 0), (0, 1), (0, 0)]), (7, [])])
    elif case == "all_minus_one_64x4":
        m1 = [[r - 1] * n for _ in range(batch)]
        got = _check(gm, 0, [m1, m1], [(r - 1, [(t & 1, t), (0, -t), (1, 0), (t & 1, 1)]) for t in range(64)], scales=[r - 1], mode=1)
        assert np.array_equal(got, np.broadcast_to(fr.wire(0, [64])[0], (batch, n, 8))), "64 x (-1)^5, times -1"
    elif case == "degree_256":
        _check(gm, 0, [x, y], [(r - 1, [(f & 1, f - 128) for f in range(256)])])
    else:  # 32 column pointers, the cap: 31 into one buffer and one apart
        cols = [x] * 31 + [y]
        h = Harness(gm, 0, n, batch)
        try:
            dx, dy, out = h.buffer(_col_words(0, x)), h.buffer(_col_words(0, y)), h.buffer(nbytes=h.bytes)
            terms = [(c + 1, [(c, c)]) for c in range(32)]
            assert h.call([dx.ptr.value] * 31 + [dy.ptr.value], terms, out.ptr.value) == 0
            assert np.array_equal(h.get(out).reshape(batch, n, 8), _expected(0, cols, terms)) and h.guard_intact(out)
        finally:
            h.close()


@pytest.mark.gpu
def test_columns_overlapping_by_half_a_vector(gm):
    n, r = _tile() + 2, fr.modulus(0)
    half = n // 2
    data = fr.random_rows(0, 0x5A000, 1, n + half)[0]
    h = Harness(gm, 0, n, 1)
    try:
        d = h.buffer(fr.wire(0, data))
        out = h.buffer(nbytes=h.bytes)
        terms = [(1, [(0, 0), (1, 0)]), (r - 1, [(1, 1)]), (3, [(0, -1)])]
        assert h.call([d.ptr.value, d.ptr.value + half * 32], terms, out.ptr.value) == 0
        want = _expected(0, [[data[:n]], [data[half:half + n]]], terms)
        assert np.array_equal(h.get(out).reshape(1, n, 8), want)
        assert h.guard_intact(out) and h.intact(d)
    finally:
        h.close()


@pytest.mark.gpu
def test_scales(gm):
    T, r = _tile(), fr.modulus(0)
    s = fr.random_rows(0, 0x6A000, 1, 16)[0]
    terms = [(1, [(0, 0), (1, 0)]), (r - 1, [(2, 1)])]
    cols = [fr.random_rows(0, 0x6B000 + k, 5, T + 1) for k in range(3)]
    _check(gm, 0, cols, terms, scales=s[:4], mode=1)  # PER_VECTOR, batch 5 over 4 scales: vector 4 takes scale 0
    for n in (3, T + 1):
        cols = [fr.random_rows(0, 0x6C000 + n + k, 2, n) for k in range(3)]
        _check(gm, 0, cols, terms, scales=s, mode=2)  # CYCLIC with 16 scales
        _check(gm, 0, cols, terms, scales=s[:5], mode=2)
        plain = _check(gm, 0, cols, terms)  # NONE with scales == NULL
        h = Harness(gm, 0, n, 2)
        try:  # NONE ignores a scales array that is there
            assert np.array_equal(h.run([_col_words(0, c) for c in cols], terms, scales=s, mode=0), plain)
        finally:
            h.close()


def _quotient_setup(log_n, log_blowup):
    """a, b random on H, c = a b; coefficients and the direct evaluation of (a b - c) / (X^n - 1) on the extended coset, all integers"""
    r = fr.modulus(0)
    n, B = 1 << log_n, 1 << log_blowup
    N = n * B
    w_N = fr.plain(0, po.root_of_unity(po.F_BN254_FR, log_n + log_blowup))[0]
    w_n, g = pow(w_N, B, r), 5
    assert pow(w_N, N, r) == 1 and pow(w_N, N // 2, r) != 1
    ev_a, ev_b = fr.random_rows(0, 0x7A000, 1, n)[0], fr.random_rows(0, 0x7B000, 1, n)[0]
    ev_c = [x * y % r for x, y in zip(ev_a, ev_b)]
    ninv = pow(n, -1, r)
    coeffs = [[ninv * sum(e[k] * pow(w_n, -j * k % n, r) for k in range(n)) % r for j in range(n)] for e in (ev_a, ev_b, ev_c)]
    at = lambda f, x: sum(c * pow(x, j, r) for j, c in enumerate(f)) % r
    pts = [g * pow(w_N, m, r) % r for m in range(N)]
    quotient = [(at(coeffs[0], x) * at(coeffs[1], x) - at(coeffs[2], x)) * pow(pow(x, n, r) - 1, -1, r) % r for x in pts]
    return r, n, B, N, w_N, w_n, g, (ev_a, ev_b, ev_c), coeffs, quotient


@pytest.mark.gpu
@pytest.mark.parametrize("order", [ffi.NTT_LDE_COSET_MAJOR, ffi.NTT_LDE_NATURAL])
def test_a_real_quotient(gm, order):
    """evaluations on H -> inverse transform -> extension to the coset -> (a b - c) / Z_H by this call, against the direct O(n N) evaluation"""
    log_n, log_blowup = 5, 2
    r, n, B, N, w_N, w_n, g, evals, coeffs, quotient = _quotient_setup(log_n, log_blowup)
    omega_n, omega_N, shift = fr.wire(0, [w_n])[0], fr.wire(0, [w_N])[0], fr.wire(0, [g])[0]
    cs = []
    for e, want in zip(evals, coeffs):
        buf = np.array(fr.wire(0, e))
        pgm.panda_intt_bn254_gpu(gm, buf, omega_n, log_n)
        assert np.array_equal(buf, fr.wire(0, want))
        cs.append(buf)
    ext = pgm.panda_ntt_gpu_lde(gm, cs, omega_N, log_n, log_blowup, shift, field=0, order=order)
    zinv = [pow(pow(g, n, r) * pow(w_N, i * n, r) - 1, -1, r) for i in range(B)]  # 1 / Z_H on coset i
    terms = [(1, [(0, 0), (1, 0)]), (r - 1, [(2, 0)])]
    if order == ffi.NTT_LDE_COSET_MAJOR:  # B vectors of n; element i n + k is the value at g w_N^(i + B k)
        cols = [e.reshape(B, n, 8) for e in ext]
        want = [quotient[i + B * k] for i in range(B) for k in range(n)]
        mode = ffi.SOP_SCALE_PER_VECTOR
    else:  # one vector of N; element m is the value at g w_N^m, Z_H there depends on m mod B
        cols = [e.reshape(1, N, 8) for e in ext]
        want = quotient
        mode = ffi.SOP_SCALE_CYCLIC
    got = pgm.panda_poly_gpu_sum_of_products(gm, cols, [(fr.wire(0, [k])[0], fs) for k, fs in terms], field=0, scales=fr.wire(0, zinv), scale_mode=mode)
    assert np.array_equal(got.reshape(-1, 8), fr.wire(0, want))


@pytest.mark.gpu
def test_in_place_and_short_buffers(gm):
    from gpu_util import DeviceBuffer
    T, r = _tile(), fr.modulus(0)
    n, batch = 2 * T + 1, 2
    cols = [fr.random_rows(0, 0x8A000 + k, batch, n) for k in range(3)]
    words = [_col_words(0, c) for c in cols]
    for terms in ([(1, [(0, 0), (1, 1)]), (r - 1, [(2, -1), (0, 0)]), (5, [])],
                  [(1, [(0, n), (1, 1)]), (r - 1, [(2, -1), (0, -n)]), (5, [(0, 0), (0, 2 * n)])]):  # rotation n is rotation 0
        out = _check(gm, 0, cols, terms)
        h = Harness(gm, 0, n, batch)
        try:
            assert np.array_equal(h.run(words, terms, in_place=0), out), "in place on column 0"
        finally:
            h.close()
    h = Harness(gm, 0, n, batch)
    short = DeviceBuffer(h.bytes - 32)  # one element short
    try:
        a, b, out = h.buffer(words[0]), h.buffer(words[1]), h.buffer(nbytes=h.bytes)
        ffi.check(h.lib.panda_memset(short.ptr, GUARD, h.bytes - 32), "memset")
        terms = [(1, [(0, 0), (1, 0)])]
        assert h.call([a.ptr.value, b.ptr.value], terms, a.ptr.value + 32) == 1 and h.call([a.ptr.value, b.ptr.value], [(1, [(0, 1)])], a.ptr.value) == 1
        assert h.call([short.ptr.value, b.ptr.value], terms, out.ptr.value) == 1 and h.call([a.ptr.value, short.ptr.value], terms, out.ptr.value) == 1
        assert h.call([a.ptr.value, b.ptr.value], terms, short.ptr.value) == 1 and h.call([short.ptr.value], [(1, [(0, 0)])], short.ptr.value) == 1
        assert h.call([a.ptr.value, b.ptr.value, short.ptr.value], terms, out.ptr.value) == 1, "a short column no factor names"
        assert (short.to_host(np.uint8) == GUARD).all() and h.untouched(out), "a refused call wrote to a buffer"
        assert h.intact(a) and h.intact(b)
        assert h.call([a.ptr.value, b.ptr.value], terms, out.ptr.value) == 0
        assert np.array_equal(h.get(out).reshape(batch, n, 8), _expected(0, cols[:2], terms))
    finally:
        short.free()
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_other_fields(gm, field):
    n, r = _tile() + 1, fr.modulus(field)
    _check(gm, field, _gate_columns(field, 0x9A000 + field, 2, n), GATE + [(r - 1, [(7, 1), (5, -1)])], scales=[r - 1, 2, 3], mode=2)
    assert not _check(gm, field, _gate_columns(field, 0x9B000 + field, 2, n, planted=True), GATE).any()


@pytest.mark.gpu
def test_scratch_is_reused_and_released(gm):
    n, batch = 5 * _tile() - 7, 4
    cols = [_col_words(0, fr.random_rows(0, 0xAA000 + k, batch, n)) for k in range(2)]
    terms = [(1, [(0, 0), (1, 1)])]
    h = Harness(gm, 0, n, batch)
    try:
        a, b, out = h.buffer(cols[0]), h.buffer(cols[1]), h.buffer(nbytes=h.bytes)
        run = lambda: h.call([a.ptr.value, b.ptr.value], terms, out.ptr.value)
        assert run() == 0  # whatever the runtime keeps from a kernel's first launch is there before the baseline is read
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        before = free_bytes(h.lib)
        assert run() == 0
        first = free_bytes(h.lib)
        o1 = h.get(out)
        assert run() == 0
        assert free_bytes(h.lib) == first, "a repeated identical call allocated"
        assert np.array_equal(h.get(out), o1)
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        assert free_bytes(h.lib) == before, "panda_ntt_tear_down releases the scratch"
    finally:
        h.close()


@pytest.mark.gpu
def test_gpu_manager_helper(gm):
    n, batch, r = _tile() + 3, 3, fr.modulus(0)
    cols = [fr.random_rows(0, 0xBA000 + k, batch, n) for k in range(3)]
    words = [np.array(_col_words(0, c)) for c in cols]
    keep = [w.copy() for w in words]
    terms = [(1, [(0, 0), (1, 0)]), (r - 1, [(2, 1)]), (9, [])]
    wire_terms = [(fr.wire(0, [k])[0], fs) for k, fs in terms]
    got = pgm.panda_poly_gpu_sum_of_products(gm, words, wire_terms)
    assert got.shape == (batch, n, 8) and got.dtype == np.uint32 and np.array_equal(got, _expected(0, cols, terms))
    s = [3, r - 1]
    got = pgm.panda_poly_gpu_sum_of_products(gm, words, wire_terms, scales=fr.wire(0, s), scale_mode=ffi.SOP_SCALE_PER_VECTOR)
    assert np.array_equal(got, _expected(0, cols, terms, s, 1))
    got = pgm.panda_poly_gpu_sum_of_products(gm, [w[0] for w in words], wire_terms, scales=fr.wire(0, s), scale_mode=ffi.SOP_SCALE_CYCLIC)
    assert got.shape == (n, 8) and np.array_equal(got, _expected(0, [c[:1] for c in cols], terms, s, 2)[0])
    assert all(np.array_equal(w, k) for w, k in zip(words, keep)), "the helper changed its input"
    with pytest.raises(pgm.PandaGpuError):
        pgm.panda_poly_gpu_sum_of_products(gm, [], wire_terms)
    with pytest.raises(pgm.PandaGpuError):
        pgm.panda_poly_gpu_sum_of_products(gm, [words[0], words[1][:, :-1]], wire_terms)


@pytest.mark.gpu
@pytest.mark.gpu_soak
def test_2_24(gm):
    """a[i] b[i+1] - c[i-1] at 2^24 on generated data, sampled indices against integers"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    lib, n, r = ffi.load(), 1 << 24, fr.modulus(0)
    bufs = [DeviceBuffer(n * 32) for _ in range(4)]
    try:
        for k in range(3):
            ffi.check(lib.panda_gen_scalars(0, 0xC0 + k, 0, n, bufs[k].ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
        terms = [(1, [(0, 0), (1, 1)]), (r - 1, [(2, -1)])]
        x = Expression(0, [b.ptr.value for b in bufs[:3]], terms)
        assert lib.panda_poly_sum_of_products(0, C.byref(x.expr), bufs[3].ptr, n, 1, gm.exec_stream.raw) == 0
        elem = lambda b, i: fr.plain(0, b.to_host(np.uint32, nbytes=32, offset=(i % n) * 32))[0]
        for i in [0, 1, n - 1, n - 2, _tile() - 1, _tile()] + [int(v) for v in np.random.default_rng(24).integers(0, n, 58)]:
            assert elem(bufs[3], i) == (elem(bufs[0], i) * elem(bufs[1], i + 1) - elem(bufs[2], i - 1)) % r, i
    finally:
        for b in bufs:
            b.free()
