"""panda_sumcheck_round / panda_mle_fold / panda_mle_eq_table / panda_sumcheck_plan: sumcheck rounds over multilinear tables.

A table is 2^k wire elements; a round binds the lowest variable (pair i = f[2i], f[2i+1]) or the highest (f[i], f[i + 2^(k-1)]):

    fold    F[i] = lo + r (hi - lo)
    round   g(t) = sum_i sum_terms coeff prod_f ( lo_f + t (hi_f - lo_f) ),  t = 0 .. n_evals - 1
    eq      out[x] = prod_j ( x_j r_j + (1 - x_j)(1 - r_j) )

Expected values are Python integers with the moduli of tests/pyref.py, evaluated from these definitions on plain residues and put back on
the wire (w = x W mod r, W = 2^256).  Outputs are canonical and field addition is exact, so every comparison is byte for byte; there is no
tolerance anywhere.  The pairs one workgroup covers and the second level's chunk come from the plan call.  Every device buffer carries a
guard run of a fixed byte pattern behind the data, which no call may touch; inputs must come back unchanged unless they are an output.
A table has a power-of-two length, so the pair counts around a workgroup's span are T / 2, T, 2 T and 4 T."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import field_ref as fr
from gpu_util import GuardedBuffers, assert_exported, free_bytes, gm, run_host_check  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

NAMES = ("panda_sumcheck_round", "panda_mle_fold", "panda_mle_eq_table", "panda_sumcheck_plan")
LOW, HIGH = ffi.MLE_BIND_LOW, ffi.MLE_BIND_HIGH
# eq (q_L a + q_R b + q_M a b + q_O c + q_C): columns eq q_L q_R q_M q_O q_C a b c, degree 4
GATE_EQ = [(1, [0, 1, 6]), (1, [0, 2, 7]), (1, [0, 3, 6, 7]), (1, [0, 4, 8]), (1, [0, 5])]


def _plan(lib, log_n, fused, n_evals):
    t, c, l = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    rc = lib.panda_sumcheck_plan(log_n, fused, n_evals, C.byref(t), C.byref(c), C.byref(l))
    return rc, t.value, c.value, l.value


@functools.lru_cache(maxsize=None)
def _tile(fused=0):
    rc, tile, chunk, _ = _plan(ffi.load(), 4, fused, 2)
    assert rc == 0 and tile >= 1 and chunk >= 1
    return tile, chunk


# ------------------------------------------------------------------------------------------------- the definitions, on plain residues
def _pairs(table, order):
    half = len(table) // 2
    return [(table[i], table[i + half]) if order == HIGH else (table[2 * i], table[2 * i + 1]) for i in range(half)]


def _fold(field, table, r, order):
    p = fr.modulus(field)
    return [(lo + r * (hi - lo)) % p for lo, hi in _pairs(table, order)]


def _round(field, cols, terms, n_evals, order):
    p = fr.modulus(field)
    prs = [_pairs(c, order) for c in cols]
    out = []
    for t in range(n_evals):
        pts = [[(lo + t * (hi - lo)) % p for lo, hi in pr] for pr in prs]
        g = 0
        for i in range(len(prs[0])):
            for k, fs in terms:
                v = k
                for c in fs:
                    v = v * pts[c][i] % p
                g += v
        out.append(g % p)
    return out


def _eq(field, point):
    p = fr.modulus(field)
    table = [1]
    for r in point:  # bit j of the index is coordinate j: each coordinate doubles the table above the ones before it
        table = [v * (1 - r) % p for v in table] + [v * r % p for v in table]
    return table


def _interpolate(field, ys, x):
    """the polynomial through (t, ys[t]) at x"""
    p = fr.modulus(field)
    total = 0
    for j, y in enumerate(ys):
        num = den = 1
        for m in range(len(ys)):
            if m != j:
                num = num * (x - m) % p
                den = den * (j - m) % p
        total += y * num * pow(den, -1, p)
    return total % p


def _expression_value(field, terms, values):
    p = fr.modulus(field)
    total = 0
    for k, fs in terms:
        v = k
        for c in fs:
            v = v * values[c] % p
        total += v
    return total % p


class Expression:
    """the ctypes arrays of one panda_sop_expression; they stay alive with the object"""

    def __init__(self, field, ptrs, terms, mode=0, rotation=0, wire_coeffs=None):
        self.ptrs = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        self.coeffs = np.ascontiguousarray(wire_coeffs if wire_coeffs is not None else fr.wire(field, [k for k, _ in terms]))
        self.degrees = (C.c_uint * max(len(terms), 1))(*[len(fs) for _, fs in terms])
        flat = [c for _, fs in terms for c in fs]
        self.factors = (ffi.SopFactor * max(len(flat), 1))(*[ffi.SopFactor(c, rotation) for c in flat])
        self.expr = ffi.SopExpression(self.ptrs, C.c_void_p(self.coeffs.ctypes.data), self.degrees, self.factors, None, len(ptrs), len(terms), 0, mode)


def _pointer_array(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*ptrs)


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, _ = assert_exported(NAMES)
    for macro, value in (("MLE_BIND_LOW", ffi.MLE_BIND_LOW), ("MLE_BIND_HIGH", ffi.MLE_BIND_HIGH), ("SUMCHECK_MAX_EVALS", ffi.SUMCHECK_MAX_EVALS)):
        assert int(re.search(r"#define\s+PANDA_%s\s+(\d+)" % macro, header).group(1)) == value
    assert (ffi.MLE_BIND_LOW, ffi.MLE_BIND_HIGH, ffi.SUMCHECK_MAX_EVALS) == (0, 1, 8)


def test_plan():
    lib = ffi.load()
    for fused in (0, 1):
        seen = set()
        for log_n in range(1 + fused, 29):
            for n_evals in range(1, ffi.SUMCHECK_MAX_EVALS + 1):
                rc, tile, chunk, launches = _plan(lib, log_n, fused, n_evals)
                assert rc == 0 and tile >= 1 and tile & (tile - 1) == 0 and chunk >= 1 and launches == 2, (log_n, fused, n_evals)
                seen.add((tile, chunk))
        assert len(seen) == 1, "neither value depends on the size or the point count"
        assert lib.panda_sumcheck_plan(5, fused, 3, None, None, None) == 0
        for log_n, n_evals in ((fused, 2), (0, 2), (29, 2), (0xFFFFFFFF, 2), (5, 0), (5, ffi.SUMCHECK_MAX_EVALS + 1), (5, 0xFFFFFFFF)):
            t = C.c_uint(0xDEAD)
            assert lib.panda_sumcheck_plan(log_n, fused, n_evals, C.byref(t), None, None) == 1 and t.value == 0xDEAD, (log_n, fused, n_evals)
    assert lib.panda_sumcheck_plan(5, 2, 2, None, None, None) == 1


def test_bad_arguments_are_refused_before_any_device_call():
    """every refusal of the contract returns 1 with the host outputs untouched -- also on a machine with no device.  Host memory stands in
    for the device buffers: nothing may dereference it."""
    lib = ffi.load()
    log_n = 4
    nbytes = 32 << log_n  # 512, folded 256
    mem = np.full(8 << 20, 0x5A, np.uint8)  # eight disjoint 1 MiB ranges
    base = mem.ctypes.data
    A, B, D, FA, FB, FD, O = (base + (k << 20) + 4096 for k in range(7))
    stream = ffi.PandaStream()
    one_term = [(1, [0, 1])]
    count = [0]

    def rnd(field=0, ptrs=(A, B, D), terms=one_term, log_n=log_n, order=LOW, n_evals=3, challenge=None, folded=None, mode=0, rotation=0,
            wire_coeffs=None, patch=None, expr_null=False, evals_null=False, wire_challenge=None):
        x = Expression(min(field, 2), list(ptrs), terms, mode, rotation, wire_coeffs)
        if patch:
            patch(x.expr)
        evals = np.full((8, 8), 0x77777777, np.uint32)
        ch = wire_challenge if wire_challenge is not None else (None if challenge is None else fr.wire(min(field, 2), [challenge]))
        fp = None if folded is None else _pointer_array(list(folded))
        rc = lib.panda_sumcheck_round(field, None if expr_null else C.byref(x.expr), log_n, order, n_evals, None if ch is None else C.c_void_p(ch.ctypes.data),
                                      fp, None if evals_null else C.c_void_p(evals.ctypes.data), stream)
        assert (evals == 0x77777777).all(), "a refused call wrote its output"
        count[0] += 1
        return rc

    def fold(field=0, cols=(A, B), folded=(FA, FB), n_columns=None, log_n=log_n, order=LOW, challenge=5, wire_challenge=None, cols_null=False,
             folded_null=False, challenge_null=False):
        ch = wire_challenge if wire_challenge is not None else fr.wire(min(field, 2), [challenge])
        count[0] += 1
        return lib.panda_mle_fold(field, None if cols_null else _pointer_array(list(cols)), None if folded_null else _pointer_array(list(folded)),
                                  len(cols) if n_columns is None else n_columns, log_n, order, None if challenge_null else C.c_void_p(ch.ctypes.data), stream)

    def eq(field=0, point=(1, 2, 3), log_n=None, out=O, point_null=False, wire_point=None):
        pt = wire_point if wire_point is not None else fr.wire(min(field, 2), list(point) or [0])
        count[0] += 1
        return lib.panda_mle_eq_table(field, None if point_null else C.c_void_p(pt.ctypes.data), len(point) if log_n is None else log_n,
                                      None if out is None else C.c_void_p(out), stream)

    def null(member):
        def patch(e):
            setattr(e, member, None)
        return patch

    def member(name, value):
        def patch(e):
            setattr(e, name, value)
        return patch

    fused = dict(challenge=7, folded=(FA, FB, FD))
    # shapes
    assert rnd(field=3) == 1 and rnd(log_n=0) == 1 and rnd(log_n=29) == 1 and rnd(order=2) == 1 and rnd(n_evals=0) == 1 and rnd(n_evals=9) == 1
    assert rnd(log_n=1, **fused) == 1 and rnd(log_n=0, **fused) == 1 and rnd(log_n=29, **fused) == 1 and rnd(field=3, **fused) == 1
    assert fold(field=3) == 1 and fold(log_n=0) == 1 and fold(log_n=29) == 1 and fold(order=2) == 1 and fold(n_columns=0) == 1
    assert fold(cols=[A] * 33, folded=[FA + 256 * k for k in range(33)]) == 1
    assert eq(field=3) == 1 and eq(log_n=29) == 1
    # pointers
    assert rnd(expr_null=True) == 1 and rnd(evals_null=True) == 1
    assert rnd(patch=null("columns")) == 1 and rnd(patch=null("coeffs")) == 1 and rnd(patch=null("degrees")) == 1 and rnd(patch=null("factors")) == 1
    for k in range(3):
        assert rnd(ptrs=[None if j == k else q for j, q in enumerate((A, B, D))]) == 1, "a NULL column pointer"
        assert rnd(challenge=7, folded=[None if j == k else q for j, q in enumerate((FA, FB, FD))]) == 1, "a NULL folded pointer"
    assert rnd(challenge=7) == 1 and rnd(folded=(FA, FB, FD)) == 1, "exactly one of challenge / folded"
    assert fold(cols_null=True) == 1 and fold(folded_null=True) == 1 and fold(challenge_null=True) == 1
    assert fold(cols=(A, None)) == 1 and fold(folded=(None, FB)) == 1
    assert eq(point_null=True) == 1 and eq(out=None) == 1 and eq(point=(), point_null=True) == 1
    # the expression errors of the sum of products
    many = [(1, [0])] * (ffi.SOP_MAX_TERMS + 1)
    assert rnd(patch=member("n_columns", 0)) == 1 and rnd(ptrs=[A] * (ffi.SOP_MAX_COLUMNS + 1), terms=[(1, [0])]) == 1
    assert rnd(terms=many, patch=member("n_terms", 0)) == 1 and rnd(terms=many) == 1
    assert rnd(terms=[(1, [0] * (ffi.SOP_MAX_FACTORS + 1))]) == 1
    assert rnd(terms=[(1, [0] * 4)] * (ffi.SOP_MAX_TERMS - 1) + [(1, [0] * 5)]) == 1, "63 x 4 + 5 = 257 factors"
    assert rnd(terms=[(1, [0, 3])]) == 1 and rnd(terms=[(1, [0xFFFFFFFF])]) == 1, "column index >= n_columns"
    # rotations and scale modes
    assert rnd(rotation=1) == 1 and rnd(rotation=-1) == 1 and rnd(rotation=1 << log_n) == 1 and rnd(rotation=1, **fused) == 1
    assert rnd(mode=1) == 1 and rnd(mode=2) == 1 and rnd(mode=3) == 1 and rnd(mode=1, **fused) == 1
    # constants at and above the modulus, per field
    for field in (0, 1, 2):
        r = fr.modulus(field)
        for bad in (r, r + 1, fr.W - 1):
            assert rnd(field=field, wire_coeffs=fr.words([bad])) == 1
            assert rnd(field=field, terms=[(1, [0]), (1, [1])], wire_coeffs=fr.words([1, bad])) == 1
            assert rnd(field=field, folded=(FA, FB, FD), wire_challenge=fr.words([bad])) == 1
            assert fold(field=field, wire_challenge=fr.words([bad])) == 1
            assert eq(field=field, wire_point=fr.words([1, bad, 2])) == 1
    # overlaps
    for order in (LOW, HIGH):
        assert rnd(order=order, challenge=7, folded=(FA, FA + 128, FD)) == 1 and fold(order=order, folded=(FA, FA + 255)) == 1, "two overlapping folded ranges"
        assert rnd(order=order, challenge=7, folded=(FA, FA, FD)) == 1 and fold(order=order, folded=(FA, FA)) == 1
        for off in (32, -32, nbytes - 1, -255):
            assert rnd(order=order, challenge=7, folded=(A + off, FB, FD)) == 1, ("a partial overlap with its own column", off)
            assert rnd(order=order, challenge=7, folded=(FA, B + off, FD)) == 1 and fold(order=order, folded=(FA, B + off)) == 1
            assert rnd(order=order, challenge=7, folded=(B + off, FB, FD)) == 1, "a folded range over another column"
        assert rnd(order=order, challenge=7, folded=(B, FB, FD)) == 1 and fold(order=order, folded=(B, FB)) == 1, "another column's pointer exactly"
    assert rnd(order=LOW, challenge=7, folded=(A, FB, FD)) == 1 and fold(order=LOW, folded=(A, FB)) == 1, "BIND_LOW in place"
    assert rnd(order=LOW, challenge=7, folded=(A, B, D)) == 1 and fold(order=LOW, folded=(A, B)) == 1
    for second in (A, A + 32, A + nbytes - 32, A - nbytes + 32):
        assert rnd(order=HIGH, ptrs=(A, second, D), challenge=7, folded=(A, FB, FD)) == 1, "BIND_HIGH in place with a second column on the first"
        assert fold(order=HIGH, cols=(A, second), folded=(A, FB)) == 1
    assert (mem == 0x5A).all(), "a refused call wrote to a buffer"
    assert count[0] > 150


def test_host_program_checks_the_bounds(tmp_path):
    """tests/host_check/sumcheck_host.cpp: the round's program builder, the per-pair routine the kernel runs (plain and fused), the fold and
    the eq table's factors, on the host under FE29_CHECK, against 256-bit arithmetic of its own -- every operand p - 1, lo = 0 with
    hi = p - 1 and the reverse, 64 terms of degree 4, one term of degree 256, 1 and 8 points, challenges 0, 1 and p - 1, the three fields"""
    assert run_host_check(tmp_path, "sumcheck_host.cpp") >= 1000


# ------------------------------------------------------------------------------------------------- on the device
class Dev(GuardedBuffers):
    """guarded device buffers, and the calls over them"""

    def __init__(self, gm, field=0):
        super().__init__()
        self.lib, self.field, self.stream = ffi.load(), field, gm.exec_stream.raw

    def rows(self, d):
        return self.get(d).reshape(-1, 8)

    def round(self, ptrs, terms, log_n, order, n_evals, challenge=None, folded=None):
        """-> (rc, evals words (n_evals, 8)); challenge a plain residue"""
        x = Expression(self.field, ptrs, terms)
        evals = np.zeros((n_evals, 8), np.uint32)
        ch = None if challenge is None else fr.wire(self.field, [challenge])
        rc = self.lib.panda_sumcheck_round(self.field, C.byref(x.expr), log_n, order, n_evals, None if ch is None else C.c_void_p(ch.ctypes.data),
                                           None if folded is None else _pointer_array(folded), C.c_void_p(evals.ctypes.data), self.stream)
        return rc, evals

    def fold(self, ptrs, folded, log_n, order, challenge):
        ch = fr.wire(self.field, [challenge])
        return self.lib.panda_mle_fold(self.field, _pointer_array(ptrs), _pointer_array(folded), len(ptrs), log_n, order, C.c_void_p(ch.ctypes.data), self.stream)


def _check_round(gm, field, cols, terms, n_evals, order, challenge=None, same_buffer=()):
    """The plain round on plain-residue tables against the definition; with a challenge also the fused round, against the definition and,
    byte for byte, against panda_mle_fold followed by the plain round on its output.  Returns the plain round's evaluations (words)."""
    n = len(cols[0])
    log_n = n.bit_length() - 1
    words = [fr.wire(field, c) for c in cols]
    h = Dev(gm, field)
    try:
        ds = []
        for k, w in enumerate(words):
            ds.append(ds[same_buffer[k]] if k < len(same_buffer) and same_buffer[k] is not None else h.buffer(w))
        ptrs = [d.ptr.value for d in ds]
        rc, got = h.round(ptrs, terms, log_n, order, n_evals)
        assert rc == 0
        assert np.array_equal(got, fr.wire(field, _round(field, cols, terms, n_evals, order))), (field, log_n, order, "plain")
        if challenge is not None and log_n >= 2:
            fs = [h.buffer(nbytes=n * 16) for _ in cols]
            rc, fused = h.round(ptrs, terms, log_n, order, n_evals, challenge, [f.ptr.value for f in fs])
            assert rc == 0
            folded = [_fold(field, c, challenge, order) for c in cols]
            assert np.array_equal(fused, fr.wire(field, _round(field, folded, terms, n_evals, order))), (field, log_n, order, "fused")
            us = [h.buffer(nbytes=n * 16) for _ in cols]
            assert h.fold(ptrs, [u.ptr.value for u in us], log_n, order, challenge) == 0
            rc, unfused = h.round([u.ptr.value for u in us], terms, log_n - 1, order, n_evals)
            assert rc == 0 and np.array_equal(fused, unfused)
            for k in range(len(cols)):
                want = fr.wire(field, folded[k])
                assert np.array_equal(h.rows(fs[k]), want) and np.array_equal(h.rows(us[k]), want), (field, log_n, order, k)
                assert h.guard_intact(fs[k]) and h.guard_intact(us[k]), "bytes behind a folded table were written"
        for d, w in zip(ds, words):
            assert h.guard_intact(d) and np.array_equal(h.rows(d), w), "a column was written"
        return got
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", [LOW, HIGH])
def test_gate_times_eq_at_the_boundary_sizes(gm, order):
    T = _tile()[0]
    assert _tile(1)[0] == T
    top = T.bit_length() - 1  # pairs T / 2 at this log_n; T, 2 T, 4 T follow (the fused round's pair counts are half of these)
    for log_n in (1, 2, 3, top, top + 1, top + 2, top + 3):
        n = 1 << log_n
        cols = [fr.random_residues(0, 0x1A000 + 16 * log_n + k, n) for k in range(9)]
        _check_round(gm, 0, cols, GATE_EQ, 5, order, challenge=fr.random_residues(0, 0x1B000 + log_n, 1)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
def test_more_tiles_than_the_second_level_takes_per_step(gm, fused):
    """one column f[x] = x mod 251 + 1, the terms f and f f, more than carry_chunk tile sums per point; numpy int64 sums reduced in Python"""
    T, chunk = _tile(fused)
    log_pairs = (chunk * T).bit_length()  # the smallest power of two above chunk * T
    assert 1 << log_pairs > chunk * T >= 1 << (log_pairs - 1)
    log_n = log_pairs + 1 + fused
    p, r = fr.modulus(0), 3
    small = fr.wire(0, range(252))
    x = np.arange(1 << log_n, dtype=np.int64) % 251 + 1
    terms = [(1, [0]), (1, [0, 0])]
    h = Dev(gm, 0)
    try:
        d = h.buffer(small[x])
        for order in (LOW, HIGH):
            halves = lambda v: (v[:len(v) // 2], v[len(v) // 2:]) if order == HIGH else (v[0::2], v[1::2])
            lo, hi = halves(x)
            if fused:
                folded = lo + r * (hi - lo)  # may be negative: the residue is taken below
                out = h.buffer(nbytes=16 << log_n)
                rc, got = h.round([d.ptr.value], terms, log_n, order, 3, r, [out.ptr.value])
                idx = np.random.default_rng(7).integers(0, len(folded), 200).tolist() + [0, len(folded) - 1]
                assert np.array_equal(h.rows(out)[idx], fr.wire(0, [int(folded[i]) for i in idx])) and h.guard_intact(out)
                lo, hi = halves(folded)
            else:
                rc, got = h.round([d.ptr.value], terms, log_n, order, 3)
            assert rc == 0
            want = [(int((lo + t * (hi - lo)).sum()) + int(((lo + t * (hi - lo)) ** 2).sum())) % p for t in range(3)]
            assert np.array_equal(got, fr.wire(0, want)), (fused, order)
            if not fused and order == HIGH:  # g(0) of the degree-1 term is the sum of the first half
                rc, g = h.round([d.ptr.value], terms[:1], log_n, order, 1)
                total = np.zeros((1, 8), np.uint32)
                assert h.lib.panda_poly_running_sum(0, d.ptr, None, 1 << (log_n - 1), 1, C.c_void_p(total.ctypes.data), h.stream) == 0
                assert rc == 0 and np.array_equal(g, total)
        assert h.guard_intact(d) and np.array_equal(d.to_host(np.uint32, nbytes=32 * 1000).reshape(-1, 8), small[x[:1000]])
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["constant", "column_twice", "same_buffer", "coefficients", "one_point", "eight_points", "zeros", "minus_ones"])
def test_edge_expressions(gm, case):
    log_n, p = _tile()[0].bit_length() + 1, fr.modulus(0)  # 2 T pairs
    n = 1 << log_n
    x, y = fr.random_residues(0, 0x4A000, n), fr.random_residues(0, 0x4B000, n)
    r = fr.random_residues(0, 0x4C000, 1)[0]
    for order in (LOW, HIGH):
        if case == "constant":
            got = _check_round(gm, 0, [x], [(12345, [])], 3, order, challenge=r)
            assert np.array_equal(got, fr.wire(0, [12345 * (n // 2)] * 3)), "g(t) = coeff 2^(log_n - 1)"
        elif case == "column_twice":
            _check_round(gm, 0, [x, y], [(1, [0, 0]), (p - 1, [1, 0, 1])], 4, order, challenge=r)
        elif case == "same_buffer":
            _check_round(gm, 0, [x, x, y], [(1, [0, 1]), (3, [1, 2])], 3, order, same_buffer=(None, 0))
        elif case == "coefficients":
            got = _check_round(gm, 0, [x, y], [(0, [0, 1]), (p - 1, [1]), (0, [])], 3, order, challenge=r)
            assert np.array_equal(got, fr.wire(0, [-v for v in _round(0, [y], [(1, [0])], 3, order)]))
            assert not _check_round(gm, 0, [x], [(0, [0])], 2, order, challenge=r).any()
        elif case == "one_point":
            _check_round(gm, 0, [x, y], [(1, [0, 1]), (7, [])], 1, order, challenge=r)
        elif case == "eight_points":
            _check_round(gm, 0, [x, y], [(p - 1, [0, 1, 0, 1, 0, 1, 0]), (5, [1])], 8, order, challenge=r)
            _check_round(gm, 0, [x, y], [(1, [0, 1, 0, 1, 0, 1, 0])], 7, order, challenge=p - 1)
        elif case == "zeros":
            assert not _check_round(gm, 0, [[0] * n] * 9, GATE_EQ, 5, order, challenge=r).any()
        else:
            m1 = [p - 1] * n
            _check_round(gm, 0, [m1] * 9, [(p - 1, fs) for _, fs in GATE_EQ], 5, order, challenge=p - 1)
            _check_round(gm, 0, [m1, m1], [(p - 1, [t & 1, 0, 1, t & 1]) for t in range(64)], 5, order, challenge=r)


def _device_sumcheck(gm, field, cols, terms, n_evals, challenges, order, fused):
    """the call sequence of a whole sumcheck on plain-residue tables -> (round evaluations, final values), plain residues"""
    k = len(challenges)
    h = Dev(gm, field)
    try:
        cur = [h.buffer(fr.wire(field, c)) for c in cols]
        evals = []
        rc, e = h.round([d.ptr.value for d in cur], terms, k, order, n_evals)
        assert rc == 0
        evals.append(fr.plain(field, e))
        for j in range(1, k):
            nxt = [h.buffer(nbytes=32 << (k - j)) for _ in cols]
            if fused:
                rc, e = h.round([d.ptr.value for d in cur], terms, k - j + 1, order, n_evals, challenges[j - 1], [d.ptr.value for d in nxt])
            else:
                assert h.fold([d.ptr.value for d in cur], [d.ptr.value for d in nxt], k - j + 1, order, challenges[j - 1]) == 0
                rc, e = h.round([d.ptr.value for d in nxt], terms, k - j, order, n_evals)
            assert rc == 0 and all(h.guard_intact(d) for d in nxt)
            evals.append(fr.plain(field, e))
            cur = nxt
        last = [h.buffer(nbytes=32) for _ in cols]
        assert h.fold([d.ptr.value for d in cur], [d.ptr.value for d in last], 1, order, challenges[k - 1]) == 0
        assert all(h.guard_intact(d) for d in last)
        return evals, [fr.plain(field, h.rows(d))[0] for d in last]
    finally:
        h.close()


def _verify_sumcheck(field, cols, terms, evals, finals, challenges, order):
    """the verifier's checks, and the final values against sum_x f(x) eq(r, x)"""
    p, k = fr.modulus(field), len(challenges)
    claim = sum(_expression_value(field, terms, [c[x] for c in cols]) for x in range(1 << k)) % p  # the true hypercube sum
    for j in range(k):
        assert (evals[j][0] + evals[j][1]) % p == claim, ("round", j)
        claim = _interpolate(field, evals[j], challenges[j])
    assert _expression_value(field, terms, finals) == claim
    point = list(challenges) if order == LOW else list(challenges)[::-1]  # coordinate j belongs to bit j of the index
    weights = _eq(field, point)
    for c, v in zip(cols, finals):
        assert v == sum(a * b for a, b in zip(c, weights)) % p
    return point


@functools.lru_cache(maxsize=None)
def _sumcheck_instance():
    """k = 10, the gate times eq: the eq column from panda_mle_eq_table's definition at a random point, the others random"""
    k = 10
    z = fr.random_residues(0, 0x5A000, k)
    cols = [_eq(0, z)] + [fr.random_residues(0, 0x5B000 + c, 1 << k) for c in range(8)]
    return k, cols, fr.random_residues(0, 0x5C000, k)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [LOW, HIGH])
@pytest.mark.parametrize("fused", [False, True])
def test_a_whole_sumcheck(gm, order, fused):
    k, cols, challenges = _sumcheck_instance()
    evals, finals = _device_sumcheck(gm, 0, cols, GATE_EQ, 5, challenges, order, fused)
    point = _verify_sumcheck(0, cols, GATE_EQ, evals, finals, challenges, order)
    # multilinear evaluation by composition: g(0) + g(1) of the term f eq(point, .)
    table = pgm.panda_mle_gpu_eq_table(gm, fr.wire(0, point))
    assert np.array_equal(table, fr.wire(0, _eq(0, point)))
    h = Dev(gm, 0)
    try:
        rc, g = h.round([h.buffer(fr.wire(0, cols[6])).ptr.value, h.buffer(table).ptr.value], [(1, [0, 1])], k, order, 2)
        assert rc == 0 and sum(fr.plain(0, g)) % fr.modulus(0) == finals[6]
    finally:
        h.close()


@pytest.mark.gpu
def test_eq_table(gm):
    p = fr.modulus(0)
    # a workgroup of the eq kernel covers 2^11 elements; 12 and 13 take two and four
    for log_n in (0, 1, 2, 11, 12, 13):
        point = fr.random_residues(0, 0x6A000 + log_n, log_n)
        for j, v in zip(range(0, log_n, 3), (0, 1, p - 1, 1, 0)):
            point[j] = v
        h = Dev(gm, 0)
        try:
            out = h.buffer(nbytes=32 << log_n)
            pt = fr.wire(0, point or [0])
            assert h.lib.panda_mle_eq_table(0, C.c_void_p(pt.ctypes.data), log_n, out.ptr, h.stream) == 0
            got = h.rows(out)
            assert h.guard_intact(out)
        finally:
            h.close()
        assert np.array_equal(got, fr.wire(0, _eq(0, point))), log_n
        assert sum(fr.plain(0, got)) % p == 1, "the table sums to one"
    bits = [1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 1, 0]  # a 0 / 1 point: the indicator of one index
    got = pgm.panda_mle_gpu_eq_table(gm, fr.wire(0, bits))
    want = np.zeros((1 << len(bits), 8), np.uint32)
    want[sum(b << j for j, b in enumerate(bits))] = fr.wire(0, [1])[0]
    assert np.array_equal(got, want)
    assert np.array_equal(pgm.panda_mle_gpu_eq_table(gm, np.zeros((0, 8), np.uint32)), fr.wire(0, [1]))


@pytest.mark.gpu
def test_fold(gm):
    T, p = _tile()[0], fr.modulus(0)
    r = fr.random_residues(0, 0x7A000, 1)[0]
    for n_columns, log_n in ((1, 1), (3, T.bit_length() + 1), (32, 5), (1, T.bit_length())):
        n = 1 << log_n
        cols = [fr.random_residues(0, 0x7B000 + 64 * log_n + k, n) for k in range(n_columns)]
        for order in (LOW, HIGH):
            h = Dev(gm, 0)
            try:
                ds = [h.buffer(fr.wire(0, c)) for c in cols]
                fs = [h.buffer(nbytes=n * 16) for _ in cols]
                for ch in (r, 0, 1, p - 1):
                    assert h.fold([d.ptr.value for d in ds], [f.ptr.value for f in fs], log_n, order, ch) == 0
                    for c, d, f in zip(cols, ds, fs):
                        want = _fold(0, c, ch, order)
                        if ch in (0, 1):
                            assert want == [pr[ch] for pr in _pairs(c, order)], "challenge 0 yields lo, challenge 1 hi"
                        assert np.array_equal(h.rows(f), fr.wire(0, want)) and h.guard_intact(f)
                        assert np.array_equal(h.rows(d), fr.wire(0, c)) and h.guard_intact(d)
                if order == HIGH:  # in place: the first half of every table becomes its fold
                    assert h.fold([d.ptr.value for d in ds], [d.ptr.value for d in ds], log_n, order, r) == 0
                    for c, d in zip(cols, ds):
                        assert np.array_equal(h.rows(d), np.concatenate([fr.wire(0, _fold(0, c, r, order)), fr.wire(0, c[n // 2:])])) and h.guard_intact(d)
            finally:
                h.close()


@pytest.mark.gpu
def test_in_place_fused_round_and_short_buffers(gm):
    from gpu_util import DeviceBuffer
    log_n = _tile()[0].bit_length() + 1
    n = 1 << log_n
    cols = [fr.random_residues(0, 0x8A000 + k, n) for k in range(3)]
    terms = [(1, [0, 1]), (2, [1, 0, 0])]  # column 2 is named by no factor and is folded all the same
    r = fr.random_residues(0, 0x8B000, 1)[0]
    h = Dev(gm, 0)
    try:
        ds = [h.buffer(fr.wire(0, c)) for c in cols]
        ptrs = [d.ptr.value for d in ds]
        rc, got = h.round(ptrs, terms, log_n, HIGH, 4, r, ptrs)
        folded = [_fold(0, c, r, HIGH) for c in cols]
        assert rc == 0 and np.array_equal(got, fr.wire(0, _round(0, folded, terms, 4, HIGH)))
        for c, f, d in zip(cols, folded, ds):
            assert np.array_equal(h.rows(d), np.concatenate([fr.wire(0, f), fr.wire(0, c[n // 2:])])) and h.guard_intact(d)
        # buffers of the library's allocator shorter than stated
        short, half, out = DeviceBuffer(32 * n - 32), DeviceBuffer(16 * n - 32), DeviceBuffer(16 * n)
        h.bufs += [short, half, out]
        assert h.round([short.ptr.value], [(1, [0])], log_n, LOW, 2)[0] == 1
        assert h.round([ds[0].ptr.value], [(1, [0])], log_n, LOW, 2, r, [half.ptr.value])[0] == 1
        assert h.fold([short.ptr.value], [out.ptr.value], log_n, LOW, r) == 1 and h.fold([ds[0].ptr.value], [half.ptr.value], log_n, LOW, r) == 1
        pt = fr.wire(0, [1] * log_n)
        assert h.lib.panda_mle_eq_table(0, C.c_void_p(pt.ctypes.data), log_n, short.ptr, h.stream) == 1
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_other_fields(gm, field):
    log_n = _tile()[0].bit_length() + 1
    cols = [fr.random_residues(field, 0x9A000 + field * 16 + k, 1 << log_n) for k in range(9)]
    for order in (LOW, HIGH):
        _check_round(gm, field, cols, GATE_EQ, 5, order, challenge=fr.random_residues(field, 0x9B000 + field, 1)[0])
    point = [0, 1, fr.modulus(field) - 1] + fr.random_residues(field, 0x9C000, 3)
    assert np.array_equal(pgm.panda_mle_gpu_eq_table(gm, fr.wire(field, point), field), fr.wire(field, _eq(field, point)))


@pytest.mark.gpu
def test_scratch_is_reused_and_released(gm):
    log_n = _tile()[0].bit_length() + 3
    cols = [fr.wire(0, fr.random_residues(0, 0xAA000 + k, 1 << log_n)) for k in range(2)]
    terms = [(1, [0, 1])]
    h = Dev(gm, 0)
    try:
        a, b = h.buffer(cols[0]), h.buffer(cols[1])
        fa, fb = h.buffer(nbytes=16 << log_n), h.buffer(nbytes=16 << log_n)
        run = lambda: h.round([a.ptr.value, b.ptr.value], terms, log_n, LOW, 3, 5, [fa.ptr.value, fb.ptr.value])
        assert run()[0] == 0  # whatever the runtime keeps from a kernel's first launch is there before the baseline is read
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        before = free_bytes(h.lib)
        rc, e1 = run()
        assert rc == 0
        first = free_bytes(h.lib)
        rc, e2 = run()
        assert rc == 0 and free_bytes(h.lib) == first, "a repeated identical call allocated"
        assert np.array_equal(e1, e2)
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        assert free_bytes(h.lib) == before, "panda_ntt_tear_down releases the scratch"
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order,fused", [(LOW, True), (HIGH, False)])
def test_gpu_manager_helper(gm, order, fused):
    k, cols, challenges = _sumcheck_instance()
    words = [np.array(fr.wire(0, c)) for c in cols]
    keep = [w.copy() for w in words]
    wire_terms = [(fr.wire(0, [c])[0], fs) for c, fs in GATE_EQ]
    evals, finals = pgm.panda_sumcheck_gpu_run(gm, words, wire_terms, 5, fr.wire(0, challenges), order=order, fused=fused)
    assert evals.shape == (k, 5, 8) and finals.shape == (9, 8) and evals.dtype == np.uint32
    _verify_sumcheck(0, cols, GATE_EQ, [fr.plain(0, e) for e in evals], fr.plain(0, finals), challenges, order)
    assert all(np.array_equal(w, q) for w, q in zip(words, keep)), "the helper changed its input"
    with pytest.raises(pgm.PandaGpuError):
        pgm.panda_sumcheck_gpu_run(gm, [], wire_terms, 5, fr.wire(0, challenges))
    with pytest.raises(pgm.PandaGpuError):
        pgm.panda_sumcheck_gpu_run(gm, words, wire_terms, 5, fr.wire(0, challenges[:-1]))
