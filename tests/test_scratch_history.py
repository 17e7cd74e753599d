"""Results must not depend on what the scratch held before.  Every entry point but the plain NTT carves its temporaries from one grow-only
arena per host thread, never cleared and carved from offset 0 again by every call, so a call runs on the bytes the call before it left: a
counter, a histogram cell, a list head or a flag that no kernel writes before another kernel reads it would meet zeros on fresh memory and
the right value after an identical call, and the suite would not notice.  Here every feature's call runs on scratch filled with zeros, with
all-ones and with a hash (panda_debug_scratch_fill: the whole arena and the pinned mailbox), and behind calls of the same feature on other
inputs, on a shape twice as large, or of another feature -- and must still give the reference's answer, byte for byte the same one where
the header documents the output as deterministic or canonical.  The protocol is gpu_util.independent_of_scratch.

No references of its own: the harnesses, shapes and expected-value helpers are the feature modules' (Python integers or the CPU oracle,
never the device).  DESIGN.md ("what every scratch block holds when it is first read") lists the writer of every block."""
import contextlib
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import field_ref as fr
import oracle as po
import points_ref as pr
import pyref
import test_ec_ntt as t_ec
import test_kzg_open_all as t_kzg
import test_lookup as t_lk
import test_msm_batch as t_mb
import test_ntt_lde as t_lde
import test_points_mul as t_pm
import test_points_to_affine as t_pa
import test_poly_open as t_po
import test_poly_product as t_pp
import test_poly_sum_of_products as t_sop
import test_sparse as t_sp
import test_sumcheck as t_sc
from gpu_util import (SCRATCH_PATTERNS, assert_exported, free_bytes, gm, has_gpu, independent_of_scratch, same_bytes, scratch_fill,  # noqa: F401
                      scratch_hash, scratch_pattern_bytes)
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm
from test_gpu_parity import _built_in_policies, _edge_scalars  # noqa: F401  (the fixture: every test starts and ends on the built-in policies)

gpu = pytest.mark.gpu
FIELD_NAME = ("bn254", "bls12_377", "bls12_381")


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbol_in_header_ffi_and_library():
    header, lib = assert_exported(["panda_debug_scratch_fill"])
    assert lib.panda_debug_scratch_fill.argtypes[2:] == [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    assert "0x7FEB352D" in header and "0x846CA68B" in header, "the header documents the hash"


def test_a_bad_mode_is_refused_and_writes_nothing():
    lib = ffi.load()
    for mode in (2, 3, 0xFFFFFFFF):
        base, capacity = C.c_void_p(0xDEAD), C.c_size_t(0xBEEF)
        assert lib.panda_debug_scratch_fill(mode, 0, C.byref(base), C.byref(capacity)) == 1
        assert (base.value, capacity.value) == (0xDEAD, 0xBEEF)
        assert lib.panda_debug_scratch_fill(mode, 0, None, None) == 1


def test_without_an_arena_the_fill_reports_none_and_allocates_nothing():
    """a host thread that has made no call has neither an arena nor a mailbox: success, (NULL, 0), either pointer may be NULL, and -- where
    there is a device -- not a byte of device memory taken"""
    lib, seen = ffi.load(), []

    def fresh_thread():
        before = free_bytes(lib) if has_gpu() else None
        for mode, value in SCRATCH_PATTERNS:
            seen.append(scratch_fill(mode, value))
            base, capacity = C.c_void_p(0xDEAD), C.c_size_t(0xBEEF)
            seen.append((lib.panda_debug_scratch_fill(mode, value, C.byref(base), None), base.value))
            seen.append((lib.panda_debug_scratch_fill(mode, value, None, C.byref(capacity)), capacity.value))
            seen.append((lib.panda_debug_scratch_fill(mode, value, None, None), None))
        seen.append(before == (free_bytes(lib) if has_gpu() else None))

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert seen == [(None, 0), (0, None), (0, 0), (0, None)] * len(SCRATCH_PATTERNS) + [True]


def test_the_python_copy_of_the_hash_is_pinned():
    """three recorded words of h(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16"""
    assert scratch_hash(0) == 0
    assert (scratch_hash(1), scratch_hash(0x5CA7C4ED), scratch_hash(0xFFFFFFFF)) == (0x688990C0, 0x941B9B07, 0x6768824A)  # from a C program of those five steps
    assert len({scratch_hash(x) for x in range(4096)}) == 4096, "a bijection has no collisions"
    assert scratch_pattern_bytes(1, 5, 3, 2).view(np.uint32).tolist() == [scratch_hash(3 ^ 5), scratch_hash(4 ^ 5)]
    assert scratch_pattern_bytes(0, 0x1FF, 0, 1).tolist() == [0xFF] * 4


# ------------------------------------------------------------------------------------------------- the fill itself
def _arena_bytes(base, offset, nbytes):
    out = np.empty(nbytes, np.uint8)
    ffi.check(ffi.load().panda_memcpy(C.c_void_p(out.ctypes.data), C.c_void_p(base + offset), nbytes), "memcpy")
    return out


@gpu
def test_the_fill_covers_the_whole_capacity(gm):
    """behind a call that has grown the arena: the first words, words in the middle and the last bytes hold the pattern, the capacity is
    at least what the call's plan says it takes, and no fill moves or grows the arena"""
    with _lookup(gm, 0, 64, 100, 0x10) as (call, check, _):
        check(call())
        lib = ffi.load()
        log_slots, scratch = C.c_uint(0), C.c_size_t(0)
        assert lib.panda_lookup_plan(64, 2, 100, C.byref(log_slots), C.byref(scratch), None) == 0
        where = None
        for mode, value in SCRATCH_PATTERNS:
            base, capacity = scratch_fill(mode, value)
            assert base and capacity >= scratch.value and (where is None or where == (base, capacity))
            where = (base, capacity)
            words = capacity // 4
            for first, count in ((0, 64), (words // 2 - 3, 61), (words - 40, 40)):
                assert np.array_equal(_arena_bytes(base, 4 * first, 4 * count), scratch_pattern_bytes(mode, value, first, count)), (mode, value, first)
            tail = capacity - 4 * words
            assert tail == 0 or (_arena_bytes(base, 4 * words, tail) == (value & 0xFF)).all()
        check(call())


# ------------------------------------------------------------------------------------------------- verdicts are remembered by content
def _checked_once(verify):
    """check(out): verify(out), unless an output with the same bytes has passed before -- the reference's verdict on equal bytes is the
    same, and the larger shapes' references take longer than the calls"""
    passed = []

    def check(out):
        if not any(same_bytes(out, p) for p in passed):
            verify(out)
            passed.append(out)
    return check


# ------------------------------------------------------------------------------------------------- the scalar-field families
# Each family is a context manager over (gm, field, shape..., seed) that yields (call, check, exact): call() runs the feature on fresh
# guarded buffers through its module's harness and returns the output, check(output) compares it with the module's reference.

def _eval_by_oracle(field, polys, z_wire):
    """f(z) of every polynomial of (batch, n, 8) through the oracle's vector operations: the powers of z by doubling, the products, a
    halving sum -> (batch, 8)"""
    fid, n = po.FR_OF[field], polys.shape[1]
    pw = np.ascontiguousarray(fr.wire_one(field, 1).reshape(1, 8))
    step = np.ascontiguousarray(np.asarray(z_wire, np.uint32).reshape(1, 8))
    while len(pw) < n:  # pw = z^0 .. z^(m-1), step = z^m
        pw = np.concatenate([pw, po.f_vec(fid, po.OP_MUL, pw, np.ascontiguousarray(np.broadcast_to(step, pw.shape)))])
        step = po.f_vec(fid, po.OP_MUL, step, step)
    pw = np.ascontiguousarray(pw[:n])
    out = []
    for coeffs in polys:
        acc = po.f_vec(fid, po.OP_MUL, np.ascontiguousarray(coeffs), pw)
        while len(acc) > 1:
            if len(acc) & 1:
                acc = np.concatenate([acc, np.zeros((1, 8), np.uint32)])
            half = len(acc) // 2
            acc = po.f_vec(fid, po.OP_ADD, np.ascontiguousarray(acc[:half]), np.ascontiguousarray(acc[half:]))
        out.append(acc[0])
    return np.stack(out)


@contextlib.contextmanager
def _poly_divide(gm, field, n, batch, seed):
    coeffs, (z_wire, z_plain) = t_po._coeffs(field, n, batch, seed), t_po._point(field, seed & 0xFF)
    want = [t_po._horner(field, coeffs[p], z_plain) for p in range(batch)] if n <= 1 << 14 else None
    h = t_po.Harness(gm, field, n, batch)

    def verify(out):
        q, rem = out
        for p in range(batch):
            if want is not None:
                assert np.array_equal(q[p], want[p][0]) and np.array_equal(rem[p], want[p][1]), (field, n, p)
            else:
                assert t_po._is_quotient(field, coeffs[p], z_wire, q[p], rem[p]), (field, n, p)
    try:
        yield (lambda: h.divide(coeffs, z_wire)), _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _poly_evaluate(gm, field, n, batch, seed):
    coeffs, (wires, plains) = t_po._coeffs(field, n, batch, seed), t_po._eval_points(field)
    if n <= 1 << 14:
        want = np.stack([np.stack([t_po._horner(field, coeffs[p], z)[1] for z in plains]) for p in range(batch)])
    else:
        want = np.stack([_eval_by_oracle(field, coeffs, w) for w in wires], axis=1)
    h = t_po.Harness(gm, field, n, batch)

    def verify(vals):
        assert np.array_equal(vals, want), (field, n)
    try:
        yield (lambda: h.evaluate(coeffs, wires)), _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _batch_inverse(gm, field, n, seed, zero_at=()):
    x = np.array(t_pp._vectors(field, n, 1, seed))
    for i in zero_at:
        x[0, i] = 0
    want = t_pp._inverse_expected(field, x[0]) if n <= 1 << 14 else None
    h = t_pp.Harness(gm, field, n)

    def verify(out):
        assert np.array_equal(out[0], want) if want is not None else t_pp._is_inverse(field, x[0], out[0]), (field, n)
    try:
        yield (lambda: h.inverse(x)), _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _grand_product(gm, field, n, batch, seed, zero_den=None):
    """zero_den = (vector, index): that vector has a zero denominator, and its output and total are all zero"""
    num, den = t_pp._vectors(field, n, batch, seed), np.array(t_pp._vectors(field, n, batch, seed + 1))
    if zero_den is not None:
        den[zero_den] = 0
    want = [t_pp._product_expected(field, num[p], den[p]) for p in range(batch)] if n <= 1 << 14 else None
    h = t_pp.Harness(gm, field, n, batch)

    def verify(out):
        z, tot = out
        for p in range(batch):
            if zero_den is not None and p == zero_den[0]:
                assert not z[p].any() and not tot[p].any(), (field, n, p, "a zero denominator")
            elif want is not None:
                assert np.array_equal(z[p], want[p][0]) and np.array_equal(tot[p], want[p][1]), (field, n, p)
            else:
                assert t_pp._is_product(field, num[p], den[p], z[p], tot[p]), (field, n, p)
    try:
        yield (lambda: h.product(num, den)), _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _running_sum(gm, field, n, batch, seed, where="o"):
    x = t_lk._vectors(field, n, batch, seed)
    want = [t_lk._sum_expected(field, x[p]) for p in range(batch)]
    want_out, want_tot = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    h = t_lk.Sums(gm, field, n, batch)

    def verify(out):
        sums, tot = out
        assert np.array_equal(tot, want_tot) and (sums is None) == (where is None) and (sums is None or np.array_equal(sums, want_out)), (field, n, where)
    try:
        yield (lambda: h.run(x, where=where)), _checked_once(verify), True
    finally:
        h.close()


# the gate of test_poly_sum_of_products.py with its b wire read one row ahead and its c wire one row behind
GATE_ROTATED = [(1, [(0, 0), (5, 0)]), (1, [(1, 0), (6, 1)]), (1, [(2, 0), (5, 0), (6, 1)]), (1, [(3, 0), (7, -1)]), (1, [(4, 0)])]


@contextlib.contextmanager
def _sum_of_products(gm, field, n, batch, seed):
    cols = t_sop._gate_columns(field, seed, batch, n)
    words, want = [t_sop._col_words(field, c) for c in cols], t_sop._expected(field, cols, GATE_ROTATED)
    h = t_sop.Harness(gm, field, n, batch)

    def verify(out):
        assert np.array_equal(out, want), (field, n, batch)
    try:
        yield (lambda: h.run(words, GATE_ROTATED)), _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _lookup(gm, field, n_table, n, seed, missing=1):
    """a table with duplicate rows, two columns drawn from it, `missing` values that are not in it"""
    pool, rng = t_lk._pool(field, 4096, 0x10061 + field), np.random.default_rng(seed)
    table = np.array(pool[rng.choice(2048, n_table, replace=False)])
    table[n_table // 2] = table[n_table // 3 + 1] = table[3 % n_table]
    cols = [np.array(table[rng.integers(0, n_table, n)]) for _ in range(2)]
    for k in range(missing):
        cols[1 - k % 2][(7 + 13 * k) % n] = pool[3000 + k]
    want = t_lk._lookup_expected(field, table, cols)
    assert want[1] == missing
    h = t_lk.Lookup(gm, field, n_table, n, 2)

    def verify(out):
        mult, lost, first = out
        assert np.array_equal(mult, want[0]) and (lost, first) == want[1:], (field, n_table, n, lost, first)
    try:
        yield (lambda: h.run(table, cols)), _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _sumcheck_round(gm, field, log_n, order, fused, seed):
    """gate times eq, five points; fused: the round over the tables folded with a challenge, and the folded tables themselves"""
    n, n_evals = 1 << log_n, 5
    cols = [fr.random_residues(field, seed + k, n) for k in range(9)]
    challenge = fr.random_residues(field, seed + 100, 1)[0] if fused else None
    folded = [t_sc._fold(field, c, challenge, order) for c in cols] if fused else None
    want = fr.wire(field, t_sc._round(field, folded if fused else cols, t_sc.GATE_EQ, n_evals, order))
    want_folded = [fr.wire(field, f) for f in folded] if fused else []
    h = t_sc.Dev(gm, field)
    ds = [h.buffer(fr.wire(field, c)) for c in cols]
    fs = [h.buffer(nbytes=n * 16) for _ in cols] if fused else []

    def call():
        for f in fs:
            h.fill(f)
        rc, evals = h.round([d.ptr.value for d in ds], t_sc.GATE_EQ, log_n, order, n_evals, challenge, [f.ptr.value for f in fs] if fused else None)
        assert rc == 0 and all(h.intact(d) for d in ds) and all(h.guard_intact(f) for f in fs)
        return [evals] + [h.rows(f) for f in fs]

    def verify(out):
        assert np.array_equal(out[0], want), (field, log_n, order, fused)
        assert all(np.array_equal(a, b) for a, b in zip(out[1:], want_folded)), (field, log_n, order, "folded")
    try:
        yield call, _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _mle_fold(gm, field, log_n, order, seed):
    n = 1 << log_n
    cols = [fr.random_residues(field, seed + k, n) for k in range(3)]
    challenge = fr.random_residues(field, seed + 100, 1)[0]
    want = [fr.wire(field, t_sc._fold(field, c, challenge, order)) for c in cols]
    h = t_sc.Dev(gm, field)
    ds, fs = [h.buffer(fr.wire(field, c)) for c in cols], [h.buffer(nbytes=n * 16) for _ in cols]

    def call():
        for f in fs:
            h.fill(f)
        assert h.fold([d.ptr.value for d in ds], [f.ptr.value for f in fs], log_n, order, challenge) == 0
        assert all(h.intact(d) for d in ds) and all(h.guard_intact(f) for f in fs)
        return [h.rows(f) for f in fs]

    def verify(out):
        assert all(np.array_equal(a, b) for a, b in zip(out, want)), (field, log_n, order)
    try:
        yield call, _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _eq_table(gm, field, log_n, seed):
    point = fr.random_residues(field, seed, log_n)
    pt, want = fr.wire(field, point), fr.wire(field, t_sc._eq(field, point))
    h = t_sc.Dev(gm, field)
    out = h.buffer(nbytes=32 << log_n)

    def call():
        h.fill(out)
        assert h.lib.panda_mle_eq_table(field, C.c_void_p(pt.ctypes.data), log_n, out.ptr, h.stream) == 0 and h.guard_intact(out)
        return h.rows(out)

    def verify(got):
        assert np.array_equal(got, want), (field, log_n)
    try:
        yield call, _checked_once(verify), True
    finally:
        h.close()


def _sparse_lengths(scale=1):
    """a row that crosses the first tile's end, a run of empty rows across the second tile's end, a row of a whole tile, rows behind it"""
    T = t_sp._tile()[0]
    return ([T - 3, 7, T - 9] + [0] * 5 + [2, 5] + [0] * 4 + [T, 3, 1]) * scale


@contextlib.contextmanager
def _sparse_matvec(gm, field, lengths, seed):
    n_cols = 61
    row_ptr, col, vals, z = t_sp._random_matrix(seed, lengths, n_cols, field)
    z2 = fr.random_residues(field, seed + 7, n_cols)
    want = np.stack([fr.wire(field, t_sp._product(field, row_ptr, col, vals, v)) for v in (z, z2)])
    h = t_sp.Dev(gm, field)
    m, bufs = h.matrix(row_ptr, col, fr.wire(field, vals), n_cols)
    zb, out = h.buffer(np.concatenate([fr.wire(field, z), fr.wire(field, z2)])), h.buffer(nbytes=2 * (len(row_ptr) - 1) * 32)

    def call():
        h.fill(out)
        assert h.check(m) == (0, t_sp.NO_INDEX) and h.matvec(m, zb, out, 2) == 0
        assert all(h.intact(d) for d in bufs + (zb,)) and h.guard_intact(out)
        return h.get(out).reshape(2, -1, 8)

    def verify(got):
        assert np.array_equal(got, want), (field, len(col))
    try:
        yield call, _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _sparse_check_defective(gm, field, lengths, seed):
    """a column index out of range in the second tile and a later one in the third: defect class 4 at the first of them"""
    T = t_sp._tile()[0]
    row_ptr, col, vals, _ = t_sp._random_matrix(seed, lengths, 61, field)
    col = col.copy()
    col[[T + 17, 2 * T + 5]] = 61
    h = t_sp.Dev(gm, field)
    m, bufs = h.matrix(row_ptr, col, fr.wire(field, vals), 61)

    def verify(got):
        assert got == (4, T + 17), got
    try:
        yield (lambda: h.check(m)), verify, True
    finally:
        h.close()


@functools.lru_cache(maxsize=None)
def _coset_reference(field, log_n, seed):
    """(x, the oracle's coset transform of x): element j times g^j, then the transform"""
    fid, n = po.FR_OF[field], 1 << log_n
    x = po.gen_scalars(fid, seed, n).reshape(n, 8)
    y = po.ntt(fid, po.f_vec(fid, po.OP_MUL, x, fr.shift_powers(field, n, t_lde.SHIFT)), po.root_of_unity(fid, log_n), log_n)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@contextlib.contextmanager
def _coset_ntt(gm, field, log_n, inverse, seed):
    x, y = _coset_reference(field, log_n, seed)
    src, want = (y, x) if inverse else (x, y)
    omega, g = po.root_of_unity(po.FR_OF[field], log_n), fr.wire_one(field, t_lde.SHIFT)

    def call():
        buf = np.array(src).reshape(-1)
        if field == 0:
            pgm.panda_coset_ntt_bn254_gpu(gm, buf, omega, g, log_n, inverse=inverse)
        else:
            pgm.panda_coset_ntt_bls12_377_gpu(gm, buf, omega, g, log_n, inverse=inverse, field=FIELD_NAME[field])
        return buf.reshape(-1, 8)

    def verify(got):
        assert np.array_equal(got, want), (field, log_n, inverse)
    yield call, _checked_once(verify), True


@contextlib.contextmanager
def _lde(gm, field, log_n, log_blowup, batch, order, seed):
    coeffs, natural = t_lde._coeffs(field, log_n, batch, seed), t_lde._oracle_natural(field, log_n, log_blowup, batch, seed)
    want = natural if order == ffi.NTT_LDE_NATURAL else t_lde._to_coset_major(natural, log_n, log_blowup)
    h = t_lde.Harness(gm, field, log_n, log_blowup, batch)

    def verify(got):
        assert np.array_equal(got, want), (field, log_n, log_blowup, batch, order)
    try:
        yield (lambda: h.lde(coeffs, order)), _checked_once(verify), True
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------- the G1 vector families
@functools.lru_cache(maxsize=None)
def _ec_ntt_reference(curve, log_n, inverse, shift):
    """(input words, expected words): P_j = (a + (j + shift) d) G by repeated additions, out[k] = (sum_j s_j omega^(jk)) G"""
    n = 1 << log_n
    a, d = fr.random_residues(curve, 0xAF00 + curve, 2)  # test_points_to_affine._points' progression
    pts = t_pa._points(curve, n + shift)[shift:]
    r = pyref.CURVES[curve].r
    want = pr.enc_multiples(curve, t_ec._dft(curve, [(a + (j + shift) * d) % r for j in range(n)], log_n, inverse))
    return pr.enc_all(curve, pts), want


@contextlib.contextmanager
def _ec_ntt(gm, curve, log_n, inverse, shift=0):
    words, want = _ec_ntt_reference(curve, log_n, inverse, shift)
    h = pr.Dev(gm, curve)
    src, dst = h.buffer(words), h.buffer(nbytes=len(words) * pr.point_bytes(curve))
    om = np.ascontiguousarray(t_ec._omega_wire(curve, log_n))

    def call():
        h.fill(dst)
        rc = h.lib.panda_ec_ntt(curve, src.ptr, dst.ptr, log_n, ffi.EC_NTT_INVERSE if inverse else ffi.EC_NTT_FORWARD, C.c_void_p(om.ctypes.data), h.stream)
        assert rc == 0 and h.intact(src) and h.guard_intact(dst)
        return h.get(dst).reshape(len(words), -1)

    def verify(got):
        pr.compare(got, want, (curve, log_n, inverse))
    try:
        yield call, _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _points_to_affine(gm, curve, n, homogeneous, seed):
    pts = list(t_pa._points(curve, n))
    pts[n // 2] = None  # an identity: Z == 0 beside nonzero X and Y
    triples, want = t_pa._triples(curve, pts, homogeneous, seed), pr.enc_all(curve, pts)
    h = pr.Dev(gm, curve)
    src, dst = h.buffer(triples), h.buffer(nbytes=n * pr.point_bytes(curve))

    def call():
        h.fill(dst)
        rc = h.lib.panda_points_to_affine(curve, src.ptr, ffi.PROJECTIVE if homogeneous else ffi.JACOBIAN, dst.ptr, n, h.stream)
        assert rc == 0 and h.intact(src) and h.guard_intact(dst)
        return h.get(dst).reshape(n, -1)

    def verify(got):
        pr.compare(got, want, (curve, n, homogeneous))
    try:
        yield call, _checked_once(verify), True
    finally:
        h.close()


@contextlib.contextmanager
def _points_mul(gm, curve, mode, n, first=0):
    """out[i] = (b_i + k_i a_i) G over the fixture of test_points_mul.py, points [first, first + n) of it"""
    f = t_pm._fixture(curve)
    ks = f.scalars(mode)
    # POWERS counts its exponent from the call's first point: only first == 0 keeps the fixture's scalars for that mode
    assert mode != t_pm.POWERS or first == 0
    want = pr.enc_multiples(curve, [f.b[i] + ks[i] * f.a[i] for i in range(first, first + n)])
    d_sc, h_sc = t_pm._mode_scalars(curve, mode, ks=f.k, one=f.one, c=f.c, s=f.s)

    def call():
        return t_pm._run(gm, curve, mode, f.P[first:], None if d_sc is None else d_sc[first:], h_sc, f.A[first:], n, (curve, mode, n))

    def verify(got):
        pr.compare(got, want, (curve, mode, n, first))
    yield call, _checked_once(verify), True


@contextlib.contextmanager
def _kzg_open_all(gm, curve, log_n, seed, work_pattern=None):
    """work_pattern: the (mode, value) the caller's d_work holds before every open, the guard byte without one"""
    n, pb, r = 1 << log_n, pr.point_bytes(curve), pyref.CURVES[curve].r
    tau, = fr.random_residues(curve, seed, 1)
    f = fr.random_residues(curve, seed + 1, n)
    want = pr.enc_multiples(curve, t_kzg._reference(curve, f, tau, log_n))
    lib, om = ffi.load(), t_kzg._omega2_wire(curve, log_n)
    rc, work_bytes, _ = t_kzg._plan(lib, curve, log_n)
    assert rc == 0 and work_bytes % 4 == 0
    h = pr.Dev(gm, curve)
    srs = h.buffer(pr.enc_multiples(curve, [pow(tau, i, r) for i in range(n)]))
    table, work, proofs = h.buffer(nbytes=2 * n * pb), h.buffer(nbytes=work_bytes), h.buffer(nbytes=n * pb)
    coeffs = h.buffer(fr.wire(curve, f))
    assert lib.panda_kzg_open_all_setup(curve, srs.ptr, log_n, pr.host_ptr(om), table.ptr, h.stream) == 0
    table.host = h.get(table)
    state = {"work": work_pattern}

    def call():
        h.fill(proofs)
        h.fill(work)
        if state["work"] is not None:
            junk = scratch_pattern_bytes(*state["work"], 0, work_bytes // 4)
            ffi.check(lib.panda_memcpy(work.ptr, C.c_void_p(junk.ctypes.data), work_bytes), "memcpy")
        assert lib.panda_kzg_open_all(curve, coeffs.ptr, table.ptr, log_n, pr.host_ptr(om), work.ptr, work_bytes, proofs.ptr, h.stream) == 0
        assert h.intact(coeffs) and h.intact(table) and h.intact(srs) and h.guard_intact(work) and h.guard_intact(proofs)
        return h.get(proofs).reshape(n, -1)

    def verify(got):
        pr.compare(got, want, (curve, log_n))
    try:
        yield call, _checked_once(verify), True, state
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------- the MSMs
# The Jacobian representative of a result follows the order of atomics, so an MSM is compared as an affine point with the oracle's
# linearity value (test_msm_batch._decode / _expected), never byte for byte.

@contextlib.contextmanager
def _msm(gm, curve, k, seed, tables=None, window_bits=0, plain_bits=0, scalars=None, batch=1, entry="single"):
    """tables: None plain, False registered (converted rows only), True window tables of `window_bits` (0: the policy's); plain_bits:
    panda_msm_set_window_bits for the call.  entry: "single" the curve's execute, "batch" panda_msm_execute_batch over `batch` members,
    ("ranges", R) R equal point ranges inside one call, ("upload", chunks) the upload pipeline from pageable host scalars."""
    b = t_mb.Batch(gm, curve, k, batch, seed, tables=tables, window_bits=window_bits)
    lib = b.lib
    try:
        if scalars is not None:
            for j in range(batch):
                b.set_member(j, scalars)
        want = [b.expected(j) for j in range(batch)]
        if entry == "batch":
            assert b.group_log()[0] >= 1, "the batch is not fused at this shape"
        host = np.ascontiguousarray(b.scalars[0])

        def call():
            ffi.check(lib.panda_msm_set_window_bits(plain_bits), "window_bits")
            try:
                ffi.check(lib.panda_memset(b.dr1.ptr, 0xA5, b.res), "memset")  # no call may pass on the result of the call before
                if entry == "single":
                    return [b.single(0)]
                if entry == "batch":
                    return b.run()[0]
                if entry[0] == "ranges":
                    ffi.check(lib.panda_msm_execute_from_host(curve, b.cfg(b.dr1.ptr), None, 0x100 | entry[1], gm.exec_stream.raw), "ranges")
                else:
                    ffi.check(lib.panda_memset(b.ds.ptr, 0xEE, b.n * 32), "memset")  # the device buffer holds nothing useful before the call
                    ffi.check(lib.panda_msm_execute_from_host(curve, b.cfg(b.dr1.ptr), C.c_void_p(host.ctypes.data), entry[1], gm.h2d_stream.raw), "upload")
                    assert np.array_equal(b.ds.to_host().reshape(b.n, 8), host), "the whole scalar set arrived on the device"
                return [t_mb._decode(curve, b.dr1.to_host(np.uint8))]
            finally:
                lib.panda_msm_set_window_bits(0)

        def check(got):
            assert got == want, (curve, k, tables, window_bits, plain_bits, entry)
        yield call, check, False
    finally:
        b.close()


def _fill_case(family, *args, arena=True, **kw):
    with family(*args, **kw) as made:
        call, check, exact = made[:3]
        independent_of_scratch(call, check, exact, arena=arena)


# ------------------------------------------------------------------------------------------------- filled scratch: the MSMs
@gpu
@pytest.mark.parametrize("curve", t_mb.CURVES)
def test_msm_plain_on_filled_scratch(gm, curve):
    _fill_case(_msm, gm, curve, 10, 0x5C00 + curve)


@gpu
@pytest.mark.parametrize("window_bits", [0, 13])
def test_msm_tabled_on_filled_scratch(gm, window_bits):
    _fill_case(_msm, gm, 0, 12, 0x5C10 + window_bits, tables=True, window_bits=window_bits)


@gpu
def test_msm_three_level_sort_on_filled_scratch(gm):
    """the plain path with 17-bit windows: u32 digit codes and the three-level sort with a bucket space per window"""
    lib, bits = ffi.load(), C.c_uint(0)
    ffi.check(lib.panda_msm_set_window_bits(17), "window_bits")
    assert lib.panda_msm_plain_window_plan(0, 14, C.byref(bits), None) == 0 and bits.value == 17, "2^14 points take no 17-bit windows"
    _fill_case(_msm, gm, 0, 14, 0x5C20, plain_bits=17)


@gpu
def test_msm_point_ranges_on_filled_scratch(gm):
    _fill_case(_msm, gm, 0, 17, 0x5C30, tables=True, entry=("ranges", 4))


@gpu
def test_msm_upload_pipeline_on_filled_scratch(gm):
    _fill_case(_msm, gm, 0, 17, 0x5C40, tables=True, entry=("upload", 2))


@gpu
def test_msm_registered_bases_on_filled_scratch(gm):
    _fill_case(_msm, gm, 0, 10, 0x5C50, tables=False)


@gpu
@pytest.mark.parametrize("curve", [0, 4])
def test_msm_fused_batch_on_filled_scratch(gm, curve):
    _fill_case(_msm, gm, curve, 10, 0x5C60 + curve, tables=True, batch=4, entry="batch")


@gpu
@pytest.mark.parametrize("kind", ["all_equal", "zeros"])
def test_msm_tabled_edge_scalars_on_filled_scratch(gm, kind):
    """one bucket per window; no bucket at all: where a counter that nothing writes would be read"""
    _fill_case(_msm, gm, 0, 12, 0x5C70, tables=True, window_bits=14, scalars=_edge_scalars(kind, 1 << 12))


# ------------------------------------------------------------------------------------------------- filled scratch: the scalar fields
def _poly_sizes():
    tile, chunk = t_po._shape()
    return tile + 1, tile * chunk + 1


def _product_sizes():
    ti, tp, chunk = t_pp._shape()
    assert ti == tp
    return ti + 1, ti * chunk + 1


@gpu
@pytest.mark.parametrize("field,which", [(0, 0), (0, 1), (2, 0)])
@pytest.mark.parametrize("family", ["evaluate", "divide"])
def test_poly_open_on_filled_scratch(gm, family, field, which):
    _fill_case(_poly_evaluate if family == "evaluate" else _poly_divide, gm, field, _poly_sizes()[which], 2, 0x5D00 + 16 * field + which)


@gpu
@pytest.mark.parametrize("field,which", [(0, 0), (0, 1), (2, 0)])
def test_batch_inverse_on_filled_scratch(gm, field, which):
    n = _product_sizes()[which]
    _fill_case(_batch_inverse, gm, field, n, 0x5D40 + 16 * field + which, zero_at=(n // 3, n - 1) if which else ())


@gpu
@pytest.mark.parametrize("field,which", [(0, 0), (0, 1), (2, 0)])
def test_grand_product_on_filled_scratch(gm, field, which):
    n = _product_sizes()[which]
    _fill_case(_grand_product, gm, field, n, 2, 0x5D80 + 16 * field + which, zero_den=None if which else (1, n // 2))


@gpu
@pytest.mark.parametrize("field,where", [(0, "o"), (0, None), (2, "o")])
def test_running_sum_on_filled_scratch(gm, field, where):
    _fill_case(_running_sum, gm, field, t_lk._shape()[0] + 1, 2, 0x5DC0 + field, where=where)


@gpu
@pytest.mark.parametrize("field", [0, 2])
def test_sum_of_products_on_filled_scratch(gm, field):
    _fill_case(_sum_of_products, gm, field, 1000, 1, 0x5E00 + field)


@gpu
@pytest.mark.parametrize("field", [0, 2])
def test_lookup_on_filled_scratch(gm, field):
    _fill_case(_lookup, gm, field, 64, 1000, 0x5E40 + field)


@gpu
@pytest.mark.parametrize("field,order,fused", [(0, t_sc.LOW, False), (0, t_sc.HIGH, False), (0, t_sc.LOW, True), (0, t_sc.HIGH, True), (2, t_sc.HIGH, True)])
def test_sumcheck_round_on_filled_scratch(gm, field, order, fused):
    _fill_case(_sumcheck_round, gm, field, 11, order, fused, 0x5E80 + 16 * field)


@gpu
def test_mle_fold_and_eq_table_on_filled_scratch(gm):
    for order in (t_sc.LOW, t_sc.HIGH):
        _fill_case(_mle_fold, gm, 0, 11, order, 0x5EC0, arena=False)  # the fold takes no scratch
    _fill_case(_eq_table, gm, 0, 12, 0x5ED0)
    _fill_case(_eq_table, gm, 2, 12, 0x5ED2)


@gpu
@pytest.mark.parametrize("field", [0, 2])
def test_sparse_on_filled_scratch(gm, field):
    _fill_case(_sparse_matvec, gm, field, _sparse_lengths(), 0x5F00 + field)
    _fill_case(_sparse_check_defective, gm, field, _sparse_lengths(), 0x5F10 + field)


@gpu
@pytest.mark.parametrize("field,log_n", [(0, 10), (0, 17), (2, 10)])
@pytest.mark.parametrize("inverse", [False, True])
def test_coset_ntt_on_filled_scratch(gm, inverse, field, log_n):
    """2^17: the second power table of the coset sweep"""
    _fill_case(_coset_ntt, gm, field, log_n, inverse, 0x5F40 + log_n)


@gpu
@pytest.mark.parametrize("field", [0, 2])
def test_lde_on_filled_scratch(gm, field):
    _fill_case(_lde, gm, field, 8, 2, 3, ffi.NTT_LDE_NATURAL, 0x5F80 + field, arena=False)  # its tables live in the twiddle cache


# ------------------------------------------------------------------------------------------------- filled scratch: the G1 vectors
@gpu
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("curve", pr.CURVES)
def test_ec_ntt_on_filled_scratch(gm, curve, inverse):
    _fill_case(_ec_ntt, gm, curve, 7, inverse)


@gpu
@pytest.mark.parametrize("curve", pr.CURVES)
def test_points_to_affine_on_filled_scratch(gm, curve):
    _fill_case(_points_to_affine, gm, curve, t_pa._chunk() + 1, False, 0x6000 + curve, arena=False)  # one launch, no scratch


@gpu
@pytest.mark.parametrize("mode", t_pm.MODES)
@pytest.mark.parametrize("curve", pr.CURVES)
def test_points_scalar_mul_on_filled_scratch(gm, curve, mode):
    _fill_case(_points_mul, gm, curve, mode, t_pm.N)


@gpu
@pytest.mark.parametrize("curve", pr.CURVES)
def test_kzg_open_all_on_filled_scratch_and_work(gm, curve):
    """the arena under the three patterns, and under each of them the caller's d_work holding the same pattern"""
    with _kzg_open_all(gm, curve, 3, 0x6040 + curve) as (call, check, exact, state):
        first = independent_of_scratch(call, check, exact)
        for pattern in SCRATCH_PATTERNS:
            state["work"] = pattern
            where = scratch_fill(*pattern)
            out = call()
            assert scratch_fill(*SCRATCH_PATTERNS[0]) == where and where[0]
            check(out)
            assert same_bytes(out, first), ("the proofs depend on what d_work or the scratch held", pattern)


# ------------------------------------------------------------------------------------------------- stale data that looks valid
def _behind_others(family, gm, args_x, args_y, args_big, **kw):
    """inputs Y behind other inputs X of the same shape, and behind a shape twice as large: Y's output is the reference's both times (and,
    where the call is exact, the same bytes)"""
    with family(gm, *args_x, **kw) as x, family(gm, *args_y, **kw) as y, family(gm, *args_big, **kw) as big:
        x[1](x[0]())
        first = y[0]()
        y[1](first)
        big[1](big[0]())
        again = y[0]()
        y[1](again)
        assert not y[2] or same_bytes(first, again), "the output depends on the call before"


@gpu
def test_poly_divide_behind_other_inputs_and_a_larger_shape(gm):
    n = _poly_sizes()[0]
    _behind_others(_poly_divide, gm, (0, n, 2, 0x6100), (0, n, 2, 0x6101), (0, 2 * n, 2, 0x6102))


@gpu
def test_poly_evaluate_behind_other_inputs_and_a_larger_shape(gm):
    n = _poly_sizes()[0]
    _behind_others(_poly_evaluate, gm, (0, n, 2, 0x6110), (0, n, 2, 0x6111), (0, 2 * n, 2, 0x6112))


@gpu
def test_batch_inverse_and_grand_product_behind_other_inputs_and_a_larger_shape(gm):
    n = _product_sizes()[0]
    _behind_others(_batch_inverse, gm, (0, n, 0x6120), (0, n, 0x6121), (0, 2 * n, 0x6122))
    _behind_others(_grand_product, gm, (0, n, 2, 0x6130), (0, n, 2, 0x6132), (0, 2 * n, 2, 0x6134))


@gpu
def test_running_sum_and_sum_of_products_behind_other_inputs_and_a_larger_shape(gm):
    n = t_lk._shape()[0] + 1
    _behind_others(_running_sum, gm, (0, n, 2, 0x6140), (0, n, 2, 0x6141), (0, 2 * n, 2, 0x6142))
    _behind_others(_sum_of_products, gm, (0, 1000, 1, 0x6150), (0, 1000, 1, 0x6160), (0, 2000, 1, 0x6170))


@gpu
def test_lookup_behind_a_table_whose_values_are_all_witnessed(gm):
    """every value found, then one missing: the miss counter and the first-miss word of the call before read `none`"""
    _behind_others(_lookup, gm, (0, 64, 1000, 0x6180), (0, 64, 1000, 0x6181), (0, 128, 2000, 0x6182))
    with _lookup(gm, 0, 64, 1000, 0x6183, missing=0) as x, _lookup(gm, 0, 64, 1000, 0x6184, missing=1) as y, _lookup(gm, 0, 64, 1000, 0x6185, missing=3) as z:
        for made in (x, y, x, z, y, x):
            made[1](made[0]())


@gpu
def test_sumcheck_round_behind_other_inputs_and_a_larger_shape(gm):
    _behind_others(_sumcheck_round, gm, (0, 11, t_sc.HIGH, True, 0x6190), (0, 11, t_sc.HIGH, True, 0x61A0), (0, 12, t_sc.HIGH, True, 0x61B0))
    _behind_others(_sumcheck_round, gm, (0, 11, t_sc.LOW, False, 0x61C0), (0, 11, t_sc.LOW, False, 0x61D0), (0, 12, t_sc.LOW, False, 0x61E0))


@gpu
def test_sparse_matvec_behind_a_defective_matrix_and_a_larger_one(gm):
    """panda_sparse_check of a defective matrix leaves its defect word in the arena; the valid matrix behind it checks clean"""
    with _sparse_check_defective(gm, 0, _sparse_lengths(), 0x6200) as bad, _sparse_matvec(gm, 0, _sparse_lengths(), 0x6210) as y, \
            _sparse_matvec(gm, 0, _sparse_lengths(2), 0x6220) as big:
        bad[1](bad[0]())
        first = y[0]()  # its own panda_sparse_check must report no defect
        y[1](first)
        big[1](big[0]())
        bad[1](bad[0]())
        again = y[0]()
        y[1](again)
        assert same_bytes(first, again)


@gpu
def test_coset_ntt_behind_other_inputs_and_a_larger_shape(gm):
    _behind_others(_coset_ntt, gm, (0, 10, False, 0x6230), (0, 10, False, 0x6231), (0, 11, False, 0x6232))
    _behind_others(_coset_ntt, gm, (0, 17, True, 0x6233), (0, 10, True, 0x6234), (0, 17, False, 0x6235))  # behind a second power table


@gpu
def test_ec_ntt_behind_other_inputs_and_a_larger_shape(gm):
    with _ec_ntt(gm, 0, 7, False, shift=1) as x, _ec_ntt(gm, 0, 7, False) as y, _ec_ntt(gm, 0, 8, True) as big:
        x[1](x[0]())
        first = y[0]()
        y[1](first)
        big[1](big[0]())
        again = y[0]()
        y[1](again)
        assert same_bytes(first, again)


@gpu
def test_points_scalar_mul_and_kzg_behind_other_calls(gm):
    """65 points behind 130 and behind the other modes; an open behind an open of other coefficients and behind one of twice the size"""
    each, one = t_pm.EACH, t_pm.ONE
    with _points_mul(gm, 0, each, 65, first=65) as x, _points_mul(gm, 0, each, 65) as y, _points_mul(gm, 0, one, t_pm.N) as big:
        x[1](x[0]())
        first = y[0]()
        y[1](first)
        big[1](big[0]())
        again = y[0]()
        y[1](again)
        assert same_bytes(first, again)
    with _kzg_open_all(gm, 0, 3, 0x6240) as x, _kzg_open_all(gm, 0, 3, 0x6250) as y, _kzg_open_all(gm, 0, 4, 0x6260) as big:
        x[1](x[0]())
        first = y[0]()
        y[1](first)
        big[1](big[0]())
        again = y[0]()
        y[1](again)
        assert same_bytes(first, again)


@gpu
@pytest.mark.parametrize("pair", ["all_equal then uniform", "uniform then zeros", "tabled then plain", "curve 4 then curve 0"])
def test_msm_behind_another_msm(gm, pair):
    n = 1 << 12
    tabled = dict(tables=True, window_bits=14)
    first, second = {
        "all_equal then uniform": ((0, 12, 0x6300, dict(tabled, scalars=_edge_scalars("all_equal", n))), (0, 12, 0x6301, tabled)),
        "uniform then zeros": ((0, 12, 0x6310, tabled), (0, 12, 0x6311, dict(tabled, scalars=_edge_scalars("zeros", n)))),
        "tabled then plain": ((0, 12, 0x6320, tabled), (0, 12, 0x6321, {})),
        "curve 4 then curve 0": ((4, 10, 0x6330, {}), (0, 10, 0x6331, {})),
    }[pair]
    with _msm(gm, *first[:3], **first[3]) as x, _msm(gm, *second[:3], **second[3]) as y:
        for made in (x, y, x, y):
            made[1](made[0]())
