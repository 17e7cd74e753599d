"""panda_sparse_matvec / panda_sparse_check / panda_sparse_plan: sparse matrix-vector products over the scalar fields.

    out[p][r] = sum_{k in row r} values[k] z[p][col[k]]        CSR: row r holds the nonzeros row_ptr[r] .. row_ptr[r + 1] - 1

Expected values are Python integers with the moduli of tests/pyref.py, computed from this definition on plain residues and put on the wire
(w = x W mod r, W = 2^256).  Outputs are canonical and field addition is exact, so every comparison is byte for byte; there is no tolerance
anywhere.  The nonzeros one workgroup covers (T) and the tiles the second launch adds per step come from the plan call.  Every device
buffer carries a guard run of a fixed byte pattern behind the data, which no call may touch; inputs must come back unchanged.  No GPU test
passes an invalid structure to the product: that is tests/host_check/sparse_host.cpp's ground."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import field_ref as fr
from gpu_util import GuardedBuffers, assert_exported, gm, run_host_check  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

CAP = 1 << 28
NAMES = ("panda_sparse_matvec", "panda_sparse_check", "panda_sparse_plan")
NO_INDEX = (1 << 64) - 1


def _plan(lib, n_rows, n_cols, nnz, batch):
    t, c, s, l = C.c_uint(0xDEAD), C.c_uint(0xDEAD), C.c_size_t(0xDEAD), C.c_uint(0xDEAD)
    rc = lib.panda_sparse_plan(n_rows, n_cols, nnz, batch, C.byref(t), C.byref(c), C.byref(s), C.byref(l))
    return rc, t.value, c.value, s.value, l.value


@functools.lru_cache(maxsize=None)
def _tile():
    rc, tile, chunk, _, _ = _plan(ffi.load(), 8, 8, 8, 1)
    assert rc == 0 and tile >= 2 and chunk >= 1
    return tile, chunk


def _row_ptr(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.uint32)


def _random_lengths(seed, nnz, longest=6):
    """row lengths 0 .. longest that add up to nnz, with an empty row at each end"""
    rng = np.random.default_rng(seed)
    lengths, have = [0], 0
    while have < nnz:
        n = min(int(rng.integers(0, longest + 1)), nnz - have)
        lengths.append(n)
        have += n
    return lengths + [0]


def _product(field, row_ptr, col, vals, z):
    """the definition, on plain residues"""
    p = fr.modulus(field)
    return [sum(vals[k] * z[col[k]] for k in range(int(row_ptr[r]), int(row_ptr[r + 1]))) % p for r in range(len(row_ptr) - 1)]


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, _ = assert_exported(NAMES)
    assert re.search(r"typedef\s+struct\s+panda_csr_matrix", header)
    assert [f[0] for f in ffi.CsrMatrix._fields_] == ["d_row_ptr", "d_col", "d_values", "n_rows", "n_cols", "nnz"]
    assert C.sizeof(ffi.CsrMatrix) == 48 and ffi.CsrMatrix.n_rows.offset == 24 and ffi.CsrMatrix.nnz.offset == 40


BAD_SHAPES = [(0, 8, 8, 1), (8, 0, 8, 1), (8, 8, 8, 0), (CAP + 1, 8, 8, 1), (8, CAP + 1, 8, 1), (8, 8, CAP + 1, 1), (1 << 20, 8, 8, 257), (8, 1 << 20, 8, 257),
              (1 << 40, 8, 8, 1), (8, 8, 1 << 40, 1), (1 << 27, 1 << 27, 8, 3)]


def test_plan():
    lib = ffi.load()
    seen = set()
    for n_rows, n_cols, nnz, batch in ((1, 1, 0, 1), (1, 1, 1, 1), (8, 8, 8, 1), (1000, 3, 5000, 7), (CAP, 1, CAP, 1), (1, CAP, 0, 1), (1 << 20, 1 << 20, 1 << 22, 256),
                                       (1, 1, CAP, CAP)):
        rc, tile, chunk, scratch, launches = _plan(lib, n_rows, n_cols, nnz, batch)
        assert rc == 0, (n_rows, n_cols, nnz, batch)
        seen.add((tile, chunk))
        assert launches == (0 if nnz == 0 else 1 if nnz <= tile else 2)
        assert scratch >= 32 * batch * -(-nnz // tile)
    assert len(seen) == 1, "tile and carry_chunk depend on none of the arguments"
    assert lib.panda_sparse_plan(8, 8, 8, 1, None, None, None, None) == 0
    for shape in BAD_SHAPES:
        rc, tile, chunk, scratch, launches = _plan(lib, *shape)
        assert rc == 1 and (tile, chunk, scratch, launches) == (0xDEAD,) * 4, shape


def test_bad_arguments_are_refused_before_any_device_call():
    """every refusal of the contract returns 1 -- also on a machine with no device.  Host memory stands in for the device buffers: nothing
    may dereference or write it."""
    lib = ffi.load()
    mem = np.full(8 << 20, 0x5A, np.uint8)  # disjoint 1 MiB ranges
    base = mem.ctypes.data
    RP, CL, VL, Z, O = (base + (k << 20) + 4096 for k in range(5))
    stream = ffi.PandaStream()
    count = [0]

    def matrix(rp=RP, cl=CL, vl=VL, n_rows=8, n_cols=8, nnz=16):
        return ffi.CsrMatrix(rp, cl, vl, n_rows, n_cols, nnz)

    def mv(field=0, m=None, z=Z, out=O, batch=1, m_null=False, **shape):
        m = matrix(**shape) if m is None else m
        count[0] += 1
        return lib.panda_sparse_matvec(field, None if m_null else C.byref(m), None if z is None else C.c_void_p(z), None if out is None else C.c_void_p(out), batch, stream)

    def chk(field=0, m=None, m_null=False, defect=True, where=True, **shape):
        m = matrix(**shape) if m is None else m
        d, w = C.c_uint(0x7777), C.c_uint64(0x7777)
        count[0] += 1
        rc = lib.panda_sparse_check(field, None if m_null else C.byref(m), C.byref(d) if defect else None, C.byref(w) if where else None, stream)
        assert d.value == 0x7777 and w.value == 0x7777, "a refused check wrote its output"
        return rc

    # field and shapes
    assert mv(field=3) == 1 and chk(field=3) == 1 and mv(field=0xFFFFFFFF) == 1
    assert mv(n_rows=0) == 1 and mv(n_cols=0) == 1 and mv(batch=0) == 1 and chk(n_rows=0) == 1 and chk(n_cols=0) == 1
    for size in ("n_rows", "n_cols", "nnz"):
        assert mv(**{size: CAP + 1}) == 1 and chk(**{size: CAP + 1}) == 1 and mv(**{size: 1 << 40}) == 1, size
    assert mv(n_rows=1 << 20, batch=257) == 1, "batch x n_rows over the cap"
    assert mv(n_cols=1 << 20, batch=257) == 1, "batch x n_cols over the cap"
    assert mv(batch=0xFFFFFFFF) == 1
    # pointers
    assert mv(m_null=True) == 1 and chk(m_null=True) == 1
    assert mv(rp=None) == 1 and chk(rp=None) == 1 and mv(z=None) == 1 and mv(out=None) == 1
    assert mv(cl=None) == 1 and mv(vl=None) == 1 and chk(cl=None) == 1 and chk(vl=None) == 1, "NULL d_col / d_values with nnz > 0"
    assert mv(rp=None, nnz=0) == 1 and chk(rp=None, nnz=0) == 1
    assert chk(defect=False, where=False) == 1, "both out pointers of the check NULL"
    assert chk(defect=False, where=False, nnz=0, cl=None, vl=None) == 1
    # d_out equal to, inside, and straddling each of the four input ranges (n_rows 8: out is 256 bytes)
    out_bytes = 8 * 32
    for name, start, size in (("row_ptr", RP, 9 * 4), ("col", CL, 16 * 4), ("values", VL, 16 * 32), ("z", Z, 8 * 32)):
        for off in (0, 4, size - 4, -4, -(out_bytes - 4), 16 if size > 16 else 8):
            assert mv(out=start + off) == 1, (name, off)
    # batch widens the ranges: with batch 2 out and z are 512 bytes
    assert mv(out=Z + 256 + 32, batch=2) == 1 and mv(out=Z - 512 + 32, batch=2) == 1 and mv(out=Z + 511, batch=2) == 1
    assert mv(out=VL + 32, nnz=16) == 1
    assert (mem == 0x5A).all(), "a refused call wrote to a buffer"
    assert count[0] > 60


def test_host_program_checks_the_bounds_and_the_accesses(tmp_path):
    """tests/host_check/sparse_host.cpp: the row search, the per-thread routine, the tile and the fix-up of sparse.h on the host under
    FE29_CHECK against 256-bit arithmetic of its own, for the three fields: every value and z p - 1, rows of length 1, 2, 3 and 4 T + 1,
    and -- through an index-checking accessor -- row_ptr all ones, decreasing and random, col all ones and random: no access leaves its
    extent"""
    assert run_host_check(tmp_path, "sparse_host.cpp") >= 1000


# ------------------------------------------------------------------------------------------------- on the device
class Dev(GuardedBuffers):
    """guarded device buffers, and the calls over them"""

    def __init__(self, gm, field=0):
        super().__init__()
        self.lib, self.field, self.stream = ffi.load(), field, gm.exec_stream.raw

    def matrix(self, row_ptr, col, value_words, n_cols):
        """-> (ffi.CsrMatrix, its three buffers); an empty col / values array is passed as NULL"""
        rp, cl, vl = self.buffer(np.asarray(row_ptr, np.uint32)), self.buffer(np.asarray(col, np.uint32)), self.buffer(value_words)
        nnz = len(col)
        m = ffi.CsrMatrix(rp.ptr.value, cl.ptr.value if nnz else None, vl.ptr.value if nnz else None, len(row_ptr) - 1, n_cols, nnz)
        return m, (rp, cl, vl)

    def check(self, m):
        d, w = C.c_uint(0x7777), C.c_uint64(0x7777)
        assert self.lib.panda_sparse_check(self.field, C.byref(m), C.byref(d), C.byref(w), self.stream) == 0
        return d.value, w.value

    def matvec(self, m, z, out, batch=1):
        return self.lib.panda_sparse_matvec(self.field, C.byref(m), z.ptr, out.ptr, batch, self.stream)


def _run(gm, field, row_ptr, col, vals, zs, n_cols, what=""):
    """check + product of a valid matrix on plain residues against the definition, for the vectors `zs` in one batched call; returns the
    output words (batch, n_rows, 8)"""
    row_ptr = np.asarray(row_ptr, np.uint32)
    n_rows, batch = len(row_ptr) - 1, len(zs)
    assert int(row_ptr[-1]) == len(col) == len(vals) and all(len(z) == n_cols for z in zs)
    h = Dev(gm, field)
    try:
        m, bufs = h.matrix(row_ptr, col, fr.wire(field, vals) if len(vals) else np.zeros((0, 8), np.uint32), n_cols)
        z = h.buffer(np.concatenate([fr.wire(field, z) for z in zs]))
        out = h.buffer(nbytes=batch * n_rows * 32)
        assert h.check(m) == (0, NO_INDEX), what
        assert h.matvec(m, z, out, batch) == 0, what
        got = h.get(out).reshape(batch, n_rows, 8)
        for p in range(batch):
            want = fr.wire(field, _product(field, row_ptr, col, vals, zs[p]))
            bad = np.nonzero((got[p] != want).any(axis=1))[0]
            assert bad.size == 0, (what, field, "vector", p, "rows", bad[:8].tolist(), "of", n_rows, "nnz", len(col))
        for d in bufs + (z, out):
            assert h.intact(d), (what, "an input or a guard was written")
        return got
    finally:
        h.close()


def _random_matrix(seed, lengths, n_cols, field=0):
    row_ptr = _row_ptr(lengths)
    nnz = int(row_ptr[-1])
    col = np.random.default_rng(seed).integers(0, n_cols, nnz).astype(np.uint32)
    return row_ptr, col, fr.random_residues(field, seed + 1, nnz), fr.random_residues(field, seed + 2, n_cols)


@pytest.mark.gpu
def test_boundary_counts(gm):
    T, _ = _tile()
    for nnz in (0, 1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 4 * T + 3):
        lengths = _random_lengths(0x2A000 + nnz, nnz) if nnz else [0] * 5
        row_ptr, col, vals, z = _random_matrix(0x2B000 + nnz, lengths, 257)
        _run(gm, 0, row_ptr, col, vals, [z], 257, "nnz %d" % nnz)


@pytest.mark.gpu
def test_rows_on_tile_ends_and_rows_over_many_tiles(gm):
    T, chunk = _tile()
    many = chunk + 1 if chunk * T <= 1 << 18 else 64
    for k, lengths in enumerate(([T - 1, 1, 5, T - 6, 3],        # a row that ends at T - 1, one that ends at T, one that starts at T
                                 [T, T, 1], [3, T - 3, 0, T, 2],  # rows that are whole tiles
                                 [3 * T + 5],                     # one row holds everything
                                 [2, 3 * T + 5, 0, 2],
                                 [3, many * T + 9, 0, 4],         # one row over more tiles than the second launch takes per step
                                 [T - 2, 2 * T + 1, 3 * T + 7, T])):  # long rows back to back
        row_ptr, col, vals, z = _random_matrix(0x2C000 + 16 * k, lengths, 61)
        _run(gm, 0, row_ptr, col, vals, [z], 61, "lengths %r" % (lengths,))


@pytest.mark.gpu
def test_empty_rows(gm):
    T, _ = _tile()
    cases = {
        "first and last": [0, 0, 0, 3, 1, 2, 0, 0],
        "2 T + 1 in the middle": [2, 5, 1] + [0] * (2 * T + 1) + [4, 1],
        "a run that ends where a tile begins": [T - 4, 4] + [0] * 700 + [3, 2],
        "a run on both sides of a tile end": [T - 4, 3] + [0] * 9 + [2, 5],
        "n_rows 1": [7],
        "n_rows 1, empty": [0],
        "3 T rows, two nonzeros": [0] * 7 + [1] + [0] * (2 * T) + [1] + [0] * (T - 9),
    }
    assert len(cases["3 T rows, two nonzeros"]) == 3 * T
    for k, (what, lengths) in enumerate(cases.items()):
        row_ptr, col, vals, z = _random_matrix(0x2D000 + 16 * k, lengths, 33)
        _run(gm, 0, row_ptr, col, vals, [z], 33, what)


@pytest.mark.gpu
def test_columns(gm):
    T, _ = _tile()
    # one column: every gather hits one element
    lengths = _random_lengths(0x2E001, T + 9)
    row_ptr = _row_ptr(lengths)
    _run(gm, 0, row_ptr, np.zeros(T + 9, np.uint32), fr.random_residues(0, 0x2E002, T + 9), [fr.random_residues(0, 0x2E003, 1)], 1, "n_cols 1")
    # a row that names one column five times; unsorted columns inside the rows
    row_ptr = _row_ptr([5, 4, 6, 1])
    col = np.array([3, 3, 3, 3, 3, 9, 0, 7, 2, 8, 8, 1, 0, 9, 4, 5], np.uint32)
    _run(gm, 0, row_ptr, col, fr.random_residues(0, 0x2E004, 16), [fr.random_residues(0, 0x2E005, 10)], 10, "repeats and unsorted columns")


@pytest.mark.gpu
def test_extreme_operands(gm):
    T, _ = _tile()
    for field in (0, 1, 2):
        p = fr.modulus(field)
        lengths = [1, 2, 3, 4, 5, 6, 7, 0, 8] + _random_lengths(0x2F000 + field, T + 1 - 36)
        row_ptr, col, _, _ = _random_matrix(0x2F100 + field, lengths, 19, field)
        nnz = int(row_ptr[-1])
        assert nnz == T + 1
        _run(gm, field, row_ptr, col, [p - 1] * nnz, [[p - 1] * 19], 19, "every value and z p - 1")
        vals = [(0, 1, p - 1)[k % 3] for k in range(nnz)]
        z = [0 if c % 4 == 1 else p - 1 if c % 4 == 2 else c + 1 for c in range(19)]
        _run(gm, field, row_ptr, col, vals, [z], 19, "0, 1, p - 1 and zeros in z")
        _run(gm, field, row_ptr, col, fr.random_residues(field, 0x2F200 + field, nnz), [fr.random_residues(field, 0x2F300 + field, 19)], 19, "random, field %d" % field)


@pytest.mark.gpu
def test_batch_equals_single_calls(gm):
    T, _ = _tile()
    lengths = _random_lengths(0x30001, 2 * T + 77, longest=40)
    n_cols = len(lengths) + 13  # n_rows != n_cols
    row_ptr, col, vals, _ = _random_matrix(0x30002, lengths, n_cols)
    zs = [fr.random_residues(0, 0x30010 + p, n_cols) for p in range(3)]
    together = _run(gm, 0, row_ptr, col, vals, zs, n_cols, "batch 3")
    for p in range(3):
        alone = _run(gm, 0, row_ptr, col, vals, [zs[p]], n_cols, "single %d" % p)
        assert np.array_equal(alone[0], together[p]), p
    assert not np.array_equal(together[0], together[1])


@pytest.mark.gpu
def test_two_runs_give_equal_bytes_and_short_buffers_are_refused(gm):
    T, _ = _tile()
    row_ptr, col, vals, z = _random_matrix(0x31001, [T // 2, 2 * T, 0, 5] + _random_lengths(0x31002, T), 101)
    n_rows = len(row_ptr) - 1
    h = Dev(gm, 0)
    try:
        m, _ = h.matrix(row_ptr, col, fr.wire(0, vals), 101)
        zb = h.buffer(fr.wire(0, z))
        a, b = h.buffer(nbytes=n_rows * 32), h.buffer(nbytes=n_rows * 32)
        assert h.matvec(m, zb, a) == 0 and h.matvec(m, zb, b) == 0 and h.matvec(m, zb, a) == 0
        assert np.array_equal(h.get(a), h.get(b)) and h.intact(a) and h.intact(b)
        assert np.array_equal(h.get(a).reshape(-1, 8), fr.wire(0, _product(0, row_ptr, col, vals, z)))
        # buffers of the library's allocator that are shorter than stated: refused, nothing written
        before = h.get(a).copy()
        wide = ffi.CsrMatrix(m.d_row_ptr, m.d_col, m.d_values, m.n_rows + 2000, m.n_cols, m.nnz)  # row_ptr and out too short
        assert h.matvec(wide, zb, a) == 1
        more = ffi.CsrMatrix(m.d_row_ptr, m.d_col, m.d_values, m.n_rows, m.n_cols + 2000, m.nnz)  # z too short
        assert h.matvec(more, zb, a) == 1
        assert h.matvec(m, zb, a, batch=50) == 1, "z and out too short for the batch"
        d, w = C.c_uint(0x7777), C.c_uint64(0x7777)
        long = ffi.CsrMatrix(m.d_row_ptr, m.d_col, m.d_values, m.n_rows, m.n_cols, m.nnz + 100000)
        assert h.lib.panda_sparse_check(0, C.byref(long), C.byref(d), C.byref(w), h.stream) == 1 and (d.value, w.value) == (0x7777, 0x7777)
        assert np.array_equal(h.get(a), before)
    finally:
        h.close()


@pytest.mark.gpu
def test_check_reports_the_first_defect(gm):
    T, _ = _tile()
    field = 0
    p = fr.modulus(field)
    lengths = _random_lengths(0x32001, 2 * T + 5)
    n_cols = 40
    row_ptr, col, vals, _ = _random_matrix(0x32002, lengths, n_cols)
    nnz, n_rows = len(col), len(row_ptr) - 1
    words = fr.wire(field, vals)
    r1, r2 = n_rows // 3, n_rows - 4          # rows whose row_ptr gets raised above the next one
    k1, k2 = T // 2 + 3, T + 17               # nonzeros in two different tiles

    def report(rp=None, cl=None, vw=None, only=None):
        h = Dev(gm, field)
        try:
            m, bufs = h.matrix(row_ptr if rp is None else rp, col if cl is None else cl, words if vw is None else vw, n_cols)
            if only is not None:
                d, w = C.c_uint(0x7777), C.c_uint64(0x7777)
                assert h.lib.panda_sparse_check(field, C.byref(m), C.byref(d) if only == "defect" else None, C.byref(w) if only == "where" else None, h.stream) == 0
                got = d.value if only == "defect" else w.value
            else:
                got = h.check(m)
            assert all(h.intact(b) for b in bufs)
            return got
        finally:
            h.close()

    def raised(*rows):
        rp = row_ptr.copy()
        for r in rows:
            rp[r] = rp[r + 1] + 1
        return rp

    def columns(*ks, value=n_cols):
        cl = col.copy()
        cl[list(ks)] = value
        return cl

    def values(*ks, value=p):
        vw = words.copy()
        vw[list(ks)] = fr.words([value])[0]
        return vw

    assert report() == (0, NO_INDEX)
    assert report(only="defect") == 0 and report(only="where") == NO_INDEX
    first = row_ptr.copy()
    first[0] = 1
    assert report(rp=first) == (1, NO_INDEX)
    assert report(rp=raised(r1)) == (2, r1) and report(rp=raised(r2)) == (2, r2) and report(rp=raised(r2, r1)) == (2, r1)
    last = row_ptr.copy()
    last[n_rows] = nnz + 1
    assert report(rp=last) == (3, NO_INDEX)
    assert report(cl=columns(k2)) == (4, k2) and report(cl=columns(k1, k2)) == (4, k1) and report(cl=columns(k1, value=0xFFFFFFFF)) == (4, k1)
    assert report(cl=columns(nnz - 1, value=n_cols - 1)) == (0, NO_INDEX), "the largest legal column"
    assert report(vw=values(k2)) == (5, k2) and report(vw=values(k2, k1)) == (5, k1) and report(vw=values(k1, value=fr.W - 1)) == (5, k1)
    assert report(vw=values(k1, value=p - 1)) == (0, NO_INDEX), "the largest legal value"
    assert report(rp=raised(r2), vw=values(k1)) == (2, r2), "the smaller class wins, whatever the indices"
    assert report(rp=raised(r2), cl=columns(0), vw=values(0)) == (2, r2)
    assert report(cl=columns(k2), vw=values(k1)) == (4, k2)
    assert report(rp=first, vw=values(k1), only="where") == NO_INDEX
    # the Python helper raises on a defect and multiplies otherwise
    with pytest.raises(pgm.PandaGpuError, match="SparseDefect4"):
        pgm.panda_sparse_gpu_matvec(gm, row_ptr, columns(k1), words, fr.wire(field, range(n_cols)), n_cols, field)
    z = fr.random_residues(field, 0x32003, n_cols)
    got = pgm.panda_sparse_gpu_matvec(gm, row_ptr, col, words, fr.wire(field, z), n_cols, field)
    assert np.array_equal(got, fr.wire(field, _product(field, row_ptr, col, vals, z)))


@pytest.mark.gpu
def test_r1cs_composes_with_the_sum_of_products(gm):
    """n copies of x x = y, y x = w, w + x + 5 = out over the witness z = (1, x.., y.., w.., out..): Az, Bz, Cz by three products, then
    a b - c by panda_poly_sum_of_products on the device-resident results: zero for a satisfying witness, non-zero exactly at the rows that
    read a corrupted entry"""
    field, n = 0, 300
    p = fr.modulus(field)
    X, Y, Wv, OUT = (lambda i, b=b: 1 + b * n + i for b in range(4))
    n_cols, n_rows = 1 + 4 * n, 3 * n
    rows = {"A": [], "B": [], "C": []}
    for i in range(n):
        rows["A"] += [[(X(i), 1)], [(Y(i), 1)], [(Wv(i), 1), (0, 5), (X(i), 1)]]  # unsorted columns in the third row
        rows["B"] += [[(X(i), 1)], [(X(i), 1)], [(0, 1)]]
        rows["C"] += [[(Y(i), 1)], [(Wv(i), 1)], [(OUT(i), 1)]]
    xs = fr.random_residues(field, 0x33001, n)
    good = [1] + xs + [x * x % p for x in xs] + [x * x * x % p for x in xs] + [(x * x * x + x + 5) % p for x in xs]
    j = 123
    bad = list(good)
    bad[Y(j)] = (bad[Y(j)] + 1) % p
    T, _ = _tile()
    assert 5 * n > T, "A crosses a tile end"
    h = Dev(gm, field)
    try:
        z = h.buffer(np.concatenate([fr.wire(field, good), fr.wire(field, bad)]))
        outs = []
        for name in "ABC":
            lengths = [len(r) for r in rows[name]]
            flat = [e for r in rows[name] for e in r]
            m, _ = h.matrix(_row_ptr(lengths), [c for c, _ in flat], fr.wire(field, [v for _, v in flat]), n_cols)
            assert h.check(m) == (0, NO_INDEX)
            out = h.buffer(nbytes=2 * n_rows * 32)
            assert h.matvec(m, z, out, batch=2) == 0
            outs.append(out)
        ptrs = (C.c_void_p * 3)(*[o.ptr.value for o in outs])
        coeffs = fr.wire(field, [1, p - 1])
        degrees = (C.c_uint * 2)(2, 1)
        factors = (ffi.SopFactor * 3)(ffi.SopFactor(0, 0), ffi.SopFactor(1, 0), ffi.SopFactor(2, 0))
        expr = ffi.SopExpression(ptrs, C.c_void_p(coeffs.ctypes.data), degrees, factors, None, 3, 2, 0, ffi.SOP_SCALE_NONE)
        res = h.buffer(nbytes=2 * n_rows * 32)
        assert h.lib.panda_poly_sum_of_products(field, C.byref(expr), res.ptr, n_rows, 2, h.stream) == 0
        got = h.get(res).reshape(2, n_rows, 8)
        assert not got[0].any(), "a satisfying witness leaves a b - c zero in every row"
        assert np.nonzero(got[1].any(axis=1))[0].tolist() == [3 * j, 3 * j + 1], "the rows that read y_j"
        az = h.get(outs[0]).reshape(2, n_rows, 8)[0]
        assert np.array_equal(az[2::3], fr.wire(field, [(x * x * x + x + 5) % p for x in xs]))
        assert all(h.intact(d) for d in h.bufs)
    finally:
        h.close()
