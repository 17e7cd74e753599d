"""panda_lookup_multiplicities / panda_lookup_plan / panda_lookup_home_slot / panda_poly_running_sum / panda_poly_running_sum_plan: the two
steps of a logUp lookup argument that are not arithmetic on columns -- m_j = how many witness values equal table[j], counted at the first
row of every table value, and the exclusive running sums Z_0 = 0, Z_(i+1) = Z_i + h_i of `batch` vectors with their totals -- on elements
resident on the device.

Expected values come from Python integers: a dict of wire values for the join (the 32 bytes of an element are the key) and a running
`% r` for the sums (moduli from po.field_info).  A count c goes to the wire as c W mod r (W = 2^256).  Outputs are canonical and every
comparison is byte for byte.  Every boundary size of the running sum comes from panda_poly_running_sum_plan.  Each device buffer carries a
guard run of a fixed byte pattern behind the data, which no call may touch; inputs must come back unchanged unless they are the output."""
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
NONE_MISSING = (1 << 64) - 1
NAMES = ("panda_lookup_multiplicities", "panda_lookup_plan", "panda_lookup_home_slot", "panda_poly_running_sum", "panda_poly_running_sum_plan")


def _wire_int(field, v):
    r = fr.modulus(field)
    return v % r * fr.W % r


def _keys(a):
    """the 32 bytes of every element: what the join compares"""
    raw = np.ascontiguousarray(a, np.uint32).reshape(-1, 8).tobytes()
    return [raw[i:i + 32] for i in range(0, len(raw), 32)]


def _lookup_plan(lib, n_table, n_columns, n):
    ls, sb, la = C.c_uint(0), C.c_size_t(0), C.c_uint(0)
    rc = lib.panda_lookup_plan(n_table, n_columns, n, C.byref(ls), C.byref(sb), C.byref(la))
    return rc, ls.value, sb.value, la.value


def _sum_plan(lib, n, batch):
    t, c, ls, lt = C.c_uint(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
    rc = lib.panda_poly_running_sum_plan(n, batch, C.byref(t), C.byref(c), C.byref(ls), C.byref(lt))
    return rc, t.value, c.value, ls.value, lt.value


@functools.lru_cache(maxsize=None)
def _shape():
    """(tile, carry_chunk) of the running sum"""
    rc, tile, chunk, _, _ = _sum_plan(ffi.load(), 1, 1)
    assert rc == 0
    return tile, chunk


def _home_slot(elem, log_slots, field=0):
    e = np.ascontiguousarray(elem, np.uint32).reshape(8)
    slot = C.c_uint64(0xDEAD)
    assert ffi.load().panda_lookup_home_slot(field, C.c_void_p(e.ctypes.data), log_slots, C.byref(slot)) == 0
    return slot.value


def _lookup_expected(field, table, cols):
    """(mult words (n_table, 8), missing, first_missing) from a dict of the table's wire values"""
    first = {}
    for j, k in enumerate(_keys(table)):
        first.setdefault(k, j)
    counts = [0] * len(table)
    missing, first_missing = 0, NONE_MISSING
    for c, col in enumerate(cols):
        for i, k in enumerate(_keys(col)):
            j = first.get(k)
            if j is None:
                missing += 1
                if first_missing == NONE_MISSING:
                    first_missing = (c << 32) | i
            else:
                counts[j] += 1
    wires = {c: _wire_int(field, c).to_bytes(32, "little") for c in set(counts)}
    mult = np.frombuffer(b"".join(wires[c] for c in counts), np.uint32).reshape(-1, 8)
    return mult, missing, first_missing


def _sum_expected(field, x):
    """(exclusive running sums (n, 8), total (8,)) of one vector"""
    r = fr.modulus(field)
    sums = np.add.accumulate(np.array([0] + fr.ints(x), dtype=object)) % r  # Python integers: the running sum, then % r
    return fr.words(sums[:-1]), fr.words(sums[-1:])[0]


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, lib = assert_exported(NAMES)
    assert lib.panda_lookup_multiplicities.argtypes[2] is C.c_uint64 and lib.panda_lookup_multiplicities.argtypes[5] is C.c_uint64
    assert lib.panda_lookup_plan.argtypes[0] is C.c_uint64 and lib.panda_lookup_plan.argtypes[2] is C.c_uint64
    assert lib.panda_poly_running_sum.argtypes[3] is C.c_uint64 and lib.panda_poly_running_sum_plan.argtypes[0] is C.c_uint64
    assert int(re.search(r"#define\s+PANDA_LOOKUP_MAX_COLUMNS\s+(\d+)", header).group(1)) == ffi.LOOKUP_MAX_COLUMNS == 32


BAD_COUNTS = (0, MAX_ELEMS + 1, 1 << 63, (1 << 64) - 1)


def test_bad_arguments_are_refused_before_any_device_call():
    """every shape, pointer and overlap error returns 1 with the host outputs untouched -- also on a machine with no device"""
    lib = ffi.load()
    mem = np.full(4 << 20, 0x5A, np.uint8)  # disjoint 1 MiB host ranges stand in for the device buffers: nothing may dereference them
    base = mem.ctypes.data
    at = lambda off: C.c_void_p(base + off)
    T, A, B, O = 0, 1 << 20, 2 << 20, 3 << 20
    stream = ffi.PandaStream()
    sentinel = 0x1234567890ABCDEF
    missing, first = C.c_uint64(sentinel), C.c_uint64(sentinel)
    totals = np.full((4, 8), 0x77777777, np.uint32)

    def mult(f=0, table=at(T), n_table=16, cols=(at(A), at(B)), n_columns=None, n=64, out=at(O), columns_null=False):
        ptrs = (C.c_void_p * max(len(cols), 1))(*cols)
        return lib.panda_lookup_multiplicities(f, table, n_table, None if columns_null else ptrs, len(cols) if n_columns is None else n_columns, n, out,
                                               C.byref(missing), C.byref(first), stream)

    def rs(f=0, i=at(A), o=at(O), n=16, batch=2, tot=C.c_void_p(totals.ctypes.data)):
        return lib.panda_poly_running_sum(f, i, o, n, batch, tot, stream)

    assert mult(f=3) == 1 and rs(f=3) == 1
    for bad in BAD_COUNTS:
        assert mult(n_table=bad) == 1 and mult(n=bad) == 1 and rs(n=bad) == 1, bad
    assert rs(batch=0) == 1 and rs(n=(MAX_ELEMS >> 1) + 1, batch=2) == 1 and rs(n=1, batch=MAX_ELEMS + 1) == 1 and rs(n=1 << 32, batch=1 << 31) == 1
    assert mult(n_columns=0) == 1 and mult(cols=(at(A),) * 33, n=1) == 1 and mult(n_columns=33) == 1
    assert mult(n=(MAX_ELEMS >> 1) + 1) == 1, "n_columns x n over the cap"
    assert mult(cols=(at(A),) * 32, n=(MAX_ELEMS >> 5) + 1) == 1 and mult(cols=(at(A),) * 3, n=1 << 63) == 1
    assert mult(table=None) == 1 and mult(columns_null=True) == 1 and mult(out=None) == 1
    assert mult(cols=(None, at(B))) == 1 and mult(cols=(at(A), None)) == 1
    # a table of 16 elements is 512 bytes, a column of 64 is 2048: every way d_mult's 512 bytes meet either range
    tb, cb = 16 * 32, 64 * 32
    for off in (0, tb - 1, 32, -32, -(tb - 1)):
        assert mult(table=at(T + 4096), out=at(T + 4096 + off)) == 1, off
    for off in (0, 32, cb - 32, cb - 1, -32, -(tb - 1), 1024):
        assert mult(cols=(at(A + 4096), at(B)), out=at(A + 4096 + off)) == 1, off
        assert mult(cols=(at(A), at(B + 4096)), out=at(B + 4096 + off)) == 1, off
        assert mult(cols=(at(B + 4096),) * 2, out=at(B + 4096 + off)) == 1, off
    assert mult(cols=(at(T), at(B)), table=at(T), out=at(T)) == 1
    assert rs(o=None, tot=None) == 1 and rs(i=None) == 1 and rs(i=None, o=None) == 1
    for off in (1023, 32, -32, -1023):  # 2 vectors of 16 are 1024 bytes
        assert rs(i=at(A + 4096), o=at(A + 4096 + off)) == 1, off
    assert missing.value == sentinel and first.value == sentinel, "a refused call wrote a host output"
    assert (totals == 0x77777777).all() and (mem == 0x5A).all(), "a refused call wrote to totals or a buffer"
    slot = C.c_uint64(sentinel)
    elem = np.zeros(8, np.uint32)
    ep = C.c_void_p(elem.ctypes.data)
    assert lib.panda_lookup_home_slot(3, ep, 4, C.byref(slot)) == 1 and lib.panda_lookup_home_slot(0, None, 4, C.byref(slot)) == 1
    assert lib.panda_lookup_home_slot(0, ep, 4, None) == 1
    assert lib.panda_lookup_home_slot(0, ep, 0, C.byref(slot)) == 1 and lib.panda_lookup_home_slot(0, ep, 30, C.byref(slot)) == 1
    assert slot.value == sentinel
    assert lib.panda_lookup_home_slot(0, ep, 29, C.byref(slot)) == 0 and slot.value < 1 << 29
    # the plans refuse exactly the same shapes
    for bad in BAD_COUNTS:
        assert lib.panda_lookup_plan(bad, 1, 1, None, None, None) == 1 and lib.panda_lookup_plan(1, 1, bad, None, None, None) == 1
        assert lib.panda_poly_running_sum_plan(bad, 1, None, None, None, None) == 1
    for n_columns, n in ((0, 1), (33, 1), (2, (MAX_ELEMS >> 1) + 1), (32, (MAX_ELEMS >> 5) + 1), (3, 1 << 63)):
        assert lib.panda_lookup_plan(1, n_columns, n, None, None, None) == 1, (n_columns, n)
    for n, batch in ((1, 0), ((MAX_ELEMS >> 1) + 1, 2), (1, MAX_ELEMS + 1), (1 << 63, 2), (1 << 32, 1 << 31)):
        assert lib.panda_poly_running_sum_plan(n, batch, None, None, None, None) == 1, (n, batch)
    assert lib.panda_lookup_plan(MAX_ELEMS, 32, MAX_ELEMS >> 5, None, None, None) == 0 and lib.panda_poly_running_sum_plan(MAX_ELEMS, 1, None, None, None, None) == 0


def test_plans():
    lib = ffi.load()
    for n_table in (1, 2, 3, 7, 8, 9, (1 << 16) + 3, 1 << 24, 1 << 28):
        seen = set()
        for n_columns, n in ((1, 1), (1, 1000), (3, 1 << 20), (32, 1 << 23), (1, 1 << 28)):
            rc, log_slots, scratch, launches = _lookup_plan(lib, n_table, n_columns, n)
            assert rc == 0 and 1 <= log_slots <= 29 and (1 << log_slots) >= 2 * n_table and launches >= 1, (n_table, n_columns, n)
            assert scratch >= (1 << log_slots) * 8, "the slots alone need this much"
            seen.add((log_slots, launches))
            outs = (log_slots, scratch, launches)
            for i in range(3):  # every out pointer may be NULL, singly
                vals = [C.c_uint(0xDEAD), C.c_size_t(0xDEAD), C.c_uint(0xDEAD)]
                args = [C.byref(v) if j != i else None for j, v in enumerate(vals)]
                assert lib.panda_lookup_plan(n_table, n_columns, n, *args) == 0
                assert [v.value for j, v in enumerate(vals) if j != i] == [v for j, v in enumerate(outs) if j != i]
        assert len(seen) == 1, "nothing but scratch_bytes depends on the columns"
    for n in (1, 2, 3, 63, 64, 65, 1000, (1 << 16) + 3, (1 << 20) + 3, 1 << 24, 1 << 28):
        seen = set()
        for batch in (1, 2, 3, 16, 1 << 20, 1 << 28):
            if n * batch > MAX_ELEMS:
                assert lib.panda_poly_running_sum_plan(n, batch, None, None, None, None) == 1
                continue
            rc, tile, chunk, l_scan, l_total = _sum_plan(lib, n, batch)
            assert rc == 0 and tile >= 1 and chunk >= 1 and l_scan >= l_total >= 1, (n, batch)
            seen.add((tile, chunk, l_scan, l_total))
            for i in range(4):
                vals = [C.c_uint(0xDEAD) for _ in range(4)]
                args = [C.byref(v) if j != i else None for j, v in enumerate(vals)]
                assert lib.panda_poly_running_sum_plan(n, batch, *args) == 0
                assert [v.value for j, v in enumerate(vals) if j != i] == [v for j, v in enumerate((tile, chunk, l_scan, l_total)) if j != i]
        assert len(seen) == 1, "none of the four depends on the batch"


@functools.lru_cache(maxsize=None)
def _pool(field=0, count=4096, seed=0x10061):
    x = po.gen_scalars(po.FR_OF[field], seed, count).reshape(count, 8)
    x.setflags(write=False)
    return x


def test_home_slot():
    pool = _pool()
    for log_slots in (1, 4, 5, 16, 29):
        for e in pool[:64]:
            s = _home_slot(e, log_slots)
            assert s < 1 << log_slots and s == _home_slot(np.array(e), log_slots)
    assert {_home_slot(e, 4) for e in pool} == set(range(16)), "over 4096 elements every one of 16 slots is some element's home"
    # elements that differ in exactly one of the eight words: each word must reach the slot
    base = np.array(pool[0])
    for word in range(8):
        slots = set()
        for k in range(256):
            e = base.copy()
            e[word] ^= np.uint32(k + 1) if word < 7 else np.uint32((k + 1) & 0x0FFFFFFF)  # stays a 256-bit value; canonical or not, the hash takes it
            slots.add(_home_slot(e, 4))
        assert len(slots) == 16, "word %d does not spread over the slots" % word


def test_host_program_checks_the_hash_and_the_bounds(tmp_path):
    """tests/host_check/lookup_host.cpp: lookup.h on the host under FE29_CHECK -- the hash against panda_lookup_home_slot, the count ->
    wire conversion at 0, 1, 2^28 - 1 and 2^28 and the running sum's addition chains at their bound with every operand p - 1, against
    256-bit arithmetic of its own, the three fields"""
    assert run_host_check(tmp_path, "lookup_host.cpp") >= 200
    elems = [np.array(e) for e in _pool()[:48]] + [np.zeros(8, np.uint32), np.full(8, 0xFFFFFFFF, np.uint32)]
    for log_slots in (1, 4, 5, 20, 29):
        out = run_host_check(tmp_path, "lookup_host.cpp", "hash", str(log_slots), *[e.tobytes().hex() for e in elems])
        assert out.returncode == 0
        assert [int(v) for v in out.stdout.split()] == [_home_slot(e, log_slots) for e in elems], log_slots


# ------------------------------------------------------------------------------------------------- on the device
class Lookup(GuardedBuffers):
    """guarded device buffers for a table, up to `max_columns` columns and the multiplicities, with room for the largest data they will
    hold: the guard run stands right behind the data of each run"""

    def __init__(self, gm, field, max_table, max_n, max_columns):
        super().__init__()
        self.lib, self.field, self.stream = ffi.load(), field, gm.exec_stream.raw
        self.t, self.m = self.buffer(nbytes=max_table * 32), self.buffer(nbytes=max_table * 32)
        self.c = [self.buffer(nbytes=max_n * 32) for _ in range(max_columns)]

    def stage(self, table, cols):
        self.fill(self.t, table)
        self.fill(self.m, nbytes=len(table) * 32)
        for d, col in zip(self.c, cols):
            self.fill(d, col)

    def run(self, table, cols, pointers=None, keep=False):
        """one panda_lookup_multiplicities -> (mult (n_table, 8), missing, first_missing); checks the guards and that the inputs are
        unchanged.  pointers: for every column "t" (d_table's pointer) or the index of the staged column to pass; keep: do not restage"""
        if not keep:
            self.stage(table, cols)
        n = len(cols[0])
        where = list(range(len(cols))) if pointers is None else pointers
        ptrs = (C.c_void_p * len(where))(*[self.t.ptr.value if w == "t" else self.c[w].ptr.value for w in where])
        missing, first = C.c_uint64(0x1111), C.c_uint64(0x2222)
        ffi.check(self.lib.panda_lookup_multiplicities(self.field, self.t.ptr, len(table), ptrs, len(where), n, self.m.ptr, C.byref(missing), C.byref(first), self.stream),
                  "multiplicities")
        assert self.intact(self.t), "the table or the bytes behind it were written"
        for d, _ in zip(self.c, cols):
            assert self.intact(d), "a column or the bytes behind it were written"
        assert self.guard_intact(self.m), "bytes behind d_mult were written"
        return self.get(self.m).reshape(-1, 8), missing.value, first.value

    def check(self, table, cols, pointers=None):
        mult, missing, first = self.run(table, cols, pointers)
        passed = cols if pointers is None else [table if w == "t" else cols[w] for w in pointers]
        want, want_missing, want_first = _lookup_expected(self.field, table, passed)
        assert np.array_equal(mult, want), (len(table), len(passed), len(passed[0]))
        assert (missing, first) == (want_missing, want_first)
        return mult, missing, first


def _count_sum(field, mult):
    """sum of the multiplicities as an integer (each is c W mod r with a small c)"""
    return sum(fr.plain(field, mult))


TABLE_SIZES = (1, 2, 3, 7, 8, 9, 255, 256, 257, 1000)
VALUE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000, 5 * 256 - 7)


@pytest.mark.gpu
@pytest.mark.parametrize("n_columns", [1, 3])
def test_multiplicities_at_the_boundary_shapes(gm, n_columns):
    """values drawn from the table with replacement: sum m == the value count, nothing missing"""
    pool, rng = _pool(), np.random.default_rng(0x20 + n_columns)
    h = Lookup(gm, 0, max(TABLE_SIZES), max(VALUE_COUNTS), n_columns)
    try:
        for n_table in TABLE_SIZES:
            table = pool[rng.choice(len(pool), n_table, replace=False)]
            for n in VALUE_COUNTS:
                cols = [table[rng.integers(0, n_table, n)] for _ in range(n_columns)]
                mult, missing, first = h.check(table, cols)
                assert missing == 0 and first == NONE_MISSING and _count_sum(0, mult) == n_columns * n
    finally:
        h.close()


def _chain_table(log_slots):
    """a table whose plan has `log_slots`: four rows sharing one home slot, two rows whose home is the last slot (the second wraps to
    slot 0 or beyond), filled up from the pool; and absent values whose home is the head of either chain"""
    pool = _pool()
    by_slot = {}
    for k, e in enumerate(pool):
        by_slot.setdefault(_home_slot(e, log_slots), []).append(k)
    last, head = (1 << log_slots) - 1, 3
    n_table = 1 << (log_slots - 1)
    chain, wrap = by_slot[head][:4], by_slot[last][:2]
    assert len(chain) == 4 and len(wrap) == 2
    absent = by_slot[head][4:7] + by_slot[last][2:4]
    assert len(absent) == 5
    used = set(chain + wrap + absent)
    rest = [k for k in range(len(pool)) if k not in used][:n_table - 6]
    rows = wrap + rest[:1] + chain + rest[1:]  # the wrap-around rows first, the chain in the middle
    assert len(rows) == n_table and _lookup_plan(ffi.load(), n_table, 1, 1)[1] == log_slots
    return pool[rows], pool[chain], pool[wrap], pool[absent]


@pytest.mark.gpu
@pytest.mark.parametrize("log_slots", [4, 5])
def test_collision_chains_and_wrap_around(gm, log_slots):
    table, chain, wrap, absent = _chain_table(log_slots)
    h = Lookup(gm, 0, len(table), 64, 2)
    try:
        ends = np.concatenate([chain[3:], wrap[1:]])  # the values at the end of the two chains
        col0 = np.concatenate([ends] * 5 + [table, chain, wrap])
        mult, missing, first = h.check(table, [col0])
        assert missing == 0 and _count_sum(0, mult) == len(col0)
        # absent values whose walk starts at the head of a chain: it must reach the empty slot behind the chain and report a miss
        col0 = np.concatenate([table[:7], absent, ends, ends])
        col1 = np.concatenate([ends, ends, absent[::-1], table[:7]])
        mult, missing, first = h.check(table, [col0, col1])
        assert missing == 10 and first == 7 and _count_sum(0, mult) == 2 * len(col0) - 10
    finally:
        h.close()


@pytest.mark.gpu
def test_duplicate_table_rows(gm):
    pool = _pool()
    table = np.array(pool[:8])
    table[5] = table[6] = table[2]
    col = np.concatenate([table, table[2:3], table[6:7], table[0:1]])
    h = Lookup(gm, 0, 8, len(col), 1)
    try:
        mult, missing, _ = h.check(table, [col])
        zero = np.zeros(8, np.uint32)
        assert missing == 0 and np.array_equal(mult[2], fr.words([_wire_int(0, 5)])[0]) and np.array_equal(mult[5], zero) and np.array_equal(mult[6], zero)
        for _ in range(5):
            again, _, _ = h.run(table, [col], keep=True)
            assert again.tobytes() == mult.tobytes(), "d_mult differs between two runs on the same buffers"
        same = np.broadcast_to(pool[9], (8, 8))
        col = np.concatenate([same[:3], pool[10:11]])
        mult, missing, first = h.check(same, [col])
        assert np.array_equal(mult[0], fr.words([_wire_int(0, 3)])[0]) and not mult[1:].any() and missing == 1 and first == 3
        for _ in range(5):
            again, _, _ = h.run(same, [col], keep=True)
            assert again.tobytes() == mult.tobytes()
    finally:
        h.close()


@pytest.mark.gpu
def test_misses(gm):
    pool = _pool()
    table, absent = pool[:300], pool[2000:2100]
    rng = np.random.default_rng(0x31)
    n = 700
    h = Lookup(gm, 0, 300, n, 3)
    try:
        cols = [np.array(table[rng.integers(0, 300, n)]) for _ in range(3)]
        _, missing, first = h.check(table, cols)
        assert missing == 0 and first == NONE_MISSING
        planted = [(0, 699), (1, 64), (1, 65), (2, 0), (0, 257)]
        for k, (c, i) in enumerate(planted):
            cols[c][i] = absent[k]
        _, missing, first = h.check(table, cols)
        assert missing == len(planted) and first == (0 << 32) | 257
        cols[0][699], cols[0][257] = table[0], table[1]  # the smallest pair is now in column 1
        _, missing, first = h.check(table, cols)
        assert missing == 3 and first == (1 << 32) | 64
        cols[2][1] = absent[7]
        cols[1][64], cols[1][65] = absent[7], absent[7]  # one absent value several times counts every time
        _, missing, first = h.check(table, cols)
        assert missing == 4 and first == (1 << 32) | 64
        # the wire zero is an ordinary value: absent from this table, present in the next
        cols[0][5] = 0
        _, missing, first = h.check(table, cols)
        assert missing == 5 and first == 5
        with_zero = np.array(table)
        with_zero[17] = 0
        mult, missing, first = h.check(with_zero, cols)  # what held table[17] before is missing now; the zero is found once
        assert np.array_equal(mult[17], fr.words([_wire_int(0, 1)])[0]) and missing >= 4
    finally:
        h.close()


@pytest.mark.gpu
def test_skewed_columns(gm):
    """padding rows all hold one value: the probe's per-wave combining must still count exactly"""
    pool = _pool()
    table, n = pool[:1000], 1 << 16
    rng = np.random.default_rng(0x41)
    h = Lookup(gm, 0, 1000, n, 1)
    try:
        mult, missing, _ = h.check(table, [np.broadcast_to(table[37], (n, 8))])
        assert missing == 0 and np.array_equal(mult[37], fr.words([_wire_int(0, n)])[0]) and _count_sum(0, mult) == n
        idx = np.where(rng.random(n) < 0.9, 501, rng.integers(0, 1000, n))
        mult, missing, _ = h.check(table, [table[idx]])
        assert missing == 0 and _count_sum(0, mult) == n
        idx = np.where(rng.random(n) < 0.5, 2, np.where(rng.random(n) < 0.5, 3, rng.integers(0, 8, n)))  # a few hot slots in every wave
        mult, missing, _ = h.check(table, [table[idx]])
        assert missing == 0 and _count_sum(0, mult) == n
    finally:
        h.close()


@pytest.mark.gpu
def test_aliased_columns(gm):
    pool = _pool()
    table = np.array(pool[:513])
    table[100] = table[7]
    rng = np.random.default_rng(0x51)
    col = table[rng.integers(0, 513, 513)]
    h = Lookup(gm, 0, 513, 513, 1)
    try:
        mult, missing, _ = h.check(table, [col], pointers=["t"])  # the table looked up in itself
        assert missing == 0 and _count_sum(0, mult) == 513
        first_rows = [j for j in range(513) if j != 100]
        assert all(mult[j].any() for j in first_rows) and not mult[100].any(), "every value's first row counts at least itself"
        single, _, _ = h.check(table, [col])
        double, missing, _ = h.check(table, [col], pointers=[0, 0])
        r = fr.modulus(0)
        assert missing == 0 and [v for v in fr.ints(double)] == [2 * v % r for v in fr.ints(single)]
        mixed, missing, _ = h.check(table, [col], pointers=[0, "t", 0])
        assert missing == 0 and _count_sum(0, mixed) == 3 * 513
    finally:
        h.close()


@pytest.mark.gpu
def test_a_grid_sized_lookup(gm):
    """table 2^16, four columns of 2^18, uniform with 1 % misses"""
    n_table, n = 1 << 16, 1 << 18
    data = po.gen_scalars(po.FR_OF[0], 0x61, n_table + 4096).reshape(-1, 8)
    table, absent = data[:n_table], data[n_table:]
    rng = np.random.default_rng(0x61)
    cols = []
    for _ in range(4):
        col = table[rng.integers(0, n_table, n)]
        where = np.flatnonzero(rng.random(n) < 0.01)
        col[where] = absent[rng.integers(0, len(absent), len(where))]
        cols.append(col)
    h = Lookup(gm, 0, n_table, n, 4)
    try:
        mult, missing, first = h.check(table, cols)
        assert 0 < missing < 4 * n // 50 and first < n and _count_sum(0, mult) == 4 * n - missing
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_multiplicities_in_the_other_fields(gm, field):
    pool = _pool(field, 1024, 0x70 + field)
    table = pool[:257]
    rng = np.random.default_rng(0x70 + field)
    cols = [np.array(table[rng.integers(0, 257, 5 * 256 - 7)]) for _ in range(2)]
    cols[1][77] = pool[900]
    h = Lookup(gm, field, 257, 5 * 256 - 7, 2)
    try:
        mult, missing, first = h.check(table, cols)
        assert missing == 1 and first == (1 << 32) | 77 and _count_sum(field, mult) == 2 * (5 * 256 - 7) - 1
    finally:
        h.close()


@pytest.mark.gpu
def test_short_buffers_are_refused(gm):
    from gpu_util import DeviceBuffer
    pool = _pool()
    table, col = pool[:64], pool[:128]
    h = Lookup(gm, 0, 64, 128, 1)
    short = DeviceBuffer(64 * 32 - 32)  # one element short of a table
    try:
        h.stage(table, [col])
        ffi.check(h.lib.panda_memset(short.ptr, GUARD, short.nbytes), "memset")
        sentinel = 0x1234567890ABCDEF
        missing, first = C.c_uint64(sentinel), C.c_uint64(sentinel)
        call = lambda t, c, n, m: h.lib.panda_lookup_multiplicities(0, t, 64, (C.c_void_p * 1)(c.value), 1, n, m, C.byref(missing), C.byref(first), h.stream)
        assert call(short.ptr, h.c[0].ptr, 128, h.m.ptr) == 1 and call(h.t.ptr, h.c[0].ptr, 128, short.ptr) == 1 and call(h.t.ptr, short.ptr, 64, h.m.ptr) == 1
        tot = np.full((1, 8), 0x77777777, np.uint32)
        rs = lambda i, o: h.lib.panda_poly_running_sum(0, i, o, 64, 1, C.c_void_p(tot.ctypes.data), h.stream)
        assert rs(short.ptr, h.m.ptr) == 1 and rs(h.t.ptr, short.ptr) == 1 and rs(short.ptr, short.ptr) == 1 and rs(short.ptr, None) == 1
        for k in (32, 64 * 32 - 32):
            assert rs(h.c[0].ptr, C.c_void_p(h.c[0].ptr.value + k)) == 1 and rs(C.c_void_p(h.c[0].ptr.value + k), h.c[0].ptr) == 1
            assert call(h.t.ptr, h.c[0].ptr, 128, C.c_void_p(h.t.ptr.value + k)) == 1
        assert missing.value == sentinel and first.value == sentinel and (tot == 0x77777777).all()
        assert (short.to_host(np.uint8) == GUARD).all() and h.intact(h.t) and h.intact(h.c[0]) and h.untouched(h.m), "a refused call wrote to a buffer"
        h.check(table, [col])
    finally:
        short.free()
        h.close()


# ------------------------------------------------------------------------------------------------- the running sum
class Sums(GuardedBuffers):
    """two guarded device buffers of batch x n elements"""

    def __init__(self, gm, field, n, batch):
        super().__init__()
        self.lib, self.field, self.n, self.batch, self.stream = ffi.load(), field, n, batch, gm.exec_stream.raw
        self.a, self.o = self.buffer(nbytes=batch * n * 32), self.buffer(nbytes=batch * n * 32)

    def run(self, x, where="o", totals=True):
        """one panda_poly_running_sum -> (out (batch, n, 8) or None, totals (batch, 8) or None); where: "o" out of place, "a" in place,
        None totals only (d_out == NULL)"""
        self.fill(self.a, x)
        self.fill(self.o)
        assert self.a.data_bytes == self.o.data_bytes
        dst = {"o": self.o, "a": self.a, None: None}[where]
        tot = np.full((self.batch, 8), 0x77777777, np.uint32) if totals else None
        ffi.check(self.lib.panda_poly_running_sum(self.field, self.a.ptr, None if dst is None else dst.ptr, self.n, self.batch,
                                                  C.c_void_p(tot.ctypes.data) if totals else None, self.stream), "running_sum")
        assert self.guard_intact(self.a) and self.guard_intact(self.o), "bytes behind the batch were written"
        if where != "a":
            assert self.intact(self.a), "d_in was written"
        if where != "o":
            assert self.untouched(self.o), "a buffer that is not the output was written"
        return (None if dst is None else self.get(dst).reshape(self.batch, self.n, 8)), tot


@functools.lru_cache(maxsize=None)
def _vectors(field, n, batch, seed):
    x = po.gen_scalars(po.FR_OF[field], seed, batch * n).reshape(batch, n, 8)
    x.setflags(write=False)
    return x


def _check_all_forms(gm, field, x):
    batch, n = x.shape[:2]
    want = [_sum_expected(field, x[p]) for p in range(batch)]
    want_out, want_tot = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    h = Sums(gm, field, n, batch)
    try:
        out, tot = h.run(x)
        assert np.array_equal(out, want_out) and np.array_equal(tot, want_tot), (field, n, batch)
        out, tot = h.run(x, where="a")
        assert np.array_equal(out, want_out) and np.array_equal(tot, want_tot), (field, n, batch, "in place")
        out, tot = h.run(x, where=None)  # the guard-filled stand-in for d_out must stay untouched: checked in run
        assert out is None and np.array_equal(tot, want_tot), (field, n, batch, "totals only")
        out, tot = h.run(x, totals=False)
        assert tot is None and np.array_equal(out, want_out), (field, n, batch, "without totals")
    finally:
        h.close()


def _small_sizes():
    tile = _shape()[0]
    return sorted({1, 2, 3, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1})


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 3])
def test_running_sum_at_the_boundary_sizes(gm, batch):
    """n around the wave, the tile and several tiles with a ragged tail (from the plan, so walked inside one test)"""
    for n in _small_sizes():
        _check_all_forms(gm, 0, _vectors(0, n, batch, 0xA000 + n))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 3])
def test_running_sum_at_the_second_level(gm, batch):
    """one tile sum more than one step of the seed kernel takes"""
    tile, chunk = _shape()
    n = tile * chunk + 1
    assert n <= 1 << 22, "the plan's tile x carry_chunk is too large for a quick test"
    _check_all_forms(gm, 0, _vectors(0, n, batch, 0xB000))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["minus_ones", "zeros"])
def test_running_sum_edge_values(gm, case):
    tile = _shape()[0]
    n, batch, r = 2 * tile + 1, 2, fr.modulus(0)
    v = fr.words([r - 1])[0] if case == "minus_ones" else np.zeros(8, np.uint32)
    x = np.ascontiguousarray(np.broadcast_to(v, (batch, n, 8)))
    _check_all_forms(gm, 0, x)
    if case == "zeros":
        h = Sums(gm, 0, n, batch)
        try:
            out, tot = h.run(x)
            assert not out.any() and not tot.any()
        finally:
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_running_sum_in_the_other_fields(gm, field):
    tile = _shape()[0]
    _check_all_forms(gm, field, _vectors(field, tile + 1, 2, 0xC000 + field))
    r = fr.modulus(field)
    _check_all_forms(gm, field, np.ascontiguousarray(np.broadcast_to(fr.words([r - 1])[0], (1, 2 * tile + 1, 8))))


@pytest.mark.gpu
def test_scratch_is_reused_and_released(gm):
    tile = _shape()[0]
    pool = _pool()
    table = pool[:1000]
    cols = [table[np.random.default_rng(0xD1).integers(0, 1000, 5 * 256 - 7)] for _ in range(2)]
    x = _vectors(0, 5 * tile - 7, 4, 0xD000)
    h, s = Lookup(gm, 0, 1000, 5 * 256 - 7, 2), Sums(gm, 0, 5 * tile - 7, 4)
    try:
        h.run(table, cols)  # whatever the runtime keeps from a kernel's first launch is there before the baseline is read
        s.run(x)
        s.run(x, where=None)
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        before = free_bytes(h.lib)
        m1 = h.run(table, cols)
        first = free_bytes(h.lib)
        m2 = h.run(table, cols)
        assert free_bytes(h.lib) == first, "a repeated identical call allocated"
        o1, t1 = s.run(x)  # needs less scratch than the lookup's slots
        o2, t2 = s.run(x)
        s.run(x, where=None)
        assert free_bytes(h.lib) == first
        assert m1[0].tobytes() == m2[0].tobytes() and m1[1:] == m2[1:] and np.array_equal(o1, o2) and np.array_equal(t1, t2)
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        assert free_bytes(h.lib) == before, "panda_ntt_tear_down releases the scratch"
    finally:
        h.close()
        s.close()


# ------------------------------------------------------------------------------------------------- the point of the feature
class _Expression:
    """the ctypes arrays of one panda_sop_expression (coefficients are wire words); they stay alive with the object"""

    def __init__(self, ptrs, terms):
        self.ptrs = (C.c_void_p * len(ptrs))(*ptrs)
        self.coeffs = np.ascontiguousarray(fr.words([k for k, _ in terms]))
        self.degrees = (C.c_uint * len(terms))(*[len(fs) for _, fs in terms])
        flat = [f for _, fs in terms for f in fs]
        self.factors = (ffi.SopFactor * max(len(flat), 1))(*[ffi.SopFactor(c, rot) for c, rot in flat])
        self.expr = ffi.SopExpression(self.ptrs, C.c_void_p(self.coeffs.ctypes.data), self.degrees, self.factors, None, len(ptrs), len(terms), 0, 0)


@pytest.mark.gpu
def test_a_real_lookup(gm):
    """a table of 2^10 rows, two witness columns of 2^12 drawn from it, a random alpha; multiplicities -> sum_of_products (alpha + f,
    alpha + t) -> batch_inverse -> sum_of_products (h) -> running_sum, everything on the device.  The witness columns are read as eight
    columns of the table's length, so h_i = sum_{k < 8} 1 / (alpha + f_k,i) - m_i / (alpha + t_i) lives on the table's domain."""
    from gpu_util import DeviceBuffer
    lib, field, stream = ffi.load(), 0, gm.exec_stream.raw
    r = fr.modulus(field)
    nt, n, parts = 1 << 10, 1 << 12, 8
    data = po.gen_scalars(po.FR_OF[field], 0xE1, nt + 2).reshape(-1, 8)
    table, absent, alpha_w = data[:nt], data[nt], fr.ints(data[nt + 1])[0]
    rng = np.random.default_rng(0xE1)
    witness = np.ascontiguousarray(table[rng.integers(0, nt, 2 * n)])  # the two columns end to end: eight parts of nt
    winv = pow(fr.W, -1, r)
    # X = [f (8 x nt) | t (nt)], D = alpha + X and then 1 / D, M = multiplicities, H = h, Z = the running sum
    X, D, M, H, Z = (DeviceBuffer(k * nt * 32) for k in (parts + 1, parts + 1, 1, 1, 1))
    at = lambda d, k: d.ptr.value + k * nt * 32
    one_w, minus_one_w = fr.W % r, (r - 1) * fr.W % r
    denominators = _Expression([X.ptr.value], [(one_w, [(0, 0)]), (alpha_w, [])])
    h_expr = _Expression([at(D, k) for k in range(parts + 1)] + [M.ptr.value],
                         [(one_w, [(k, 0)]) for k in range(parts)] + [(minus_one_w, [(parts, 0), (parts + 1, 0)])])

    def chain(wit):
        ffi.check(lib.panda_memcpy(X.ptr, C.c_void_p(wit.ctypes.data), wit.nbytes), "memcpy")
        ffi.check(lib.panda_memcpy(C.c_void_p(at(X, parts)), C.c_void_p(np.ascontiguousarray(table).ctypes.data), nt * 32), "memcpy")
        cols = (C.c_void_p * 2)(X.ptr.value, X.ptr.value + n * 32)
        missing, first = C.c_uint64(0), C.c_uint64(0)
        ffi.check(lib.panda_lookup_multiplicities(field, C.c_void_p(at(X, parts)), nt, cols, 2, n, M.ptr, C.byref(missing), C.byref(first), stream), "multiplicities")
        ffi.check(lib.panda_poly_sum_of_products(field, C.byref(denominators.expr), D.ptr, nt, parts + 1, stream), "denominators")
        ffi.check(lib.panda_field_batch_inverse(field, D.ptr, D.ptr, (parts + 1) * nt, stream), "inverse")
        ffi.check(lib.panda_poly_sum_of_products(field, C.byref(h_expr.expr), H.ptr, nt, 1, stream), "h")
        tot = np.full((1, 8), 0x77777777, np.uint32)
        ffi.check(lib.panda_poly_running_sum(field, H.ptr, Z.ptr, nt, 1, C.c_void_p(tot.ctypes.data), stream), "running_sum")
        return missing.value, first.value, tot[0], M.to_host().reshape(-1, 8), H.to_host().reshape(-1, 8), Z.to_host().reshape(-1, 8)

    try:
        missing, first, tot, m, h, z = chain(witness)
        want_m, _, _ = _lookup_expected(field, table, [witness])
        assert missing == 0 and first == NONE_MISSING and np.array_equal(m, want_m)
        assert not tot.any(), "the logUp sum of a valid lookup is zero"
        # the same h and Z from Python integers, on plain values
        alpha = alpha_w * winv % r
        f = [v * winv % r for v in fr.ints(witness)]
        t = [v * winv % r for v in fr.ints(table)]
        counts = [v * winv % r for v in fr.ints(want_m)]
        hs = [(sum(pow(alpha + f[k * nt + i], -1, r) for k in range(parts)) - counts[i] * pow(alpha + t[i], -1, r)) % r for i in range(nt)]
        zs, acc = [], 0
        for v in hs:
            zs.append(acc)
            acc = (acc + v) % r
        assert acc == 0
        assert np.array_equal(h, fr.wire(field, hs)) and np.array_equal(z, fr.wire(field, zs)), "every Z_i is the running sum"
        assert (fr.ints(z[-1:])[0] + fr.ints(h[-1:])[0]) % r == 0, "Z's last step closes"
        bad = np.array(witness)
        bad[n + 123] = absent
        missing, first, tot, _, _, _ = chain(bad)
        assert missing == 1 and first == (1 << 32) | 123 and tot.any(), "a value that is not in the table breaks the sum"
    finally:
        for d in (X, D, M, H, Z):
            d.free()


@pytest.mark.gpu
def test_gpu_manager_helpers(gm):
    pool = _pool()
    table = np.array(pool[:300])
    rng = np.random.default_rng(0xF1)
    cols = [np.array(table[rng.integers(0, 300, 777)]) for _ in range(3)]
    cols[2][5] = pool[3000]
    keep = [c.copy() for c in cols]
    mult, missing, first = pgm.panda_lookup_gpu_multiplicities(gm, table, cols)
    want, want_missing, want_first = _lookup_expected(0, table, cols)
    assert mult.shape == (300, 8) and mult.dtype == np.uint32 and np.array_equal(mult, want) and (missing, first) == (want_missing, want_first) == (1, (2 << 32) | 5)
    assert all(np.array_equal(a, b) for a, b in zip(cols, keep)) and np.array_equal(table, pool[:300]), "a helper changed its input"
    h = Lookup(gm, 0, 300, 777, 3)
    try:
        raw, raw_missing, raw_first = h.run(table, cols)
        assert np.array_equal(raw, mult) and (raw_missing, raw_first) == (missing, first)
    finally:
        h.close()
    tile = _shape()[0]
    n, batch = tile + 3, 3
    x = _vectors(0, n, batch, 0xF200)
    vecs = [np.array(v) for v in x]
    sums, totals = pgm.panda_poly_gpu_running_sum(gm, vecs)
    assert len(sums) == batch and totals.shape == (batch, 8) and totals.dtype == np.uint32
    s = Sums(gm, 0, n, batch)
    try:
        raw, raw_tot = s.run(x)
    finally:
        s.close()
    for p in range(batch):
        want, want_t = _sum_expected(0, x[p])
        assert sums[p].shape == (n, 8) and np.array_equal(sums[p], want) and np.array_equal(totals[p], want_t)
        assert np.array_equal(raw[p], want) and np.array_equal(raw_tot[p], want_t) and np.array_equal(vecs[p], x[p])
    s0, t0 = pgm.panda_poly_gpu_running_sum(gm, [])
    assert s0 == [] and t0.shape == (0, 8)


@pytest.mark.gpu
@pytest.mark.gpu_soak
def test_2_24(gm):
    """table 2^24 with one column of 2^24, by sum m, missing and 4096 sampled rows against a dict of the sampled values; the running sum at
    2^24 + 3 through the oracle's vector ops by out_(i+1) = out_i + in_i"""
    fid = po.FR_OF[0]
    nt = n = 1 << 24
    table = po.gen_scalars(fid, 0x2401, nt).reshape(-1, 8)
    rng = np.random.default_rng(0x24)
    idx = rng.integers(0, nt, n)
    col = table[idx]
    absent_at = rng.choice(n, 1000, replace=False)
    col[absent_at] = po.gen_scalars(fid, 0x2402, 1000).reshape(-1, 8)
    h = Lookup(gm, 0, nt, n, 1)
    try:
        mult, missing, first = h.run(table, [col])
        assert missing == 1000 and first == int(absent_at.min())
        counts = np.bincount(np.delete(idx, absent_at), minlength=nt)
        rows = rng.choice(nt, 4096, replace=False)
        wanted = {c: _wire_int(0, int(c)).to_bytes(32, "little") for c in set(counts[rows].tolist())}
        assert all(mult[j].tobytes() == wanted[counts[j]] for j in rows)
        assert counts.sum() == n - 1000
        for c in np.unique(counts):  # every row holds the wire form of its count, so sum m is the number of values found
            rows_c = mult[counts == c]
            assert np.array_equal(rows_c, np.broadcast_to(fr.words([_wire_int(0, int(c))])[0], rows_c.shape)), c
    finally:
        h.close()
    n = (1 << 24) + 3
    x = _vectors(0, n, 1, 0x2403)
    s = Sums(gm, 0, n, 1)
    try:
        out, tot = s.run(x)
        nxt = np.concatenate([out[0, 1:], tot[0].reshape(1, 8)])
        assert not out[0, 0].any() and np.array_equal(po.f_vec(fid, po.OP_ADD, out[0], np.ascontiguousarray(x[0])), nxt)
        _, tot2 = s.run(x, where=None)
        assert np.array_equal(tot, tot2)
    finally:
        s.close()
