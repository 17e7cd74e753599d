"""panda_poly_evaluate_lagrange / panda_poly_divide_linear_lagrange / panda_poly_lagrange_plan: KZG openings of polynomials held as
evaluations.  n = 2^log_n, x_i = s w^i, position j of a vector holds e_j = f(x_sigma(j)) (sigma the identity or the bit reversal); the
calls return f(z) and the evaluations of q = (f - f(z)) / (X - z) in the same form, domain and order, exact also where z is a domain point.

Expected values never come from the code under test: random coefficients -> the CPU oracle's ntt (pre-scaled by fr.shift_powers for a
coset, permuted in numpy for the bit-reversed order) gives the input; plain Horner over Python integers gives f(z) and the quotient's
coefficients, and the oracle's ntt of those the expected quotient.  Every comparison is byte for byte.

At 2^20 and above, where a Python loop over n is too slow, the quotient is checked by its COMPLETE characterisation with the oracle's
vector operations:   q_i (x_i - z) = e_i - y for every i,   and   sum_i q_i w^i = 0.
These determine (q, y).  The sum is n s^(n-1) times the coefficient of X^(n-1) of the polynomial of degree < n through the q_i, so it
says "degree < n - 1".  Off the domain every x_i - z is invertible, so the equations give q_i = (e_i - y) / (x_i - z) and the sum becomes
A - y B with B = sum_i w^i / (x_i - z) = -n / (s (u^n - 1)) != 0: one y satisfies it, and that y is f(z) because the true quotient does.
On the domain the equation at x_m = z reads 0 = e_m - y, which fixes y, the others fix q_i for i != m, and the sum, in which q_m has the
coefficient w^m != 0, fixes q_m.  (y is also compared with f(z) from six pow calls.)

Every device buffer carries a guard run behind the batch, which no call may touch; the evaluations must come back unchanged unless the
division is in place."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import field_ref as fr
import oracle as po
import pyref
from gpu_util import GUARD, DeviceBuffer, GuardedBuffers, assert_exported, free_bytes, gm, independent_of_scratch  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

MAX_POINTS = 8  # PANDA_POLY_MAX_POINTS
MAX_LOG = 28
NAT, REV = 0, 1
SYMBOLS = ("panda_poly_evaluate_lagrange", "panda_poly_divide_linear_lagrange", "panda_poly_lagrange_plan")


def _plan(lib, log_n, batch, n_points):
    outs = [C.c_uint(0) for _ in range(4)]
    rc = lib.panda_poly_lagrange_plan(log_n, batch, n_points, *[C.byref(o) for o in outs])
    return (rc,) + tuple(o.value for o in outs)


@functools.lru_cache(maxsize=None)
def _log_tile():
    rc, tile, _, _, _ = _plan(ffi.load(), 10, 1, 1)
    assert rc == 0 and tile >= 2 and tile & (tile - 1) == 0
    return tile.bit_length() - 1


# ------------------------------------------------------------------------------------------------- the reference
@functools.lru_cache(maxsize=None)
def _domain(field, log_n):
    """(omega wire words, omega as a plain integer)"""
    om = po.root_of_unity(po.FR_OF[field], log_n) if log_n else fr.wire_one(field, 1)
    return om, fr.plain(field, om)[0]


@functools.lru_cache(maxsize=None)
def _shift(field, seed):
    """a coset shift as a plain integer; seed 0 is the subgroup itself"""
    return 1 if seed == 0 else fr.random_residues(field, 0x5151 + seed, 1, nonzero=True)[0]


@functools.lru_cache(maxsize=None)
def _perm(log_n):
    """sigma as an index array: position j holds the natural-order element sigma[j]"""
    j = np.arange(1 << log_n, dtype=np.int64)
    r = np.zeros_like(j)
    for b in range(log_n):
        r |= ((j >> b) & 1) << (log_n - 1 - b)
    return r


def _ordered(nat, log_n, order):
    """natural-order vectors (..., n, 8) in the order of the call"""
    return np.ascontiguousarray(nat[..., _perm(log_n), :]) if order == REV else np.ascontiguousarray(nat)


def _sigma_inv(log_n, order, m):
    return int(_perm(log_n)[m]) if order == REV else m  # the bit reversal is its own inverse


def _evaluations(field, log_n, coeff_wire, s):
    """coefficients (batch, n, 8) on the wire -> their evaluations on s w^i in natural order, by the CPU oracle"""
    fid, n = po.FR_OF[field], 1 << log_n
    om, _ = _domain(field, log_n)
    out = []
    for c in coeff_wire:
        c = np.ascontiguousarray(c)
        if s != 1:
            c = po.f_vec(fid, po.OP_MUL, c, fr.shift_powers(field, n, s))
        out.append(po.ntt(fid, c, om, log_n) if log_n else c.copy())
    return np.stack(out)


def _horner(r, c, z):
    """(quotient coefficients, value) of the plain coefficients c by X - z"""
    q, acc = [0] * len(c), 0
    for j in range(len(c) - 1, -1, -1):
        q[j] = acc
        acc = (c[j] + z * acc) % r
    return q, acc


@functools.lru_cache(maxsize=None)
def _rows(field, log_n, batch, seed):
    return tuple(tuple(row) for row in fr.random_rows(field, seed, batch, 1 << log_n))


@functools.lru_cache(maxsize=None)
def _input_nat(field, log_n, batch, seed, shift_seed):
    e = _evaluations(field, log_n, np.stack([fr.wire(field, row) for row in _rows(field, log_n, batch, seed)]), _shift(field, shift_seed))
    e.setflags(write=False)
    return e


def _expected(field, log_n, rows, s, z):
    """(values (batch, 8), quotient evaluations in natural order (batch, n, 8)) at the plain point z"""
    r = fr.modulus(field)
    qs, ys = [], []
    for row in rows:
        q, y = _horner(r, row, z)
        qs.append(fr.wire(field, q))
        ys.append(y)
    return fr.wire(field, ys), _evaluations(field, log_n, np.stack(qs), s)


def _x(field, log_n, s, m):
    _, w = _domain(field, log_n)
    r = fr.modulus(field)
    return s * pow(w, m, r) % r


def _random_point(field, seed):
    return fr.random_residues(field, 0x7A7A + seed, 1)[0]


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, lib = assert_exported(SYMBOLS)
    assert re.search(r"#define\s+PANDA_DOMAIN_NATURAL\s+%du\b" % ffi.DOMAIN_NATURAL, header)
    assert re.search(r"#define\s+PANDA_DOMAIN_BITREV\s+%du\b" % ffi.DOMAIN_BITREV, header)
    assert (ffi.DOMAIN_NATURAL, ffi.DOMAIN_BITREV) == (NAT, REV)
    assert len(lib.panda_poly_evaluate_lagrange.argtypes) == 11 and len(lib.panda_poly_divide_linear_lagrange.argtypes) == 11
    assert lib.panda_poly_evaluate_lagrange.argtypes[2] is C.c_uint and lib.panda_poly_lagrange_plan.argtypes[0] is C.c_uint


def test_bad_arguments_are_refused_before_any_device_call():
    """every shape, pointer, root, shift, point and overlap error returns 1 with the host outputs untouched -- also with no device"""
    lib = ffi.load()
    mem = np.zeros(2 << 20, np.uint8)  # two disjoint 1 MiB host ranges stand in for the device buffers: nothing may dereference them
    base = mem.ctypes.data
    at = lambda off: C.c_void_p(base + off)
    evals, quot = at(0), at(1 << 20)
    stream = ffi.PandaStream()
    out = np.full((4 * MAX_POINTS, 8), 0x5A5A5A5A, np.uint32)
    outp = C.c_void_p(out.ctypes.data)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    for field in range(3):
        r = fr.modulus(field)
        log_n = 4  # 2 vectors of 16 elements are 1024 bytes
        om, w = _domain(field, log_n)
        good = np.stack([fr.wire_one(field, 3 + k) for k in range(MAX_POINTS)])
        shift = fr.wire_one(field, 5)
        at_modulus = np.array(pyref.int_to_limbs(r, 8), np.uint32)
        all_ones = np.full(8, 0xFFFFFFFF, np.uint32)
        zero = np.zeros(8, np.uint32)
        one = fr.wire_one(field, 1)
        om_sq = fr.wire_one(field, w * w % r)

        def ev(f=field, e=evals, ln=log_n, batch=2, o=ptr(om), s=ptr(shift), order=0, pts=ptr(good), k=2, vals=outp):
            return lib.panda_poly_evaluate_lagrange(f, e, ln, batch, o, s, order, pts, k, vals, stream)

        def dv(f=field, e=evals, q=quot, ln=log_n, batch=2, o=ptr(om), s=ptr(shift), order=0, pt=ptr(good), rem=outp):
            return lib.panda_poly_divide_linear_lagrange(f, e, q, ln, batch, o, s, order, pt, rem, stream)

        assert ev(f=3) == 1 and dv(f=3) == 1
        assert ev(ln=MAX_LOG + 1, batch=1) == 1 and dv(ln=MAX_LOG + 1, batch=1) == 1
        assert ev(ln=32) == 1 and dv(ln=32) == 1 and ev(ln=0xFFFFFFFF) == 1 and dv(ln=64) == 1
        assert ev(batch=0) == 1 and dv(batch=0) == 1
        assert ev(batch=(1 << (MAX_LOG - log_n)) + 1) == 1 and dv(batch=(1 << (MAX_LOG - log_n)) + 1) == 1
        assert ev(order=2) == 1 and dv(order=2) == 1 and ev(order=0xFFFFFFFF) == 1
        assert ev(k=0) == 1 and ev(k=MAX_POINTS + 1) == 1
        assert ev(e=None) == 1 and ev(o=None) == 1 and ev(pts=None) == 1 and ev(vals=None) == 1
        assert dv(e=None) == 1 and dv(q=None) == 1 and dv(o=None) == 1 and dv(pt=None) == 1
        for bad in (at_modulus, all_ones):
            assert ev(o=ptr(bad)) == 1 and dv(o=ptr(bad)) == 1
            assert ev(s=ptr(bad)) == 1 and dv(s=ptr(bad)) == 1
            assert dv(pt=ptr(bad)) == 1
            for pos in (0, 1, MAX_POINTS - 1):  # a bad point anywhere in the list
                pts = good.copy()
                pts[pos] = bad
                assert ev(pts=ptr(pts), k=pos + 1) == 1
        assert ev(s=ptr(zero)) == 1 and dv(s=ptr(zero)) == 1
        # omega must be a PRIMITIVE 2^log_n-th root: its square, one and zero are not; the root of another size is not; for log_n == 0
        # only one is
        for bad in (om_sq, one, zero, _domain(field, log_n + 1)[0], _domain(field, log_n - 1)[0]):
            assert ev(o=ptr(bad)) == 1 and dv(o=ptr(bad)) == 1
        assert ev(ln=0, o=ptr(om)) == 1 and dv(ln=0, o=ptr(om)) == 1 and ev(ln=0, o=ptr(zero)) == 1
        assert ev(ln=1, o=ptr(one)) == 1 and dv(ln=1, o=ptr(one)) == 1
        # every way the two ranges can meet without being equal
        assert dv(q=at(1023)) == 1
        assert dv(e=at((1 << 20) + 1023)) == 1
        assert dv(q=at(32)) == 1
        assert dv(e=at(512), q=at(0)) == 1
    assert (out == 0x5A5A5A5A).all(), "a refused call wrote to values / remainders"


def test_lagrange_plan():
    lib = ffi.load()
    for log_n in range(MAX_LOG + 1):
        seen = set()
        for batch in (1, 2, 3, 16, 1 << 10, 1 << 28):
            if batch << log_n > 1 << MAX_LOG:
                assert lib.panda_poly_lagrange_plan(log_n, batch, 1, None, None, None, None) == 1
                continue
            rc, tile, le, ld, inv = _plan(lib, log_n, batch, 1)
            assert rc == 0 and tile >= 2 and tile & (tile - 1) == 0 and le >= 1 and ld >= le and inv >= 1, (log_n, batch)
            seen.add((tile, le, ld, inv))
            for i in range(4):  # every out pointer may be NULL, singly
                outs = [C.c_uint(0xDEAD) for _ in range(4)]
                args = [C.byref(o) if j != i else None for j, o in enumerate(outs)]
                assert lib.panda_poly_lagrange_plan(log_n, batch, MAX_POINTS, *args) == 0
                assert [o.value for j, o in enumerate(outs) if j != i] == [v for j, v in enumerate((tile, le, ld, inv)) if j != i]
        assert len(seen) == 1, "no figure depends on the batch"
    for log_n, batch, k in ((MAX_LOG + 1, 1, 1), (32, 1, 1), (0xFFFFFFFF, 1, 1), (0, 0, 1), (MAX_LOG, 2, 1), (0, (1 << MAX_LOG) + 1, 1), (4, 1, 0), (4, 1, MAX_POINTS + 1)):
        assert lib.panda_poly_lagrange_plan(log_n, batch, k, None, None, None, None) == 1, (log_n, batch, k)


# ------------------------------------------------------------------------------------------------- on the device
class Harness(GuardedBuffers):
    """the evaluation and the quotient buffer, each with a guard run behind the batch"""

    def __init__(self, gm, field, log_n, batch, s=1, order=NAT):
        super().__init__()
        self.lib, self.gm, self.field, self.log_n, self.batch, self.order = ffi.load(), gm, field, log_n, batch, order
        self.n = 1 << log_n
        self.bytes = batch * self.n * 32
        self.e, self.q = self.buffer(nbytes=self.bytes), self.buffer(nbytes=self.bytes)
        self.stream = gm.exec_stream.raw
        self.omega = _domain(field, log_n)[0]
        self.shift = None if s == 1 else fr.wire_one(field, s)

    def _dom(self):
        return C.c_void_p(self.omega.ctypes.data), None if self.shift is None else C.c_void_p(self.shift.ctypes.data)

    def load(self, evals):
        assert np.asarray(evals).nbytes == self.bytes
        self.fill(self.e, evals)
        self.fill(self.q)

    def divide(self, evals, z, in_place=False, remainders=True):
        """one division at the plain point z -> (quotients (batch, n, 8), remainders (batch, 8) or None); checks guards and the input"""
        self.load(evals)
        zw = fr.wire_one(self.field, z)
        rem = np.full((self.batch, 8), 0x77777777, np.uint32) if remainders else None
        dst = self.e if in_place else self.q
        om, sh = self._dom()
        ffi.check(self.lib.panda_poly_divide_linear_lagrange(self.field, self.e.ptr, dst.ptr, self.log_n, self.batch, om, sh, self.order, C.c_void_p(zw.ctypes.data),
                                                             C.c_void_p(rem.ctypes.data) if remainders else None, self.stream), "divide")
        assert self.guard_intact(self.e) and self.guard_intact(self.q), "bytes behind the batch were written"
        if in_place:
            assert self.untouched(self.q), "the other buffer was written by a division in place"
        else:
            assert self.intact(self.e), "d_evals was written"
        return self.get(dst).reshape(self.batch, self.n, 8), rem

    def evaluate(self, evals, zs):
        self.load(evals)
        pts = np.stack([fr.wire_one(self.field, z) for z in zs])
        vals = np.full((self.batch, len(pts), 8), 0x77777777, np.uint32)
        om, sh = self._dom()
        ffi.check(self.lib.panda_poly_evaluate_lagrange(self.field, self.e.ptr, self.log_n, self.batch, om, sh, self.order, C.c_void_p(pts.ctypes.data), len(pts),
                                                        C.c_void_p(vals.ctypes.data), self.stream), "evaluate")
        assert self.intact(self.e), "d_evals or the bytes behind the batch were written"
        assert self.untouched(self.q), "an evaluation wrote to an unrelated buffer"
        return vals


def _check_division(h, nat, rows, s, z, all_forms=False):
    """the division at z against Horner; all_forms: in place and without remainders as well, all with one quotient"""
    want_y, want_q = _expected(h.field, h.log_n, rows, s, z)
    want_q = _ordered(want_q, h.log_n, h.order)
    evals = _ordered(nat, h.log_n, h.order)
    q, rem = h.divide(evals, z)
    assert np.array_equal(rem, want_y), (h.field, h.log_n, h.order, z)
    assert np.array_equal(q, want_q), (h.field, h.log_n, h.order, z)
    if all_forms:
        for in_place, remainders in ((True, True), (False, False), (True, False)):
            q2, rem2 = h.divide(evals, z, in_place=in_place, remainders=remainders)
            assert np.array_equal(q2, q) and (rem2 is None or np.array_equal(rem2, rem)), (in_place, remainders)
    return want_y


def _check_evaluation(h, nat, rows, zs):
    r = fr.modulus(h.field)
    vals = h.evaluate(_ordered(nat, h.log_n, h.order), zs)
    for p, row in enumerate(rows):
        want = fr.wire(h.field, [_horner(r, row, z)[1] for z in zs])
        assert np.array_equal(vals[p], want), (h.field, h.log_n, h.order, p)
    return vals


def _small_sizes():
    lt = _log_tile()
    return sorted({0, 1, 2, 3, 6, lt - 1, lt, lt + 1, lt + 2})


@pytest.mark.gpu
@pytest.mark.parametrize("shift_seed", [0, 1])
@pytest.mark.parametrize("order", [NAT, REV])
def test_small_sizes_vs_python_integers(gm, order, shift_seed):
    """below one thread's run, one thread, a few lanes, one wave, a ragged tile, one tile and the first multi-tile sizes (the sizes come
    from the plan, so they are walked inside the test); batch 1 and 3; division in all four forms, evaluation at 1, 2 and 8 points"""
    s = _shift(0, shift_seed)
    for log_n in _small_sizes():
        for batch in (1, 3):
            rows = _rows(0, log_n, batch, 0xA000 + log_n)
            nat = _input_nat(0, log_n, batch, 0xA000 + log_n, shift_seed)
            zs = [_random_point(0, 16 * log_n + k) for k in range(MAX_POINTS)]
            h = Harness(gm, 0, log_n, batch, s, order)
            try:
                want_y = _check_division(h, nat, rows, s, zs[0], all_forms=True)
                for k in (1, 2, 8):
                    vals = _check_evaluation(h, nat, rows, zs[:k])
                    assert np.array_equal(vals[:, 0], want_y)
            finally:
                h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", [NAT, REV])
def test_points_on_the_domain(gm, order):
    """z = x_m: the value is the stored element, and the quotient -- q_m included -- the transform of the Horner quotient"""
    lt = _log_tile()
    r = fr.modulus(0)
    for shift_seed in (0, 2):
        s = _shift(0, shift_seed)
        for log_n in (1, 3, lt + 1):
            n, batch = 1 << log_n, 2
            ms = {0, 1, n // 2, n - 1}
            if log_n == lt + 1:  # the last position of tile 0 and the first of tile 1, whichever exponent they hold
                ms |= {int(_perm(log_n)[j]) if order == REV else j for j in ((1 << lt) - 1, 1 << lt)}
            rows = _rows(0, log_n, batch, 0xB000 + log_n)
            nat = _input_nat(0, log_n, batch, 0xB000 + log_n, shift_seed)
            evals = _ordered(nat, log_n, order)
            h = Harness(gm, 0, log_n, batch, s, order)
            try:
                for m in sorted(ms):
                    want_y = _check_division(h, nat, rows, s, _x(0, log_n, s, m), all_forms=(m == 1))
                    assert np.array_equal(want_y, evals[:, _sigma_inv(log_n, order, m)]), "f(x_m) is the stored element"
                # on and off the domain in one list, one point twice
                zs = [_x(0, log_n, s, n - 1), _random_point(0, 900), _x(0, log_n, s, 0), _random_point(0, 900), _x(0, log_n, s, n - 1), _random_point(0, 901)]
                vals = _check_evaluation(h, nat, rows, zs)
                assert np.array_equal(vals[:, 0], evals[:, _sigma_inv(log_n, order, n - 1)])
                # zero, -1 and a point of the other coset of the domain twice the size (u^n = -1)
                w2 = fr.plain(0, po.root_of_unity(po.F_BN254_FR, log_n + 1))[0]
                for z in (0, r - 1, s * w2 % r):
                    if pow(z * pow(s, -1, r) % r, n, r) == 1:
                        continue  # r - 1 = s w^(n/2) lies on the subgroup; the domain points are covered above
                    _check_division(h, nat, rows, s, z)
                _check_evaluation(h, nat, rows, [0, r - 1, s * w2 % r])
            finally:
                h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", [NAT, REV])
@pytest.mark.parametrize("case", ["zero", "allm1", "top", "delta"])
def test_edge_values(gm, case, order):
    log_n = _log_tile()
    n, r, s = 1 << log_n, fr.modulus(0), _shift(0, 3)
    m = 5 * n // 8 + 3
    z = _random_point(0, 77)
    if case == "zero":
        row = [0] * n
    elif case == "allm1":
        row = [r - 1] + [0] * (n - 1)
    elif case == "top":
        row = [0] * (n - 1) + [1]
    else:  # v L_m(X): c_j = v / (n x_m^j); the point is x_m
        v, xinv = 0x1234567, pow(_x(0, log_n, s, m), -1, r)
        row = [v * pow(n, -1, r) * pow(xinv, j, r) % r for j in range(n)]
        z = _x(0, log_n, s, m)
    rows = (tuple(row), tuple(row))
    nat = _evaluations(0, log_n, np.stack([fr.wire(0, row)] * 2), s)
    if case == "allm1":
        assert np.array_equal(nat[0], np.broadcast_to(fr.wire_one(0, r - 1), (n, 8)))
    if case == "delta":
        want = np.zeros((n, 8), np.uint32)
        want[m] = fr.wire_one(0, 0x1234567)
        assert np.array_equal(nat[0], want), "the input is zero except at x_m"
    h = Harness(gm, 0, log_n, 2, s, order)
    try:
        want_y = _check_division(h, nat, rows, s, z, all_forms=True)
        vals = _check_evaluation(h, nat, rows, [z, _x(0, log_n, s, m), 0])
        assert np.array_equal(vals[:, 0], want_y)
        if case in ("zero", "allm1"):
            q, rem = h.divide(_ordered(nat, log_n, order), z)
            assert not q.any() and np.array_equal(rem[0], fr.wire_one(0, row[0]))
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
@pytest.mark.parametrize("order", [NAT, REV])
def test_other_fields(gm, field, order):
    lt = _log_tile()
    s = _shift(field, 4)
    for log_n in (lt, lt + 1):
        n, batch = 1 << log_n, 2
        rows = _rows(field, log_n, batch, 0xC000 + log_n)
        nat = _input_nat(field, log_n, batch, 0xC000 + log_n, 4)
        h = Harness(gm, field, log_n, batch, s, order)
        try:
            off, on = _random_point(field, 5), _x(field, log_n, s, n - 3)
            _check_division(h, nat, rows, s, off, all_forms=True)
            _check_division(h, nat, rows, s, on, all_forms=True)
            _check_evaluation(h, nat, rows, [off, on])
        finally:
            h.close()


SPARSE_DEGREES = lambda n: (0, 1, 777, n // 2 + 1, n - 2, n - 1)


@functools.lru_cache(maxsize=None)
def _domain_vectors(log_n, s):
    """(x_i, w^i) of BN254 in natural order, by doubling with the oracle's vector product: w^(2^k + i) = w^i w^(2^k)"""
    fid, n, r = po.F_BN254_FR, 1 << log_n, fr.modulus(0)
    wi = np.zeros((n, 8), np.uint32)
    wi[0] = fr.wire_one(0, 1)
    for k in range(log_n):
        half = 1 << k
        step = np.ascontiguousarray(np.broadcast_to(fr.wire_one(0, pow(_domain(0, log_n)[1], half, r)), (half, 8)))
        wi[half:2 * half] = po.f_vec(fid, po.OP_MUL, np.ascontiguousarray(wi[:half]), step)
    xi = po.f_vec(fid, po.OP_MUL, wi, np.ascontiguousarray(np.broadcast_to(fr.wire_one(0, s), (n, 8))))
    wi.setflags(write=False)
    xi.setflags(write=False)
    return xi, wi


@functools.lru_cache(maxsize=None)
def _sparse_case(log_n, batch, s):
    """six monomials per vector -> (coefficient values per vector, evaluations in natural order, x_i, w^i), all by the oracle's ntt"""
    fid, n, r = po.F_BN254_FR, 1 << log_n, fr.modulus(0)
    om, _ = _domain(0, log_n)
    degs = SPARSE_DEGREES(n)
    cs, nat = [], []
    for p in range(batch):
        vals = fr.random_residues(0, 0xD000 + p, len(degs), nonzero=True)
        c = np.zeros((n, 8), np.uint32)
        for d, v in zip(degs, vals):
            c[d] = fr.wire_one(0, v * pow(s, d, r) % r)  # the coset's pre-scaling, on six elements
        cs.append(vals)
        nat.append(po.ntt(fid, c, om, log_n))
    xi, wi = _domain_vectors(log_n, s)
    for a in nat:
        a.setflags(write=False)
    return cs, np.stack(nat), xi, wi


def _is_quotient(log_n, xi, e_nat, q_nat, y_wire, z):
    """the complete characterisation (module docstring) on natural-order vectors"""
    fid, n = po.F_BN254_FR, 1 << log_n
    full = lambda v: np.ascontiguousarray(np.broadcast_to(v, (n, 8)))
    lhs = po.f_vec(fid, po.OP_MUL, q_nat, po.f_vec(fid, po.OP_SUB, xi, full(fr.wire_one(0, z))))
    if not np.array_equal(lhs, po.f_vec(fid, po.OP_SUB, np.ascontiguousarray(e_nat), full(y_wire))):
        return False
    return not po.ntt_eval_at(fid, q_nat, _domain(0, log_n)[0], log_n, 1).any()  # sum_i q_i w^i


def _large_case(gm, log_n, batch, order, zs):
    s, r = _shift(0, 6), fr.modulus(0)
    n = 1 << log_n
    cs, nat, xi, _ = _sparse_case(log_n, batch, s)
    inv = np.argsort(_perm(log_n)) if order == REV else None
    h = Harness(gm, 0, log_n, batch, s, order)
    try:
        evals = _ordered(nat, log_n, order)
        for z in zs:
            want = fr.wire(0, [sum(v * pow(z, d, r) for d, v in zip(SPARSE_DEGREES(n), vals)) % r for vals in cs])
            q, rem = h.divide(evals, z)
            assert np.array_equal(rem, want), (log_n, order, z)
            for p in range(batch):
                q_nat = np.ascontiguousarray(q[p][inv]) if order == REV else q[p]
                assert _is_quotient(log_n, xi, nat[p], q_nat, rem[p], z), (log_n, order, p)
            assert np.array_equal(h.evaluate(evals, [z])[:, 0], want)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", [NAT, REV])
def test_2_20_by_the_characterisation(gm, order):
    """no Python loop over n: six monomials, the value from six pow calls, the quotient by its complete characterisation; one point off
    the domain and one on it"""
    log_n = 20
    _large_case(gm, log_n, 2, order, [_random_point(0, 2020), _x(0, log_n, _shift(0, 6), (1 << 19) + 12345)])


def _second_level_log_n():
    """the smallest size at which the one-workgroup kernels take a second step over the per-tile partials: they combine tile / 2 of them
    per step (the header's word on panda_poly_lagrange_plan), so tile x tile / 2 positions are one full step"""
    return min(2 * _log_tile(), 22)  # the size is capped at 2^22: a larger tile would leave the second step to the bench tool


@pytest.mark.gpu
@pytest.mark.parametrize("on_domain", [False, True])
@pytest.mark.parametrize("order", [NAT, REV])
def test_second_step_over_the_tile_partials(gm, order, on_domain):
    """Two full steps of the one-workgroup kernels (2^22 for a tile of 2^11; the issue caps the size there).  No transform of that size:
    the input is sparse in EVALUATION form -- zero but at the first and last position, the two positions either side of the step
    boundary and two others -- the value comes from the barycentric sum over those six in Python integers (off the domain) or is the
    stored element (on it), and the quotient is checked by the complete characterisation of the module docstring."""
    log_n = _second_level_log_n()
    n, r, s = 1 << log_n, fr.modulus(0), _shift(0, 9)
    _, w = _domain(0, log_n)
    xi, _ = _domain_vectors(log_n, s)
    boundary = n // 2  # tile x tile / 2 positions: the first position of the second step
    positions = (0, 12345, boundary - 1, boundary, boundary + (n >> 3) + 7, n - 1)
    idx = [int(_perm(log_n)[j]) if order == REV else j for j in positions]  # their natural indices
    vals = fr.random_residues(0, 0xE222 + order, len(idx), nonzero=True)
    e_nat = np.zeros((n, 8), np.uint32)
    for i, v in zip(idx, vals):
        e_nat[i] = fr.wire_one(0, v)
    if on_domain:
        z, y = _x(0, log_n, s, idx[3]), vals[3]
    else:
        z = _random_point(0, 2222)
        u = z * pow(s, -1, r) % r
        y = (pow(u, n, r) - 1) * pow(n, -1, r) * sum(v * pow(w, i, r) * pow((u - pow(w, i, r)) % r, -1, r) for i, v in zip(idx, vals)) % r
    inv = np.argsort(_perm(log_n)) if order == REV else None
    h = Harness(gm, 0, log_n, 1, s, order)
    try:
        evals = _ordered(e_nat[None], log_n, order)
        q, rem = h.divide(evals, z)
        assert np.array_equal(rem[0], fr.wire_one(0, y))
        q_nat = np.ascontiguousarray(q[0][inv]) if order == REV else q[0]
        assert _is_quotient(log_n, xi, e_nat, q_nat, rem[0], z)
        assert np.array_equal(h.evaluate(evals, [z])[0, 0], rem[0])
    finally:
        h.close()


@pytest.mark.gpu
def test_more_vectors_than_a_grid_dimension_or_a_slice_holds(gm):
    """batch above 65535 (no grid dimension but the first takes that) and above what the scratch of one slice covers: 2^18 + 3 vectors at
    eight points, 2^21 + 3 vectors for a division, of two elements each; three distinct vectors repeated, so the reference is three
    Horner runs"""
    log_n, order = 1, REV
    s, r = _shift(0, 10), fr.modulus(0)
    rows = _rows(0, log_n, 3, 0xF500)
    base = _ordered(_input_nat(0, log_n, 3, 0xF500, 10), log_n, order)
    zs = [_random_point(0, 81 + k) for k in range(6)] + [_x(0, log_n, s, 1), _random_point(0, 81)]

    def repeat(a, batch):
        return np.ascontiguousarray(np.concatenate([a] * (batch // 3 + 1))[:batch])

    batch = (1 << 18) + 3
    h = Harness(gm, 0, log_n, batch, s, order)
    try:
        want = np.stack([fr.wire(0, [_horner(r, row, z)[1] for z in zs]) for row in rows])
        assert np.array_equal(h.evaluate(repeat(base, batch), zs), repeat(want, batch))
    finally:
        h.close()
    batch = (1 << 21) + 3
    h = Harness(gm, 0, log_n, batch, s, order)
    try:
        for z in (zs[0], zs[6]):
            want_y, want_q = _expected(0, log_n, rows, s, z)
            q, rem = h.divide(repeat(base, batch), z, in_place=(z == zs[6]))
            assert np.array_equal(rem, repeat(want_y, batch))
            assert np.array_equal(q, repeat(_ordered(want_q, log_n, order), batch))
    finally:
        h.close()


@pytest.mark.gpu
def test_agrees_with_the_coefficient_route(gm):
    """evaluations -> the library's inverse transform -> panda_poly_evaluate: the parent commit's route gives the same bytes"""
    log_n, batch = _log_tile() + 1, 2
    nat = _input_nat(0, log_n, batch, 0xE000, 0)
    zs = [_random_point(0, 31), _x(0, log_n, 1, 77), _random_point(0, 32)]
    pts = np.stack([fr.wire_one(0, z) for z in zs])
    h = Harness(gm, 0, log_n, batch)
    try:
        vals = h.evaluate(nat, zs)
    finally:
        h.close()
    coeffs = []
    for p in range(batch):
        buf = np.array(nat[p])
        pgm.panda_intt_bn254_gpu(gm, buf, _domain(0, log_n)[0], log_n)
        coeffs.append(buf)
    assert np.array_equal(np.stack(coeffs), np.stack([fr.wire(0, row) for row in _rows(0, log_n, batch, 0xE000)]))
    assert np.array_equal(pgm.panda_poly_gpu_evaluate(gm, coeffs, pts), vals)


@pytest.mark.gpu
def test_results_do_not_depend_on_the_scratch(gm):
    """one evaluation (4 points, one on the domain) and one division in place, each on scratch filled with every pattern, and each again
    behind a call of the same feature on other inputs at twice the size"""
    log_n, batch, order = _log_tile() + 1, 2, REV
    s = _shift(0, 7)
    rows, nat = _rows(0, log_n, batch, 0xF000), _input_nat(0, log_n, batch, 0xF000, 7)
    zs = [_random_point(0, 41), _x(0, log_n, s, 5), _random_point(0, 42), _random_point(0, 43)]
    big_nat = _input_nat(0, log_n + 1, batch, 0xF001, 7)
    h, big = Harness(gm, 0, log_n, batch, s, order), Harness(gm, 0, log_n + 1, batch, s, order)
    try:
        evals = _ordered(nat, log_n, order)
        r = fr.modulus(0)
        want_vals = np.stack([fr.wire(0, [_horner(r, row, z)[1] for z in zs]) for row in rows])
        for z in (zs[0], zs[1]):
            want_y, want_q = _expected(0, log_n, rows, s, z)
            want_q = _ordered(want_q, log_n, order)

            def check_div(out, want_q=want_q, want_y=want_y):
                assert np.array_equal(out[0], want_q) and np.array_equal(out[1], want_y)

            first = independent_of_scratch(lambda z=z: h.divide(evals, z, in_place=True), check_div, exact=True)
            big.divide(_ordered(big_nat, log_n + 1, order), _random_point(0, 44), in_place=True)
            again = h.divide(evals, z, in_place=True)
            assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])

        def check_eval(out):
            assert np.array_equal(out, want_vals)

        first = independent_of_scratch(lambda: h.evaluate(evals, zs), check_eval, exact=True)
        big.evaluate(_ordered(big_nat, log_n + 1, order), [_random_point(0, 45 + k) for k in range(4)])
        assert np.array_equal(h.evaluate(evals, zs), first)
    finally:
        h.close()
        big.close()


@pytest.mark.gpu
def test_scratch_is_reused_and_released(gm):
    log_n, batch = _log_tile() + 2, 3
    nat = _input_nat(0, log_n, batch, 0xF100, 0)
    z = _random_point(0, 51)
    h = Harness(gm, 0, log_n, batch)
    try:
        h.divide(nat, z)  # whatever the runtime keeps from a kernel's first launch is there before the baseline is read
        h.evaluate(nat, [z])
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        before = free_bytes(h.lib)
        q1, r1 = h.divide(nat, z)
        first = free_bytes(h.lib)
        q2, r2 = h.divide(nat, z)
        assert free_bytes(h.lib) == first, "a repeated identical call allocated"
        v = h.evaluate(nat, [z])  # needs no more scratch than the division
        assert free_bytes(h.lib) == first
        assert np.array_equal(q1, q2) and np.array_equal(r1, r2) and np.array_equal(v[:, 0], r1)
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        assert free_bytes(h.lib) == before, "panda_ntt_tear_down releases the scratch"
    finally:
        h.close()


@pytest.mark.gpu
def test_short_device_buffers_are_refused(gm):
    log_n, batch = _log_tile() + 1, 3
    rows, nat = _rows(0, log_n, batch, 0xF200), _input_nat(0, log_n, batch, 0xF200, 0)
    z = _random_point(0, 61)
    h = Harness(gm, 0, log_n, batch)
    short = DeviceBuffer(h.bytes - 32)  # one element short
    try:
        h.load(nat)
        ffi.check(h.lib.panda_memset(short.ptr, GUARD, h.bytes - 32), "memset")
        out = np.full((batch, 8), 0x77777777, np.uint32)
        zw = fr.wire_one(0, z)
        zp, op = C.c_void_p(zw.ctypes.data), C.c_void_p(out.ctypes.data)
        om, sh = h._dom()
        div = lambda e, q: h.lib.panda_poly_divide_linear_lagrange(0, e, q, log_n, batch, om, sh, NAT, zp, op, h.stream)
        assert div(short.ptr, h.q.ptr) == 1 and div(h.e.ptr, short.ptr) == 1 and div(short.ptr, short.ptr) == 1
        assert h.lib.panda_poly_evaluate_lagrange(0, short.ptr, log_n, batch, om, sh, NAT, zp, 1, op, h.stream) == 1
        assert (out == 0x77777777).all()
        assert (short.to_host(np.uint8) == GUARD).all() and h.untouched(h.q) and h.intact(h.e), "a refused call wrote to a buffer"
        _check_division(h, nat, rows, 1, z)
    finally:
        short.free()
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [0, 1, 2])
def test_gpu_manager_helpers(gm, field):
    log_n, batch, order = 7, 3, REV
    s = _shift(field, 8)
    rows, nat = _rows(field, log_n, batch, 0xF300), _input_nat(field, log_n, batch, 0xF300, 8)
    evals = [np.array(v) for v in _ordered(nat, log_n, order)]
    keep = [v.copy() for v in evals]
    om, sw = _domain(field, log_n)[0], fr.wire_one(field, s)
    zs = [_random_point(field, 71), _x(field, log_n, s, 9)]
    pts = np.stack([fr.wire_one(field, z) for z in zs])
    vals = pgm.panda_poly_gpu_evaluate_lagrange(gm, evals, om, pts, field=field, shift=sw, order=ffi.DOMAIN_BITREV)
    assert vals.shape == (batch, 2, 8) and vals.dtype == np.uint32
    for k, z in enumerate(zs):
        want_y, want_q = _expected(field, log_n, rows, s, z)
        quotients, rems = pgm.panda_poly_gpu_divide_lagrange(gm, evals, om, pts[k], field=field, shift=sw, order=ffi.DOMAIN_BITREV)
        assert len(quotients) == batch and rems.shape == (batch, 8)
        assert np.array_equal(rems, want_y) and np.array_equal(vals[:, k], want_y)
        assert np.array_equal(np.stack(quotients), _ordered(want_q, log_n, order))
    assert all(np.array_equal(a, b) for a, b in zip(evals, keep)), "a helper changed its input"
    # the subgroup in natural order: the defaults
    nat1 = _input_nat(field, log_n, batch, 0xF300, 0)
    vals = pgm.panda_poly_gpu_evaluate_lagrange(gm, [np.array(v) for v in nat1], om, pts[:1], field=field)
    assert np.array_equal(vals[:, 0], _expected(field, log_n, rows, 1, zs[0])[0])
    assert pgm.panda_poly_gpu_evaluate_lagrange(gm, [], om, pts).shape == (0, 2, 8)
    q0, r0 = pgm.panda_poly_gpu_divide_lagrange(gm, [], om, pts[0])
    assert q0 == [] and r0.shape == (0, 8)
