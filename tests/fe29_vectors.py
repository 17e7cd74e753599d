"""Operands at the edges of the fe29 bounds contract (panda_amd/csrc/fe29.h) for the op table of panda_amd/csrc/fe29_debug_ops.h, the
checks a result of that table must pass, and a model of the column schedule of the products.

Elements are internal-form limbs: N u32 words of 29 bits each (the top one wider), 2 N for Fq2; the value x of the limbs stands for
the field element x / R, R = 2^(29 N).  Every vector is validated against the contract as it is built (`make_case`), so a bad vector
fails an assert here rather than an assert inside an FE29_CHECK build.  The column model (`mont_model`, `shoup_model`) replays the
product-scanning schedule in 64-bit halves: it yields each product's output limbs and the largest column accumulator it reaches,
which must stay below 2^64 and -- for the set as a whole -- goes beyond what canonical operands (fe_from_wire: tight, below 2p) can
produce."""
import math
import random

import numpy as np

import pyref

W = 29
MASK = (1 << W) - 1
TIGHT = (1 << W) - 1            # limbs 0..N-2 of a product's output
LOOSE = (1 << W) + 8            # fe_norm / fe_sub / fe_add
RAW = (1 << 30) + 16            # fe_add_nr of two loose values (fe_sub_raw_bias<.., 3> takes up to this)
RAW31 = (1 << 31) + (1 << 24)   # fe_sub_raw / fe_neg_raw outputs stay below this
SHOUP = 3 * (1 << 30) + 64      # fe_mul_shoup's x stays below this
MUL_A, MUL_B = 1518500250, 1 << 30  # fe_mul: limb(a) < 2^30.5, limb(b) < 2^30

OPS = dict(MUL=0, SQR=1, MUL_ADD=2, SUB_RAW2_MUL=3, SUB_RAW8_MUL=4, MUL_ADD_NEG_RAW=5, SHOUP=6, SHOUP_UNIFORM=7, BFLY2=8, BFLY3=9,
           SHOUP_PREPARE=10, REDUCE_MAD=11, REDUCE_SMALL=12, INV=13, EXT2_C0=14)
OP_NAMES = {v: k for k, v in OPS.items()}
BASE_FIELDS = {0: (pyref.CURVES[0].p, 9), 1: (pyref.CURVES[0].r, 9), 2: (pyref.CURVES[1].p, 14), 3: (pyref.CURVES[1].r, 9),
               4: (pyref.CURVES[2].p, 14), 5: (pyref.CURVES[2].r, 9)}
EXT2_FIELDS = {6: (0, -1), 7: (4, -1), 8: (2, -5)}  # Fq2 over BN254 / BLS12-381 / BLS12-377 Fq: (base field id, beta = u^2)
FIELD_NAMES = {0: "BN254 Fq", 1: "BN254 Fr", 2: "BLS12-377 Fq", 3: "BLS12-377 Fr", 4: "BLS12-381 Fq", 5: "BLS12-381 Fr",
               6: "BN254 Fq2", 7: "BLS12-381 Fq2", 8: "BLS12-377 Fq2"}


class Field:
    def __init__(self, fid):
        self.fid = fid
        self.p, self.N = BASE_FIELDS[fid]
        self.R = 1 << (W * self.N)
        self.Rinv = pow(self.R, -1, self.p)
        self.INV = (-pow(self.p, -1, 1 << W)) % (1 << W)
        self.P = limbs(self.p, self.N)
        self.PNEG = limbs(self.R - self.p, self.N)
        self.margin = 1 if self.P[-1] >= 16 else 6  # SubMargin
        self.top_shift = W * (self.N - 1)

    def keff(self, k):
        while (k * self.p) >> self.top_shift < 4:
            k += 1
        return k

    def kp_biased(self, k):
        """KP[k] of fe29_params.h: KEFF[k] p with every limb below the top raised by 4 2^29"""
        c = limbs(self.keff(k) * self.p, self.N)
        return [c[0] + (4 << W)] + [x + (4 << W) - 4 for x in c[1:-1]] + [c[-1] - 4]

    def kp_bias(self, k, u):
        """fe_kp_bias<F, k, u> (u = 2: fe_kp30): the same value with the bias lowered to u 2^29"""
        kp, s = self.kp_biased(k), 4 - u
        return [kp[0] - (s << W)] + [x - (s << W) + s for x in kp[1:-1]] + [kp[-1] + s]


def limbs(v, n):
    return [(v >> (W * i)) & MASK for i in range(n - 1)] + [v >> (W * (n - 1))]


def base_of(fid):
    return Field(EXT2_FIELDS[fid][0] if fid in EXT2_FIELDS else fid)


def supported(fid, op):
    """mirror of fe29_debug_supported"""
    if fid in EXT2_FIELDS:
        return op in (OPS["MUL"], OPS["SQR"], OPS["MUL_ADD"], OPS["INV"], OPS["EXT2_C0"])
    F = Field(fid)
    if op in (OPS["MUL"], OPS["SQR"], OPS["MUL_ADD"], OPS["INV"], OPS["SHOUP_PREPARE"], OPS["REDUCE_SMALL"]):
        return True
    if op in (OPS["SUB_RAW2_MUL"], OPS["SUB_RAW8_MUL"], OPS["MUL_ADD_NEG_RAW"], OPS["SHOUP"], OPS["SHOUP_UNIFORM"], OPS["BFLY2"], OPS["BFLY3"]):
        return F.N <= 9
    if op == OPS["REDUCE_MAD"]:
        return F.P[-1] >= (1 << 16)
    return False


def cases():
    return [(fid, op) for fid in range(9) for op in range(len(OPS)) if supported(fid, op)]


def out_width(fid, op):
    N = base_of(fid).N
    return 2 * N if (fid in EXT2_FIELDS or op == OPS["SHOUP_PREPARE"]) else N


# ------------------------------------------------------------------------------------------------------------ limb arrays
def to_array(rows, n_limbs):
    a = np.array(rows, dtype=np.uint64).reshape(len(rows), n_limbs)
    assert (a < (1 << 32)).all()
    return a.astype(np.uint32)


def values(arr):
    """Python-int value of every row of an (n, N) limb array"""
    wts = np.array([1 << (W * j) for j in range(arr.shape[1])], dtype=object)
    return list((arr.astype(np.uint64).astype(object) * wts).sum(axis=1))


def in_class(rng, v, N, lim, full=False):
    """v in N limbs whose low N-1 limbs are pushed as close to lim (inclusive) as the value allows, by borrowing from the limb above;
    rng picks how far (none / part / all the way), full: all the way"""
    l = limbs(v, N)
    mode = 2 if full else rng.randrange(3)
    for j in range(N - 1, 0, -1):
        room = (lim - l[j - 1]) >> W
        t = min(room, l[j]) if mode == 2 else (rng.randint(0, min(room, l[j])) if mode == 1 else 0)
        l[j] -= t
        l[j - 1] += t << W
    return l


def at_top(N, lim, vmax):
    """the largest value below vmax whose low limbs are all exactly lim, or None"""
    low = sum(lim << (W * j) for j in range(N - 1))
    if vmax <= low:
        return None
    top = (vmax - 1 - low) >> (W * (N - 1))
    return [lim] * (N - 1) + [top]


# ------------------------------------------------------------------------------------------------------------ column model
_M32 = np.uint64(0xFFFFFFFF)


class _Acc:
    """a column accumulator as (hi, lo) uint64 halves, value hi 2^32 + lo; exact while hi < 2^61"""

    def __init__(self, n):
        self.hi = np.zeros(n, np.uint64)
        self.lo = np.zeros(n, np.uint64)
        self.peak = np.zeros(n, np.uint64)
        self.ok = np.ones(n, bool)

    def add(self, x, y):  # x, y: (n, cnt) uint64 below 2^32, or y a (cnt,) constant row
        if x.shape[1] == 0:
            return
        p = x * y
        self.lo += (p & _M32).sum(axis=1, dtype=np.uint64)
        self.hi += (p >> np.uint64(32)).sum(axis=1, dtype=np.uint64)

    def end_column(self):
        self.hi += self.lo >> np.uint64(32)
        self.lo &= _M32
        self.ok &= self.hi < (np.uint64(1) << np.uint64(32))
        self.peak = np.maximum(self.peak, np.where(self.ok, (self.hi << np.uint64(32)) | self.lo, self.peak))

    def low29(self):
        return self.lo & np.uint64(MASK)

    def shift(self):
        v = (self.hi << np.uint64(3)) | (self.lo >> np.uint64(W))
        self.hi, self.lo = v >> np.uint64(32), v & _M32


def mont_model(F, pairs):
    """fe_mul (one pair) / fe_mul_add (two pairs): (output limbs, largest column accumulator per element, every column below 2^64)"""
    N = F.N
    n = pairs[0][0].shape[0]
    ps = [(x.astype(np.uint64), y.astype(np.uint64)) for x, y in pairs]
    P = np.array(F.P, np.uint64)
    m = np.zeros((n, N), np.uint64)
    out = np.zeros((n, N), np.uint64)
    acc = _Acc(n)
    for k in range(2 * N - 1):
        ix = np.arange(max(0, k - N + 1), min(k, N - 1) + 1)
        for x, y in ps:
            acc.add(x[:, ix], y[:, k - ix])
        if k < N:
            im = np.arange(0, k)
            acc.add(m[:, im], P[k - im])
            m[:, k] = (acc.low29() * np.uint64(F.INV)) & np.uint64(MASK)
            acc.add(m[:, k:k + 1], P[0:1])
        else:
            acc.add(m[:, ix], P[k - ix])
        acc.end_column()
        if k >= N:
            out[:, k - N] = acc.low29()
        acc.shift()
    out[:, N - 1] = acc.lo  # (u32) acc: the shifted accumulator is below 2^35
    return out, acc.peak, acc.ok, m


def shoup_model(F, x, w, wq):
    """fe_mul_shoup: (output limbs, largest column accumulator, every column below 2^64)"""
    N = F.N
    n = x.shape[0]
    x, w, wq = (a.astype(np.uint64) for a in (x, w, wq))
    PN = np.array(F.PNEG, np.uint64)
    q = np.zeros((n, N), np.uint64)
    out = np.zeros((n, N), np.uint64)
    acc = _Acc(n)
    for c in range(N - 2, 2 * N - 1):
        ix = np.arange(0 if c < N else c - N + 1, (c if c < N else N - 1) + 1)
        acc.add(x[:, ix], wq[:, c - ix])
        acc.end_column()
        if c >= N:
            q[:, c - N] = acc.low29()
        acc.shift()
    q[:, N - 1] = acc.lo & np.uint64(MASK)
    hi_peak, ok = acc.peak, acc.ok
    acc = _Acc(n)
    for c in range(N):
        ix = np.arange(0, c + 1)
        acc.add(x[:, ix], w[:, c - ix])
        acc.add(q[:, ix], PN[c - ix])
        acc.end_column()
        out[:, c] = acc.low29()
        acc.shift()
    return out, np.maximum(hi_peak, acc.peak), ok & acc.ok


def canonical_column_bound(F):
    """An upper bound on every column accumulator of fe_mul / fe_sqr for canonical operands (tight, value below 2p): every product
    at its largest limb bound, quotient digits at 2^29 - 1, plus the carry of the column before."""
    N = F.N
    amax = [TIGHT] * (N - 1) + [(2 * F.p - 1) >> F.top_shift]
    best, carry = 0, 0
    for k in range(2 * N - 1):
        ix = range(max(0, k - N + 1), min(k, N - 1) + 1)
        col = carry + sum(amax[i] * amax[k - i] for i in ix)
        col += sum(TIGHT * F.P[k - i] for i in (range(0, k + 1) if k < N else ix))
        best = max(best, col)
        carry = col >> W
    return best


# ------------------------------------------------------------------------------------------------------------ the vectors
class Case:
    """Inputs of one (field, op) run: limb arrays a, b, c, d (None where the op takes none), and what the checks need"""

    def __init__(self, fid, op):
        self.fid, self.op = fid, op
        self.F = base_of(fid)
        self.a = self.b = self.c = self.d = None
        self.x = None       # the operand the product actually sees, where the op forms it itself (raw differences)
        self.peak = 0       # the largest column accumulator the model found
        self.model = None   # model output limbs, where the op is a single product

    @property
    def n(self):
        return self.a.shape[0]


def _quotient_max(F, rng, la, lb=None):
    """(a, b): a b = p mod R, so every Montgomery quotient digit of a b is 2^29 - 1; b odd below 0.9 p, a below R.  With lb, b has
    every low limb at lb (limb 0 made odd) and a has its low limbs pushed all the way to la: the largest columns the digits allow."""
    b = at_top(F.N, lb, 9 * F.p // 10) if lb is not None else None
    if b is None:
        b = limbs(rng.randrange(1, 9 * F.p // 10) | 1, F.N)
    b[0] -= 1 - b[0] % 2
    a = F.p * pow(values(to_array([b], F.N))[0], -1, F.R) % F.R
    return in_class(rng, a, F.N, la, full=lb is not None), b


def _pairs(F, rng, n, la, lb, vcap=None):
    """n operand pairs (a limbs <= la, b limbs <= lb below the top) with a b < 0.9 R p: specials, the largest k p - 1 times p - 1,
    every low limb at the top of its class, all-maximal quotient digits, values just under the product bound, and random ones"""
    N, p, R = F.N, F.p, F.R
    lim = (9 * R * p - 1) // 10                   # a b <= lim  <=>  a b < 0.9 R p
    vcap = vcap or 2 * R
    A, B = [], []
    sp = [0, 1, p - 1, p, 2 * p - 1]
    for x in sp:
        for y in sp:
            A.append(limbs(x, N))
            B.append(limbs(y, N))
    k = 9 * R // (10 * p)                          # k p - 1 times p - 1 (BLS12-381 Fr: 63 p - 1, the twiddle product's operand bound)
    A.append(in_class(rng, k * p - 1, N, la))
    B.append(limbs(p - 1, N))
    for va in (p, 2 * p, 8 * p, R // 4, R, vcap):
        ta = at_top(N, la, min(va, vcap))
        if ta is None:
            continue
        vb = lim // max(1, values(to_array([ta], N))[0]) + 1
        tb = at_top(N, lb, min(vb, vcap))
        if tb is not None:
            A.append(ta)
            B.append(tb)
    while len(A) < n:
        mode = len(A) % 5
        if mode == 0:
            a, b = _quotient_max(F, rng, la, lb if len(A) % 10 == 0 else None)
        elif mode == 1:
            a, b = limbs(rng.randrange(2 * p), N), limbs(rng.randrange(2 * p), N)
        else:
            va = rng.randrange(1, min(vcap, [2 * p, 16 * p, R][mode - 2]))
            vb = min(lim // va, vcap - 1)
            vb = vb if mode == 4 else rng.randrange(0, vb + 1)   # mode 4: the product just under 0.9 R p
            a, b = in_class(rng, va, N, la), in_class(rng, vb, N, lb)
        A.append(a)
        B.append(b)
    return to_array(A, N), to_array(B, N)


def _class_values(F, rng, n, lim, vmax, specials=()):
    """n elements below vmax with low limbs up to lim: specials, the top of the class, then random ones"""
    rows = [limbs(v, F.N) for v in specials if v < vmax]
    t = at_top(F.N, lim, vmax)
    if t is not None:
        rows.append(t)
    while len(rows) < n:
        rows.append(in_class(rng, rng.randrange(vmax), F.N, lim))
    return to_array(rows[:n], F.N)


def _wq(F, ws):
    return to_array([limbs(w, F.N) for w in ws], F.N), to_array([limbs(w * F.R // F.p, F.N) for w in ws], F.N)


def _assert_limbs(arr, lim, what, top=None):
    """low limbs <= lim (and the top limb <= top when given)"""
    bad = np.nonzero((arr[:, :-1].astype(np.uint64) > lim).any(axis=1) | ((arr[:, -1].astype(np.uint64) > top) if top is not None else False))[0]
    assert not len(bad), f"{what}: limb class violated at {bad[:5]}: {arr[bad[0]].tolist()}"


def _assert_product_bound(F, xs, ys, what, extra=None):
    lim = 9 * F.R * F.p
    for i, (x, y) in enumerate(zip(xs, ys)):
        v = x * y + (extra[i] if extra is not None else 0)
        assert 10 * v < lim, f"{what}: operand values above 0.9 R p at {i}"


def _raw_diff(F, a, b, kb, u):
    """the limbs of fe_sub_raw<F,kb> (u = 2) / fe_sub_raw_bias<F,kb,u>: a + kp - b, checked against the limb range their asserts take"""
    kp = np.array(F.kp_bias(kb + F.margin, u), dtype=np.int64)
    x = a.astype(np.int64) + kp - b.astype(np.int64)
    top = RAW31 if u == 2 else SHOUP
    assert (x >= 0).all() and (x < top).all(), f"raw difference outside its class (bias {u}, every limb)"
    return x.astype(np.uint32)


def make_case(fid, op, n=3000, seed=0):
    """the validated vectors of one (field, op)"""
    rng = random.Random(1000 * fid + op + 7919 * seed)
    cs = Case(fid, op)
    F, N, p, R = cs.F, cs.F.N, cs.F.p, cs.F.R
    name = f"{FIELD_NAMES[fid]} {OP_NAMES[op]}"
    if fid in EXT2_FIELDS:
        return _make_ext2(cs, rng, n, name)
    if op == OPS["MUL"]:
        # the limb bounds of fe_mul itself where the columns have room for them (N = 9); raw times loose for N = 14
        la, lb = (MUL_A - 1, MUL_B - 1) if N <= 9 else (RAW, LOOSE)
        cs.a, cs.b = _pairs(F, rng, n, la, lb)
        _assert_limbs(cs.a, la, name, MUL_A - 1)
        _assert_limbs(cs.b, lb, name, MUL_B - 1)
        _assert_product_bound(F, values(cs.a), values(cs.b), name)
        cs.model, peak, ok, _ = mont_model(F, [(cs.a, cs.b)])
    elif op == OPS["SQR"]:
        la = (1 << 30) - 1 if N <= 9 else LOOSE  # a raw operand may not be squared when N = 14
        vmax = math.isqrt((9 * R * p - 1) // 10)  # a^2 < 0.9 R p
        cs.a = np.concatenate([_class_values(F, rng, n // 3, TIGHT, 2 * p, (0, 1, p - 1, p, 2 * p - 1)),
                               _class_values(F, rng, n - n // 3, la, vmax, (vmax - 1, vmax // 2, 8 * p))])
        _assert_limbs(cs.a, la, name, MUL_B - 1)
        va = values(cs.a)
        _assert_product_bound(F, va, va, name)
        cs.model, peak, ok, _ = mont_model(F, [(cs.a, cs.a)])
    elif op == OPS["MUL_ADD"] or op == OPS["MUL_ADD_NEG_RAW"]:
        cs.a, cs.b = _pairs(F, rng, n, LOOSE, LOOSE)
        cs.c, cs.d = _pairs(F, rng, n, LOOSE, LOOSE)
        # halve the larger product of each element until the sum fits 0.9 R p (the edges stay: the shifts move whole limbs)
        if op == OPS["MUL_ADD_NEG_RAW"]:
            cs.d = _class_values(F, rng, n, LOOSE, 2 * p, (0, 1, p - 1, p, 2 * p - 1))
            kp = np.array(F.kp_bias(2 + F.margin, 2), dtype=np.int64)
            assert (cs.d.astype(np.int64) <= kp).all(), name
            cs.x = (kp - cs.d.astype(np.int64)).astype(np.uint32)  # fe_neg_raw<F,2>
            dd = cs.x
        else:
            dd = cs.d
        va, vb, vc, vd = values(cs.a), values(cs.b), values(cs.c), values(dd)
        lim = 9 * R * p // 10
        for i in range(n):
            while va[i] * vb[i] + vc[i] * vd[i] >= lim:
                if va[i] * vb[i] >= vc[i] * vd[i]:
                    va[i] >>= 1
                    cs.a[i] = in_class(rng, va[i], N, LOOSE)
                else:
                    vc[i] >>= 1
                    cs.c[i] = in_class(rng, vc[i], N, LOOSE)
        for arr in (cs.a, cs.b, cs.c):
            _assert_limbs(arr, LOOSE, name, MUL_B - 1)
        _assert_limbs(dd, LOOSE if op == OPS["MUL_ADD"] else RAW31 - 1, name, MUL_B - 1 if op == OPS["MUL_ADD"] else RAW31 - 1)
        _assert_product_bound(F, values(cs.a), values(cs.b), name, [x * y for x, y in zip(values(cs.c), values(dd))])
        cs.model, peak, ok, _ = mont_model(F, [(cs.a, cs.b), (cs.c, dd)])
    elif op in (OPS["SUB_RAW2_MUL"], OPS["SUB_RAW8_MUL"]):
        kb = 2 if op == OPS["SUB_RAW2_MUL"] else 8
        cs.a = _class_values(F, rng, n, LOOSE, 8 * p, (0, p - 1, 2 * p - 1))
        cs.b = _class_values(F, rng, n, LOOSE, kb * p, (0, kb * p - 1))
        cs.b[: n // 8] = 0                       # a - 0: every difference limb at the top of the raw31 class
        cs.x = _raw_diff(F, cs.a, cs.b, kb, 2)
        vx = values(cs.x)
        lim = (9 * R * p - 1) // 10
        rows = []
        for i in range(n):
            vmax = lim // max(vx[i], 1) + 1
            t = at_top(N, LOOSE, vmax) if i % 4 == 0 else None
            rows.append(t if t is not None else in_class(rng, rng.randrange(vmax) if i % 3 else vmax - 1, N, LOOSE))
        cs.c = to_array(rows, N)
        _assert_limbs(cs.c, LOOSE, name, MUL_B - 1)
        _assert_product_bound(F, vx, values(cs.c), name)
        cs.model, peak, ok, _ = mont_model(F, [(cs.x, cs.c)])
    elif op in (OPS["SHOUP"], OPS["SHOUP_UNIFORM"]):
        # every limb, the top one included, below 3 2^30 + 64; values up to 6 R
        rows = [[0] * N, [SHOUP - 1] * N, [SHOUP - 1] * (N - 1) + [0], limbs(R - 1, N), limbs(p - 1, N)]
        while len(rows) < n:
            m = len(rows) % 4
            vmax = [2 * p, 64 * p, 4 * R, 0][m]
            rows.append(in_class(rng, rng.randrange(vmax), N, SHOUP - 1) if m < 3 else
                        [rng.randrange(SHOUP - (1 << 26), SHOUP) for _ in range(N - 1)] + [rng.randrange(SHOUP)])
        cs.a = to_array(rows, N)
        nw = n if op == OPS["SHOUP"] else (n + 63) // 64
        ws = [0, 1, p - 1, 2, (p - 1) // 2][:nw] + [rng.randrange(p) for _ in range(max(0, nw - 5))]
        cs.b, cs.c = _wq(F, ws)
        w_rows, wq_rows = (cs.b, cs.c) if op == OPS["SHOUP"] else (np.repeat(cs.b, 64, axis=0)[:n], np.repeat(cs.c, 64, axis=0)[:n])
        _assert_limbs(cs.a, SHOUP - 1, name, SHOUP - 1)
        cs.model, peak, ok = shoup_model(F, cs.a, w_rows, wq_rows)
        cs.w_rows = w_rows
    elif op in (OPS["BFLY2"], OPS["BFLY3"]):
        u = 2 if op == OPS["BFLY2"] else 3
        lim = LOOSE if u == 2 else RAW
        cs.a = _class_values(F, rng, n, lim, 8 * p, (0, p, 8 * p - 1))
        cs.b = _class_values(F, rng, n, lim, 8 * p, (0, p, 8 * p - 1))
        cs.b[: n // 8] = 0
        cs.x = _raw_diff(F, cs.a, cs.b, 8, u)
        ws = [0, 1, p - 1] + [rng.randrange(p) for _ in range(n - 3)]
        cs.c, cs.d = _wq(F, ws)
        cs.model, peak, ok = shoup_model(F, cs.x, cs.c, cs.d)
        cs.w_rows = cs.c
    elif op == OPS["SHOUP_PREPARE"]:
        cs.a = _class_values(F, rng, n, TIGHT, 2 * p, (0, 1, p - 1, p, p + 1, 2 * p - 1, R % p))
        peak, ok = 0, True
    elif op in (OPS["REDUCE_MAD"], OPS["REDUCE_SMALL"]):
        top = (1 << 32) - 1 if op == OPS["REDUCE_MAD"] else (1 << 32) - 8   # fe_reduce_small_2p's carry pass: a limb plus 7 fits 32 bits
        vmax = 512 * p
        cs.a = _class_values(F, rng, n, top, vmax, (0, p, 2 * p - 1, vmax - 1, vmax - p))
        peak, ok = 0, True
    elif op == OPS["INV"]:
        n = min(n, 200)
        cs.a = np.concatenate([_class_values(F, rng, n // 2, TIGHT, 2 * p, (0, 1, p - 1, p + 1, 2 * p - 1, R % p)),
                               _class_values(F, rng, n - n // 2, LOOSE, 4 * p)])
        peak, ok = 0, True
    else:
        raise AssertionError(name)
    assert np.all(ok), f"{name}: a column accumulator of the model reaches 2^64"
    cs.peak = int(np.max(peak)) if np.size(peak) else 0
    return cs


def _make_ext2(cs, rng, n, name):
    F, op = cs.F, cs.op
    N, p, R = F.N, F.p, F.R
    if op == OPS["INV"]:
        n = min(n, 100)
    if op == OPS["EXT2_C0"]:
        t0 = _class_values(F, rng, n, TIGHT, 2 * p, (0, p - 1, p, 2 * p - 1))
        t1 = _class_values(F, rng, n, TIGHT, 2 * p, (2 * p - 1, p, 0, 2 * p - 1))
        cs.a = np.concatenate([t0, t1], axis=1)
        return cs
    lim = 9 * R * p // 10

    def comps(cnt, lm, vmax):
        return [_class_values(F, rng, n, lm, vmax, (0, 1, p - 1, p, 2 * p - 1)) for _ in range(cnt)]

    if op == OPS["INV"]:
        a = comps(2, TIGHT, 2 * p)
        a[1][: n // 2] = _class_values(F, rng, n // 2, LOOSE, 4 * p)   # fe_inv wants tight or loose, below 4p
        cs.a = np.concatenate(a, axis=1)
        return cs
    bound = 1 << ((lim // (2 if op == OPS["MUL_ADD"] else 1)).bit_length() // 2 - 1)   # component values: every cross product in bound
    a0, a1, b0, b1 = comps(4, LOOSE, bound)
    if op != OPS["SQR"]:
        for i in range(0, n, 3):  # all-maximal quotient digits in a0 b0 and a1 b1; b below 0.9 p keeps the cross products in bound
            a0[i], b0[i] = _quotient_max(F, rng, LOOSE, LOOSE if i % 2 else None)
            a1[i], b1[i] = _quotient_max(F, rng, LOOSE, LOOSE if i % 2 else None)
    cs.a = np.concatenate([a0, a1], axis=1)
    cs.b = np.concatenate([b0, b1], axis=1) if op != OPS["SQR"] else None
    prods = [[(a0, b0)], [(a1, b1)], [(a0, b1)], [(a1, b0)]] if op == OPS["MUL"] else [[(a0, a0)], [(a1, a1)], [(a0, a1)]]
    if op == OPS["MUL_ADD"]:
        c0, c1, d0, d1 = comps(4, LOOSE, bound)
        for arr in (c0, c1, d0, d1):
            arr[::3] = 0          # where a b has all-maximal quotient digits, c d = 0 keeps it so
        cs.c = np.concatenate([c0, c1], axis=1)
        cs.d = np.concatenate([d0, d1], axis=1)
        prods = [[(a0, b0), (c0, d0)], [(a1, b1), (c1, d1)], [(a0, b1), (c0, d1)], [(a1, b0), (c1, d0)]]
    peak = 0
    for pr in prods:
        for x, _ in pr:
            _assert_limbs(x, LOOSE, name, MUL_B - 1)
        vals = [(values(x), values(y)) for x, y in pr]
        tot = [sum(vx[i] * vy[i] for vx, vy in vals) for i in range(n)]
        assert all(10 * t < 9 * R * p for t in tot), f"{name}: a component product above 0.9 R p"
        _, pk, ok, _ = mont_model(F, pr)
        assert np.all(ok), f"{name}: a column accumulator of the model reaches 2^64"
        peak = max(peak, int(np.max(pk)))
    cs.peak = peak
    return cs


# ------------------------------------------------------------------------------------------------------------ the checks
def _fail(cs, i, why):
    ops = ", ".join(f"{k}={getattr(cs, k)[i].tolist()}" for k in "abcd" if getattr(cs, k) is not None and i < getattr(cs, k).shape[0])
    raise AssertionError(f"{FIELD_NAMES[cs.fid]} (field {cs.fid}) op {OP_NAMES[cs.op]}: element {i}: {why}; operands {ops}")


def _tight_below(cs, F, i, row, bound):
    if any(int(x) > TIGHT for x in row[:-1]):
        _fail(cs, i, f"output not tight: {row.tolist()}")
    v = sum(int(x) << (W * j) for j, x in enumerate(row))
    if v >= bound:
        _fail(cs, i, f"output value {v} not below {bound} ({row.tolist()})")
    return v


def check(cs, out):
    """every element of out (the op's result) against Python big integers: the congruence the op is specified by, the limb class and
    the value bound fe29.h states for it; and, where the op is one product, the column model's limbs bit for bit"""
    F, op, fid = cs.F, cs.op, cs.fid
    N, p, R, Ri = F.N, F.p, F.R, F.Rinv
    n = cs.n
    assert out.shape == (n, out_width(fid, op)), out.shape
    if fid in EXT2_FIELDS:
        return _check_ext2(cs, out)
    if cs.model is not None and not (out == cs.model).all():
        i = int(np.nonzero((out != cs.model).any(axis=1))[0][0])
        _fail(cs, i, f"limbs {out[i].tolist()} differ from the column model's {cs.model[i].tolist()}")
    va = values(cs.a)
    vb = values(cs.b) if cs.b is not None else None
    vc = values(cs.c) if cs.c is not None else None
    vd = values(cs.d) if cs.d is not None else None
    vx = values(cs.x) if cs.x is not None else None
    for i in range(n):
        row = out[i]
        if op in (OPS["MUL"], OPS["SQR"], OPS["MUL_ADD"], OPS["SUB_RAW2_MUL"], OPS["SUB_RAW8_MUL"], OPS["MUL_ADD_NEG_RAW"]):
            if op == OPS["MUL"]:
                t, want = va[i] * vb[i], va[i] * vb[i]
            elif op == OPS["SQR"]:
                t, want = va[i] * va[i], va[i] * va[i]
            elif op == OPS["MUL_ADD"]:
                t, want = va[i] * vb[i] + vc[i] * vd[i], va[i] * vb[i] + vc[i] * vd[i]
            elif op == OPS["MUL_ADD_NEG_RAW"]:
                t, want = va[i] * vb[i] + vc[i] * vx[i], va[i] * vb[i] - vc[i] * vd[i]
            else:
                t, want = vx[i] * vc[i], (va[i] - vb[i]) * vc[i]
            assert vx is None or op == OPS["MUL_ADD_NEG_RAW"] or (vx[i] - va[i] + vb[i]) % p == 0
            v = _tight_below(cs, F, i, row, 2 * p)
            if v * R >= t + p * R:                 # fe_mul: value < a b / R + p
                _fail(cs, i, f"output {v} not below a b / R + p")
            if (v - want * Ri) % p:
                _fail(cs, i, "output not congruent to the product / R")
        elif op in (OPS["SHOUP"], OPS["SHOUP_UNIFORM"], OPS["BFLY2"], OPS["BFLY3"]):
            X = vx[i] if vx is not None else va[i]
            w = values(cs.w_rows[i:i + 1])[0]
            if any(int(x) > TIGHT for x in row):
                _fail(cs, i, f"output not tight: {row.tolist()}")
            v = values(out[i:i + 1])[0]
            if v * R * (1 << 23) >= (R * (1 << 23) + X * (1 << 23) + R) * p:   # value < (1 + x / R + 2^-23) p
                _fail(cs, i, f"output {v} not below (1 + x / R + 2^-23) p")
            src = X if op in (OPS["SHOUP"], OPS["SHOUP_UNIFORM"]) else va[i] - vb[i]
            if (v - src * w) % p:
                _fail(cs, i, "output not congruent to x w")
        elif op == OPS["SHOUP_PREPARE"]:
            w = va[i] * Ri % p
            want = limbs(w, N) + limbs(w * R // p, N)
            if row.tolist() != want:
                _fail(cs, i, f"(w, wq) = {row.tolist()}, want {want}")
        elif op in (OPS["REDUCE_MAD"], OPS["REDUCE_SMALL"]):
            v = _tight_below(cs, F, i, row, 2 * p)
            if (v - va[i]) % p:
                _fail(cs, i, "output not congruent to the input")
        elif op == OPS["INV"]:
            v = _tight_below(cs, F, i, row, 2 * p)
            e = va[i] * Ri % p
            if (v * Ri - (pow(e, -1, p) if e else 0)) % p:
                _fail(cs, i, "output not the inverse")
        else:
            raise AssertionError(op)


def _check_ext2(cs, out):
    F, op = cs.F, cs.op
    N, p, Ri = F.N, F.p, F.Rinv
    beta = EXT2_FIELDS[cs.fid][1]

    def halves(arr):
        return (values(arr[:, :N]), values(arr[:, N:])) if arr is not None else (None, None)

    (a0, a1), (b0, b1), (c0, c1), (d0, d1) = (halves(x) for x in (cs.a, cs.b, cs.c, cs.d))
    for i in range(cs.n):
        r0 = _tight_below(cs, F, i, out[i, :N], 2 * p)
        r1 = _tight_below(cs, F, i, out[i, N:], 2 * p)
        if op == OPS["EXT2_C0"]:
            want = (a0[i] + beta * a1[i], 0)
            if r1 != 0 or out[i, N:].any():
                _fail(cs, i, "c1 not zero")
        elif op == OPS["INV"]:
            e0, e1 = a0[i] * Ri % p, a1[i] * Ri % p
            nrm = (e0 * e0 - beta * e1 * e1) % p
            ni = pow(nrm, -1, p) if nrm else 0
            want = (e0 * ni * F.R, -e1 * ni * F.R)
        else:
            x0, x1 = a0[i], a1[i]
            y0, y1 = (b0[i], b1[i]) if op != OPS["SQR"] else (x0, x1)
            w0, w1 = x0 * y0 + beta * x1 * y1, x0 * y1 + x1 * y0
            if op == OPS["MUL_ADD"]:
                w0 += c0[i] * d0[i] + beta * c1[i] * d1[i]
                w1 += c0[i] * d1[i] + c1[i] * d0[i]
            want = (w0 * Ri, w1 * Ri)
        if (r0 - want[0]) % p or (r1 - want[1]) % p:
            _fail(cs, i, f"output {out[i].tolist()} not congruent to the expected element")
