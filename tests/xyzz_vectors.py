"""Stored points at the edges of the lazy-reduction contract of panda_amd/csrc/curve29.h, for the op table of
panda_amd/csrc/curve29_debug_ops.h, and the checks a result of that table must pass.

A stored point is the 4 W u32 limbs store_xyzz writes -- X, Y, ZZ, ZZZ in internal form (fe29_vectors: the value v of a coordinate's
limbs stands for v / R), W = N limbs each, 2 N for G2 (c0 then c1) -- and an affine base is 2 W limbs.  The contract (units of p):
    X < XB p loose,  Y < YB p loose (2p out of an addition; K p - y in an accumulator seeded from a negated base),  ZZ, ZZZ < 2p tight.
The residues are points m G of pyref / pyref_bls381_g2 / pyref_bls377_g2, scaled by a random non-zero z (X = x z^2, Y = y z^3,
ZZ = z^2, ZZZ = z^3).  What the families choose is the REPRESENTATIVE of each coordinate: residue + j p for every j the bound admits,
with tight limbs.  The LOOSE copy of a family cannot keep the residue: a given residue + j p has one loose spelling only where a digit
is 8 or less, which a random residue never offers.  There the limbs come first -- X and Y are free values in the chosen
representative's range with their limbs at 2^29 + 8 (loose_coord) -- and the point is whatever they stand for, off the curve; the other
operand of a same / opposite vector is then built from the decoded point.  The formulas do not use the curve's b, so nothing changes
for them.  Three more families leave the curve for the same reason: `y0` (Y = j p: a point of order two), `near` (an x one off the
other operand's) and `small` (coordinates whose internal residue is a small integer, which is how a product comes out as residue + p
and P, R reach their largest multiples of p).

A ZZ that is a NON-ZERO multiple of p is left out: a stored ZZ is a product of non-zero field elements (ZZ1 PP, V ZZ, or one), so it is
either all-zero limbs -- the identity -- or a non-zero residue.  Only an all-zero ZZ stands for the identity here.

Every vector is validated against the contract as it is built, and what its family says about it (which rare branch, identity or not)
is compared with what the affine group law says about the decoded operands, so a bad vector fails here and not inside an FE29_CHECK
build."""
import random

import fe29_vectors as fv
import pyref
import pyref_bls377_g2 as g377
import pyref_bls381_g2 as g381
from fe29_vectors import LOOSE, TIGHT, W as LB, at_top, limbs

OPS = dict(MADD_CORE=0, MADD=1, MADD_NEG=2, MADD_NEG_RAW=3, MADD_TRACE=4, DBL_AFFINE=5, DBL=6, ADD=7, ADD_QUAD=8, DBL_QUAD=9,
           TO_JACOBIAN_WIRE=10, TO_HOMOGENEOUS_WIRE=11, TO_AFFINE_INTERNAL=12)
OP_NAMES = {v: k for k, v in OPS.items()}
CURVE_IDS = (0, 1, 2, 3, 4, 6)
CURVE_NAMES = {0: "BN254 G1", 1: "BLS12-377 G1", 2: "BLS12-381 G1", 3: "BN254 G2", 4: "BLS12-381 G2", 6: "BLS12-377 G2"}
_DEF = {0: (0, 1, None, 8), 1: (2, 1, None, 12), 2: (4, 1, None, 12), 3: (0, 2, -1, 8), 4: (4, 2, -1, 12), 6: (2, 2, -5, 12)}
MADD_OPS = (OPS["MADD_CORE"], OPS["MADD"], OPS["MADD_NEG"], OPS["MADD_NEG_RAW"], OPS["MADD_TRACE"])
QUAD_OPS = (OPS["ADD_QUAD"], OPS["DBL_QUAD"])
SAME_X_FAMILIES = ("same", "opposite", "small-same", "small-opposite", "seeded-same", "seeded-opposite")


class Curve:
    """field (fe29_vectors.Field of the base field, D components, beta = u^2), Bounds<F> of curve29.h, and the affine group law"""

    def __init__(self, cid):
        fid, self.D, self.beta, self.Lc = _DEF[cid]
        self.cid, self.F = cid, fv.Field(fid)
        F = self.F
        self.N, self.p, self.W = F.N, F.p, self.D * F.N
        self.M = F.margin
        self.XB = 8 + self.M
        self.YB = F.keff(2 + self.M)
        self.KX, self.KY = F.keff(self.XB + self.M), F.keff(self.YB + self.M)   # what fe_sub<F, XB> / fe_sub<F, YB> add, in units of p
        self.PB, self.RB, self.VB, self.NB = 2 + self.KX, 2 + self.KY, 2 + self.KX, self.YB
        self.raw_ok = self.D == 1 and F.N <= 9
        self.one = (1,) + (0,) * (self.D - 1)
        if cid < 3:
            c = pyref.CURVES[cid]
            self.G = ((c.g[0],), (c.g[1],))
            self._add = lambda P, Q: self._wrap1(pyref.ec_add(c, self._un1(P), self._un1(Q)))
        else:
            self.G = {3: pyref.G2_GEN, 4: g381.GEN, 6: g377.GEN}[cid]
            self._add = {3: pyref.g2_add, 4: g381.add, 6: g377.add}[cid]

    @staticmethod
    def _un1(P):
        return None if P is None else (P[0][0], P[1][0])

    @staticmethod
    def _wrap1(P):
        return None if P is None else ((P[0],), (P[1],))

    def bounds(self):
        return [self.M, self.XB, self.YB, self.PB, self.RB, self.VB, self.NB]

    # field elements: tuples of D canonical integers
    def fmul(self, a, b):
        p = self.p
        if self.D == 1:
            return (a[0] * b[0] % p,)
        return ((a[0] * b[0] + self.beta * a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def finv(self, a):
        p = self.p
        if self.D == 1:
            return (pow(a[0], -1, p),)
        n = pow((a[0] * a[0] - self.beta * a[1] * a[1]) % p, -1, p)
        return (a[0] * n % p, -a[1] * n % p)

    def fneg(self, a):
        return tuple(-x % self.p for x in a)

    def enc(self, e):
        """internal-form residues of a field element"""
        return tuple(x * self.F.R % self.p for x in e)

    def dec(self, vals):
        return tuple(v * self.F.Rinv % self.p for v in vals)

    # the affine group law of pyref; None is the identity.  Its chord and tangent formulas do not use the curve's b, so they also say what
    # the XYZZ formulas (the same rational functions) give for the off-curve operands of the y0 / near / small families.
    def add(self, P, Q):
        if P is not None and Q is not None and P[0] == Q[0] and P[1] != Q[1]:
            assert self.fneg(P[1]) == Q[1], "same x, unrelated y: not a case the formulas define"
        return self._norm(self._add(self._norm(P), self._norm(Q)))

    def _norm(self, P):
        return None if P is None else (tuple(int(v) for v in P[0]), tuple(int(v) for v in P[1]))

    def neg(self, P):
        return None if P is None else (P[0], self.fneg(P[1]))

    def multiples(self, n):
        out, acc = [], None
        for _ in range(n):
            acc = self.add(acc, self.G)
            out.append(acc)
        return out


_CURVES = {}


def curve(cid):
    if cid not in _CURVES:
        _CURVES[cid] = Curve(cid)
    return _CURVES[cid]


def supported(cid, op):
    """mirror of xyzz_debug_supported"""
    return cid in CURVE_IDS and 0 <= op < len(OPS) and (op != OPS["MADD_NEG_RAW"] or curve(cid).raw_ok)


def cases():
    return [(cid, op) for cid in CURVE_IDS for op in range(len(OPS)) if supported(cid, op)]


def out_width(cid, op):
    c = curve(cid)
    if op == OPS["MADD_CORE"]:
        return 4 * c.W + 1
    if op == OPS["MADD_TRACE"]:
        return 3 * c.W
    if op in QUAD_OPS:
        return 16 * c.W
    if op in (OPS["TO_JACOBIAN_WIRE"], OPS["TO_HOMOGENEOUS_WIRE"]):
        return 3 * c.D * c.Lc
    if op == OPS["TO_AFFINE_INTERNAL"]:
        return 2 * c.W
    return 4 * c.W


# ------------------------------------------------------------------------------------------------------------ building blocks
def _j(c, j):
    return (j,) * c.D if isinstance(j, int) else tuple(j)


def coord(c, rng, res, j, delta=None):
    """W tight limbs: component k at res[k] + j[k] p (+ delta[k])"""
    out = []
    for k, jk in enumerate(_j(c, j)):
        v = res[k] + jk * c.p + (delta[k] if delta else 0)
        assert v >= 0
        out += limbs(v, c.N)
    return out


def loose_coord(c, rng, j, full=True):
    """W limbs of a FREE value at the top of the loose class: component k somewhere in [j[k] p, (j[k] + 1) p), its limbs 0 .. N-3 at
    2^29 + 8 (full; otherwise anywhere in [2^29, 2^29 + 8]) and limb N-2 there as well where that range holds such a value (at_top).
    A residue that is given cannot be written this way -- a digit of a random residue is almost never 8 or less, which is what borrowing
    2^29 from the limb above needs -- so the limbs come first and the residue, hence the point, is whatever they stand for."""
    out = []
    N, p = c.N, c.p
    unit = 1 << (LB * (N - 2))
    for jk in _j(c, j):
        t = at_top(N, LOOSE, (jk + 1) * p) if full else None
        if t is not None and sum(x << (LB * i) for i, x in enumerate(t)) >= jk * p:
            out += t
            continue
        low = [LOOSE if full else rng.randint(1 << LB, LOOSE) for _ in range(N - 2)]
        v0 = (jk + 1) * p - 1 if full else rng.randrange(jk * p + 2 * unit, (jk + 1) * p)
        rem = (v0 - sum(x << (LB * i) for i, x in enumerate(low))) >> (LB * (N - 2))   # the value lands in (v0 - unit, v0]
        out += low + [rem & fv.MASK, rem >> LB]
    return out


def stored(c, rng, A, z, jx=0, jy=0, jzz=0, jzzz=0, loose=False, full=True, dx=None, dy=None):
    """the point A scaled by z, each coordinate at the chosen representative, tight.  loose (True, or 'x' / 'y' for one coordinate): X and
    / or Y are FREE loose values in the chosen representative's range instead (loose_coord), so the point is no longer A but whatever
    decode_stored says -- off the curve, which the formulas do not mind; a family that needs the other operand equal to it decodes it."""
    zz = c.fmul(z, z)
    zzz = c.fmul(zz, z)
    lx, ly = loose in (True, "x"), loose in (True, "y")
    assert not (lx and dx) and not (ly and dy)
    return ((loose_coord(c, rng, jx, full) if lx else coord(c, rng, c.enc(c.fmul(A[0], zz)), jx, dx))
            + (loose_coord(c, rng, jy, full) if ly else coord(c, rng, c.enc(c.fmul(A[1], zzz)), jy, dy))
            + coord(c, rng, c.enc(zz), jzz) + coord(c, rng, c.enc(zzz), jzzz))


def base(c, rng, B, jx=0, jy=0, dx=None, dy=None):
    if B is None:
        return [0] * (2 * c.W)
    return coord(c, rng, c.enc(B[0]), jx, dx) + coord(c, rng, c.enc(B[1]), jy, dy)


def fe_norm(l):
    """fe_norm of fe29.h on one component's limbs"""
    n = len(l)
    cy = [x >> LB for x in l[:-1]]
    return [l[0] & fv.MASK] + [(l[i] & fv.MASK) + cy[i - 1] for i in range(1, n - 1)] + [l[-1] + cy[-1]]


def seeded(c, rng, B0, raw):
    """what xyzz_from_affine leaves when an identity accumulator takes a NEGATED base: (x, fe_norm(K p - y), one, one) with K p - y formed
    as fe_neg<F, 1> does (raw: as fe_neg_raw<F, 1> does, then fe_norm, the way k_accumulate stores it).  Stands for -B0."""
    F = c.F
    kp = F.kp_bias(1 + F.margin, 2) if raw else F.kp_biased(1 + F.margin)
    y = []
    for r in c.enc(B0[1]):
        t = [k - x for k, x in zip(kp, limbs(r, c.N))]
        assert min(t) >= 0
        y += fe_norm(t)
    one = c.enc(c.one)
    return coord(c, rng, c.enc(B0[0]), 0) + y + coord(c, rng, one, 0) + coord(c, rng, one, 0)


def identity_point(c, rng):
    """ZZ all zero; X, Y, ZZZ arbitrary within their classes (only ZZ decides)"""
    full = rng.random() < 0.5
    return (loose_coord(c, rng, [rng.randrange(c.XB) for _ in range(c.D)], full) + loose_coord(c, rng, [rng.randrange(c.YB) for _ in range(c.D)], full)
            + [0] * c.W + coord(c, rng, [rng.randrange(2 * c.p) for _ in range(c.D)], 0))


def rand_z(c, rng):
    return tuple(rng.randrange(1, c.p) for _ in range(c.D))


def rand_stored(c, rng, A):
    """A under a random z at random representatives, tight; or (more often) free loose X, Y with limbs anywhere in [2^29, 2^29 + 8]"""
    D = c.D
    return stored(c, rng, A, rand_z(c, rng), [rng.randrange(c.XB) for _ in range(D)], [rng.randrange(c.YB) for _ in range(D)],
                  [rng.randrange(2) for _ in range(D)], [rng.randrange(2) for _ in range(D)], loose=rng.random() < 0.6, full=False)


# ------------------------------------------------------------------------------------------------------------ decoding
def split(c, row, k):
    """coordinate k of a limb row as D component values"""
    return tuple(sum(int(x) << (LB * j) for j, x in enumerate(row[k * c.W + d * c.N: k * c.W + (d + 1) * c.N])) for d in range(c.D))


def decode_stored(c, row):
    """affine point of a stored point, None for the identity (ZZ all zero)"""
    if not any(int(x) for x in row[2 * c.W: 3 * c.W]):
        return None
    X, Y, ZZ, ZZZ = (c.dec(split(c, row, k)) for k in range(4))
    assert any(ZZ), "ZZ is a non-zero multiple of p: not a stored value"
    return c.fmul(X, c.finv(ZZ)), c.fmul(Y, c.finv(ZZZ))


def decode_base(c, row):
    if not any(int(x) for x in row[: 2 * c.W]):
        return None
    return c.dec(split(c, row, 0)), c.dec(split(c, row, 1))


def _class_ok(c, row, k, lim, bound):
    vals = split(c, row, k)
    for d in range(c.D):
        seg = row[k * c.W + d * c.N: k * c.W + (d + 1) * c.N]
        if any(int(x) > lim for x in seg[:-1]) or vals[d] >= bound * c.p:
            return False
    return True


def stored_contract_violation(c, row, ybound=None):
    """None, or what a stored point breaks: X < XB p loose, Y < ybound p (default YB) loose, ZZ, ZZZ < 2p tight, ZZ^3 = ZZZ^2"""
    if not _class_ok(c, row, 0, LOOSE, c.XB):
        return "X outside [0, XB p) or its limbs not loose"
    if not _class_ok(c, row, 1, LOOSE, ybound or c.YB):
        return f"Y outside [0, {ybound or c.YB} p) or its limbs not loose"
    if not _class_ok(c, row, 2, TIGHT, 2) or not _class_ok(c, row, 3, TIGHT, 2):
        return "ZZ or ZZZ outside [0, 2p) or not tight"
    if any(int(x) for x in row[2 * c.W: 3 * c.W]):
        ZZ, ZZZ = c.dec(split(c, row, 2)), c.dec(split(c, row, 3))
        if not any(ZZ):
            return "ZZ is a non-zero multiple of p"
        if c.fmul(c.fmul(ZZ, ZZ), ZZ) != c.fmul(ZZZ, ZZZ):
            return "ZZ^3 != ZZZ^2"
    return None


# ------------------------------------------------------------------------------------------------------------ the vectors
class Case:
    def __init__(self, cid, op):
        self.cid, self.op, self.c = cid, op, curve(cid)
        self.rows_a, self.rows_b, self.family, self.expect = [], [], [], []
        self.a = self.b = None

    def put(self, family, a, b, expect=None):
        """expect: what the family says of the vector -- 'same' / 'opposite' (the rare branches), 'identity' (the result), 'plain'"""
        self.rows_a.append(a)
        self.rows_b.append(b)
        self.family.append(family)
        self.expect.append(expect)

    @property
    def n(self):
        return len(self.family)

    def where(self, *families):
        return [i for i, f in enumerate(self.family) if f in families]


def _neg_mode(op):
    return {OPS["MADD_NEG"]: 1, OPS["MADD_NEG_RAW"]: 2}.get(op, 0)


def _madd_vectors(cs, rng):
    c, op = cs.c, cs.op
    neg = _neg_mode(op)
    with_identity = op not in (OPS["MADD_CORE"], OPS["MADD_TRACE"])
    jbs = (0,) if neg else (0, 1)   # fe_neg<F, 1> takes a canonical y
    pts = c.multiples(9)
    D, XB, YB, p = c.D, c.XB, c.YB, c.p
    eff = (lambda P: c.neg(P)) if neg else (lambda P: P)   # the base to store so that the point ADDED is P

    def reps(A, z, fam, mk_b, expect, loose_modes=(False, True)):
        """the accumulator's X, then Y, over every representative; the other coordinate and the base cycle through theirs.  mk_b gets the
        point the accumulator stands for: A in the tight pass, a free one in the loose pass"""
        k = 0
        for loose in loose_modes:
            for jx in range(XB):
                k += 1
                jb = jbs[k % len(jbs)]
                jxs = (jx, XB - 1 - jx) if D == 2 and loose else jx   # G2: the components at different representatives in the loose pass
                acc = stored(c, rng, A, z, jxs, jx % YB, k % 2, (k // 2) % 2, loose)
                cs.put(fam, acc, mk_b(jb, decode_stored(c, acc)), expect)
            for jy in range(YB):
                k += 1
                jb = jbs[k % len(jbs)]
                jys = (jy, YB - 1 - jy) if D == 2 and loose else jy
                acc = stored(c, rng, A, z, (3 * jy + 1) % XB, jys, (k // 2) % 2, k % 2, loose)
                cs.put(fam, acc, mk_b(jb, decode_stored(c, acc)), expect)

    # sweep: every representative of X and of Y, ZZ and ZZZ at residue and residue + p, tight and loose
    for A, B in ((pts[0], pts[1]), (pts[4], pts[2])):
        reps(A, rand_z(c, rng), "sweep", lambda jb, P, B=B: base(c, rng, eff(B), jb, jb), "plain")
    # top: the largest values the contract admits in all four coordinates at once
    for A, B in ((pts[1], pts[3]), (pts[5], pts[0]), (pts[6], pts[7])):
        for loose in (False, True):
            cs.put("top", stored(c, rng, A, rand_z(c, rng), XB - 1, YB - 1, 1, 1, loose), base(c, rng, eff(B), jbs[-1], jbs[-1]), "plain")
    # seeded: Y = fe_norm(K p - y), then a tight / negated / raw-negated base (whichever this op feeds)
    for B0 in pts[:3]:
        for raw in ((False, True) if c.raw_ok else (False,)):
            for B in (pts[3], pts[8]):
                cs.put("seeded", seeded(c, rng, B0, raw), base(c, rng, eff(B), jbs[-1], 0), "plain")
            cs.put("seeded-same", seeded(c, rng, B0, raw), base(c, rng, eff(c.neg(B0))), "same")
            cs.put("seeded-opposite", seeded(c, rng, B0, raw), base(c, rng, eff(B0)), "opposite")
    # same point / opposite points: the base is the accumulator's point (or its negative), z = 1 and z != 1
    for A in pts[:2]:
        for z in (c.one, rand_z(c, rng)):
            reps(A, z, "same", lambda jb, P: base(c, rng, eff(P), jb, jb), "same")
            reps(A, z, "opposite", lambda jb, P: base(c, rng, eff(c.neg(P)), jb, jb), "opposite")
    # small: internal residues 1, 2, 3, ... (off the curve), z = 1 -- the products base x ZZ and base y ZZZ then come out as residue + p
    # whenever the base sits at residue + p, which is what takes P and R to their largest multiple of p
    for t in (1, 2, 5):
        A = (c.dec((t,) * D), c.dec((t + 1,) * D))
        reps(A, c.one, "small-same", lambda jb, P: base(c, rng, eff(P), jbs[-1], jbs[-1]), "same", (False,))
        reps(A, c.one, "small-opposite", lambda jb, P: base(c, rng, eff(c.neg(P)), jbs[-1], jbs[-1]), "opposite", (False,))
    # near miss: the accumulator's X one off the value that would make the x coordinates equal, in every representative (p +- 1,
    # 2p +- 1, ... across representatives): never the rare branch
    k = 0
    for A in pts[2:4]:
        for z in (c.one, rand_z(c, rng)):
            for jx in range(XB):
                for d in (1, -1):
                    k += 1
                    dx = tuple(d if (D == 1 or comp == k % 2) else 0 for comp in range(D))
                    if jx == 0 and d < 0:
                        continue
                    cs.put("near", stored(c, rng, A, z, jx, k % YB, 0, 0, "y" if k % 2 else False, dx=dx), base(c, rng, eff(A), jbs[k % len(jbs)], 0), "plain")
    # identity accumulators and identity bases
    if with_identity:
        for B in pts[:4]:
            cs.put("identity", identity_point(c, rng), base(c, rng, eff(B), jbs[-1], 0), "plain")
            cs.put("identity", rand_stored(c, rng, B), base(c, rng, None), "plain")
            cs.put("identity", identity_point(c, rng), base(c, rng, None), "identity")
        cs.put("identity", [0] * (4 * c.W), base(c, rng, eff(pts[0])), "plain")
    # bulk: random representatives inside the classes
    for i in range(150):
        A, B = pts[rng.randrange(9)], pts[rng.randrange(9)]
        if A[0] == B[0]:
            continue
        cs.put("bulk", rand_stored(c, rng, A), base(c, rng, eff(B), rng.choice(jbs), rng.choice(jbs)), "plain")


def _single_vectors(cs, rng, families):
    """one stored point per element: DBL, DBL_QUAD and the output conversions"""
    c = cs.c
    pts = c.multiples(9)
    D, XB, YB, p = c.D, c.XB, c.YB, c.p
    k = 0
    for A in (pts[0], pts[3]):
        z = rand_z(c, rng)
        for loose in (False, True):
            for jx in range(XB):
                k += 1
                cs.put("sweep", stored(c, rng, A, z, (jx, XB - 1 - jx) if D == 2 and k % 2 else jx, jx % YB, k % 2, (k // 2) % 2, loose), None, "plain")
            for jy in range(YB):
                k += 1
                cs.put("sweep", stored(c, rng, A, z, (5 * jy + 2) % XB, (jy, YB - 1 - jy) if D == 2 and k % 2 else jy, (k // 2) % 2, k % 2, loose), None, "plain")
    for A in pts[4:7]:
        for loose in (False, True):
            cs.put("top", stored(c, rng, A, rand_z(c, rng), XB - 1, YB - 1, 1, 1, loose), None, "plain")
    for B0 in pts[:3]:
        for raw in ((False, True) if c.raw_ok else (False,)):
            cs.put("seeded", seeded(c, rng, B0, raw), None, "plain")
    if "identity" in families:
        for _ in range(4):
            cs.put("identity", identity_point(c, rng), None, "identity")
        cs.put("identity", [0] * (4 * c.W), None, "identity")
    if "y0" in families:
        # Y = j p in every representative (both components for G2): "a point of order two", off the curve; and Y = j p +- 1, which is not
        for A in pts[1:3]:
            z = rand_z(c, rng)
            zero = (A[0], (0,) * D)
            for jy in range(YB):
                k += 1
                cs.put("y0", stored(c, rng, zero, z, k % XB, (jy, (jy + k) % YB) if D == 2 else jy, 0, k % 2, "x" if k % 2 else False), None, "identity")
                for d in (1, -1):
                    if jy == 0 and d < 0:
                        continue
                    dy = tuple(d if comp == k % D else 0 for comp in range(D))
                    cs.put("y0-near", stored(c, rng, zero, z, k % XB, jy, 0, 0, False, dy=dy), None, "plain")
    for i in range(150):
        cs.put("bulk", rand_stored(c, rng, pts[rng.randrange(9)]), None, "plain")


def _dbl_affine_vectors(cs, rng):
    c = cs.c
    pts = c.multiples(9)
    D = c.D
    for A in pts:
        for jx in (0, 1):
            for jy in (0, 1):
                cs.put("sweep", None, base(c, rng, A, jx, (jy, 1 - jy) if D == 2 else jy), "plain")
    for A in pts[:3]:
        zero = (A[0], (0,) * D)
        for jy in ((0, 0), (0, 1), (1, 0), (1, 1)) if D == 2 else (0, 1):
            cs.put("y0", None, base(c, rng, zero, 1, jy), "identity")
        for jy in (0, 1):
            for d in (1, -1):
                if jy == 0 and d < 0:
                    continue
                cs.put("y0-near", None, base(c, rng, zero, 0, jy, dy=(d,) + (0,) * (D - 1)), "plain")
    for i in range(100):
        cs.put("bulk", None, base(c, rng, pts[rng.randrange(9)], [rng.randrange(2) for _ in range(D)], [rng.randrange(2) for _ in range(D)]), "plain")


def _add_vectors(cs, rng):
    c = cs.c
    pts = c.multiples(9)
    D, XB, YB = c.D, c.XB, c.YB

    def reps(fam, A, za, Bq, zb, expect):
        """every representative of X and Y, first in the accumulator, then in the second operand, tight and loose; the other operand tight at
        random representatives.  In the loose pass the swept operand is a free point, and the other one is built from what it decodes to"""
        k = 0

        def pair(side, jx, jy, jzz, jzzz, loose):
            sw = stored(c, rng, (A, Bq)[side], (za, zb)[side], jx, jy, jzz, jzzz, loose)
            other = (Bq, A)[side]
            if loose and expect != "plain":
                P = decode_stored(c, sw)
                other = P if expect == "same" else c.neg(P)
            ot = stored(c, rng, other, (zb, za)[side], rng.randrange(XB), rng.randrange(YB), rng.randrange(2), rng.randrange(2))
            cs.put(fam, *((sw, ot) if side == 0 else (ot, sw)), expect)

        for side in (0, 1):
            for loose in (False, True):
                for jx in range(XB):
                    k += 1
                    pair(side, (jx, XB - 1 - jx) if D == 2 and k % 2 else jx, jx % YB, k % 2, (k // 2) % 2, loose)
                for jy in range(YB):
                    k += 1
                    pair(side, (3 * jy + 1) % XB, (jy, YB - 1 - jy) if D == 2 and k % 2 else jy, (k // 2) % 2, k % 2, loose)

    reps("sweep", pts[0], rand_z(c, rng), pts[1], rand_z(c, rng), "plain")
    for A, B in ((pts[1], pts[3]), (pts[5], pts[0]), (pts[6], pts[7])):   # top: both operands at once
        for loose in (False, True):
            cs.put("top", stored(c, rng, A, rand_z(c, rng), XB - 1, YB - 1, 1, 1, loose), stored(c, rng, B, rand_z(c, rng), XB - 1, YB - 1, 1, 1, loose), "plain")
    for A in (pts[2], pts[4]):   # same point under two different z, and its negative
        reps("same", A, rand_z(c, rng), A, rand_z(c, rng), "same")
        reps("opposite", A, rand_z(c, rng), c.neg(A), rand_z(c, rng), "opposite")
    reps("same", pts[3], c.one, pts[3], rand_z(c, rng), "same")
    for B0 in pts[:3]:
        for raw in ((False, True) if c.raw_ok else (False,)):
            z = rand_z(c, rng)
            cs.put("seeded", seeded(c, rng, B0, raw), rand_stored(c, rng, pts[5]), "plain")
            cs.put("seeded", rand_stored(c, rng, pts[5]), seeded(c, rng, B0, raw), "plain")
            cs.put("seeded-same", seeded(c, rng, B0, raw), stored(c, rng, c.neg(B0), z, XB - 1, YB - 1, 1, 1), "same")
            cs.put("seeded-opposite", stored(c, rng, B0, z, XB - 1, YB - 1, 1, 1), seeded(c, rng, B0, raw), "opposite")
    k = 0
    for A in pts[2:4]:   # near miss: z = 1 on both sides, so U1 = X1 and U2 = X2 as residues; X one off, in every representative
        for jx in range(XB):
            for d in (1, -1):
                k += 1
                if jx == 0 and d < 0:
                    continue
                dx = tuple(d if (D == 1 or comp == k % 2) else 0 for comp in range(D))
                near = stored(c, rng, A, c.one, jx, k % YB, 0, 0, "y" if k % 2 else False, dx=dx)
                plain = stored(c, rng, A, c.one, (k * 5) % XB, (k * 3) % YB, 0, 0, "y" if k % 3 == 0 else False)
                cs.put("near", *((near, plain) if k % 4 < 2 else (plain, near)), "plain")
    for B in pts[:4]:
        cs.put("identity", identity_point(c, rng), rand_stored(c, rng, B), "plain")
        cs.put("identity", rand_stored(c, rng, B), identity_point(c, rng), "plain")
        cs.put("identity", identity_point(c, rng), identity_point(c, rng), "identity")
    for i in range(150):
        A, B = pts[rng.randrange(9)], pts[rng.randrange(9)]
        if A[0] == B[0]:
            continue
        cs.put("bulk", rand_stored(c, rng, A), rand_stored(c, rng, B), "plain")


def operands(cs, i):
    """(A, B) of element i as affine points decoded from its limbs, B already negated where the op negates it; B is None for one-operand ops"""
    c, op = cs.c, cs.op
    if op in MADD_OPS:
        B = decode_base(c, cs.b[i])
        return decode_stored(c, cs.a[i]), (c.neg(B) if _neg_mode(op) else B)
    if op == OPS["DBL_AFFINE"]:
        B = decode_base(c, cs.b[i])
        return B, B
    if op in (OPS["ADD"], OPS["ADD_QUAD"]):
        return decode_stored(c, cs.a[i]), decode_stored(c, cs.b[i])
    A = decode_stored(c, cs.a[i])
    return A, (A if op in (OPS["DBL"], OPS["DBL_QUAD"]) else None)


def want_rare(c, A, B):
    """what xyzz_madd_core must return for non-identity A, B"""
    if A[0] != B[0]:
        return 0
    return 1 if A[1] == B[1] else 2


def _validate(cs):
    c, op = cs.c, cs.op
    name = f"{CURVE_NAMES[cs.cid]} {OP_NAMES[op]}"
    stored_b = op in (OPS["ADD"], OPS["ADD_QUAD"])
    for i in range(cs.n):
        what = f"{name} element {i} ({cs.family[i]})"
        if cs.a is not None:
            bad = stored_contract_violation(c, cs.a[i])
            assert bad is None, f"{what}: a: {bad}"
        if cs.b is not None and stored_b:
            bad = stored_contract_violation(c, cs.b[i])
            assert bad is None, f"{what}: b: {bad}"
        elif cs.b is not None:   # an affine base: tight, below 2p; canonical where the op negates it
            for k in (0, 1):
                assert _class_ok(c, cs.b[i], k, TIGHT, 1 if (_neg_mode(op) and k == 1) else 2), f"{what}: base coordinate {k} outside its class"
        A, B = operands(cs, i)
        if op in (OPS["MADD_CORE"], OPS["MADD_TRACE"]):
            assert A is not None and B is not None, f"{what}: xyzz_madd_core takes no identity"
        exp = cs.expect[i]
        if B is not None or op in MADD_OPS or stored_b:
            if A is not None and B is not None and (op in MADD_OPS or stored_b):
                assert {0: "plain", 1: "same", 2: "opposite"}[want_rare(c, A, B)] == (exp if exp in ("same", "opposite") else "plain"), f"{what}: family says {exp}"
            res = c.add(A, B)
            assert (res is None) == (exp in ("opposite", "identity")), f"{what}: family says {exp}, the group law says {res}"
        else:
            assert (A is None) == (exp == "identity"), what


def make_case(cid, op, seed=0):
    """the validated vectors of one (curve, op)"""
    assert supported(cid, op)
    # the ops of one group share their vectors (one seed): MADD / MADD_CORE / MADD_TRACE, ADD / ADD_QUAD, DBL / DBL_QUAD
    group = {OPS["MADD_CORE"]: OPS["MADD_TRACE"], OPS["ADD_QUAD"]: OPS["ADD"], OPS["DBL_QUAD"]: OPS["DBL"]}.get(op, op)
    rng = random.Random(1000 * cid + group + 7919 * seed)
    cs = Case(cid, op)
    c = cs.c
    if op in MADD_OPS:
        _madd_vectors(cs, rng)
    elif op == OPS["DBL_AFFINE"]:
        _dbl_affine_vectors(cs, rng)
    elif op in (OPS["ADD"], OPS["ADD_QUAD"]):
        _add_vectors(cs, rng)
    elif op in (OPS["DBL"], OPS["DBL_QUAD"]):
        _single_vectors(cs, rng, ("identity", "y0"))
    elif op == OPS["TO_AFFINE_INTERNAL"]:
        _single_vectors(cs, rng, ())
    else:
        _single_vectors(cs, rng, ("identity",))
    assert cs.n <= 2000, cs.n
    if cs.rows_a[0] is not None:
        cs.a = fv.to_array(cs.rows_a, 4 * c.W)
    if cs.rows_b[0] is not None:
        cs.b = fv.to_array(cs.rows_b, len(cs.rows_b[0]))
    cs.rows_a = cs.rows_b = None
    _validate(cs)
    return cs


# ------------------------------------------------------------------------------------------------------------ the checks
def _fail(cs, i, why):
    ops = ", ".join(f"{k}={getattr(cs, k)[i].tolist()}" for k in "ab" if getattr(cs, k) is not None)
    raise AssertionError(f"{CURVE_NAMES[cs.cid]} (curve {cs.cid}) op {OP_NAMES[cs.op]}: element {i} ({cs.family[i]}): {why}; operands {ops}")


def check_point(cs, i, row, want, formula):
    """a stored point out of the table: the affine point it stands for, and the stored-point contract.  formula: the point came out of
    an addition or doubling (Y below 2p, the identity as all-zero limbs); otherwise an operand was handed through (Y below YB p)."""
    c = cs.c
    bad = stored_contract_violation(c, row, 2 if formula else None)
    if bad:
        _fail(cs, i, f"result {row.tolist()}: {bad}")
    got = decode_stored(c, row)
    if want is None:
        if got is not None:
            _fail(cs, i, f"result is not the identity: {row.tolist()}")
        if formula and row.any():
            _fail(cs, i, f"the identity out of a formula is all-zero limbs, got {row.tolist()}")
    elif got != want:
        _fail(cs, i, f"result {row.tolist()} stands for {got}, the group law gives {want}")


def _wire(c, e):
    """canonical wire words of a field element: component by component, e 2^(32 Lc) mod p in 32-bit limbs"""
    return [int(x) for comp in e for x in pyref.int_to_limbs(comp * (1 << (32 * c.Lc)) % c.p, c.Lc)]


def check(cs, out):
    """every element of out against Python integers and the affine group law of pyref"""
    c, op = cs.c, cs.op
    W = c.W
    assert out.shape == (cs.n, out_width(cs.cid, op)), out.shape
    for i in range(cs.n):
        row = out[i]
        A, B = operands(cs, i)
        if op == OPS["MADD_TRACE"]:
            continue   # read by the reach test
        if op in (OPS["TO_JACOBIAN_WIRE"], OPS["TO_HOMOGENEOUS_WIRE"]):
            if A is None:
                want = [0] * (3 * c.D * c.Lc)
            else:
                X, Y, ZZ, ZZZ = (c.dec(split(c, cs.a[i], k)) for k in range(4))
                if op == OPS["TO_JACOBIAN_WIRE"]:
                    want = _wire(c, c.fmul(X, ZZ)) + _wire(c, c.fmul(Y, ZZZ)) + _wire(c, ZZ)
                else:
                    want = _wire(c, c.fmul(X, ZZZ)) + _wire(c, c.fmul(Y, ZZ)) + _wire(c, c.fmul(ZZ, ZZZ))
            if row.tolist() != want:
                _fail(cs, i, f"wire words {row.tolist()}, want the canonical {want}")
            continue
        if op == OPS["TO_AFFINE_INTERNAL"]:
            for k in (0, 1):
                if not _class_ok(c, row, k, TIGHT, 2):
                    _fail(cs, i, f"affine coordinate {k} not tight below 2p: {row.tolist()}")
            got = (c.dec(split(c, row, 0)), c.dec(split(c, row, 1)))
            if got != A:
                _fail(cs, i, f"affine point {got}, want {A}")
            continue
        want = c.add(A, B)
        if op == OPS["MADD_CORE"]:
            rare = int(row[4 * W])
            if rare != want_rare(c, A, B):
                _fail(cs, i, f"rare = {rare}, want {want_rare(c, A, B)}")
            if rare:
                if row[: 4 * W].tolist() != cs.a[i].tolist():
                    _fail(cs, i, "the accumulator changed on a rare return")
            else:
                check_point(cs, i, row[: 4 * W], want, True)
            continue
        formula = A is not None and B is not None
        if op in QUAD_OPS:
            for lane in range(1, 4):
                if (row[lane * 4 * W: (lane + 1) * 4 * W] != row[: 4 * W]).any():
                    _fail(cs, i, f"lane {lane} of the quad holds {row[lane * 4 * W: (lane + 1) * 4 * W].tolist()}, lane 0 {row[: 4 * W].tolist()}")
        if op in (OPS["DBL"], OPS["DBL_QUAD"], OPS["DBL_AFFINE"]):
            formula = True
        check_point(cs, i, row[: 4 * W], want, formula)
