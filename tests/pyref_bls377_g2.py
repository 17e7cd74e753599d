"""BLS12-377 G2 over Python integers (test infrastructure; curve id 6 of the C ABI).

The twist y^2 = x^3 + b' over Fq2 = Fq[u]/(u^2 + 5), b' = 1/u = (0, -1/5 mod p).  p = 1 mod 4 here, so -1 is a square and u^2 = -1
would not give a field; -5 is a non-residue.  This implementation -- affine arithmetic over pairs of Python ints, sharing no code with
the kernels or the oracle -- is the only oracle the BLS12-377 G2 tests have, pinned by the curve equation, b' u = 1 and the group order
of arkworks' G2 generator.  Wire format as for BLS12-381 G2: an Fq2 element is c0 || c1, each 12 Montgomery-form u32 limbs
(R = 2^384); affine x || y = 48 words (identity <=> x == 0), Jacobian / homogeneous X || Y || Z = 72 words.  Scalars: 8
Montgomery-form words of BLS12-377 Fr, as for G1.
"""
from __future__ import annotations

import numpy as np

from pyref import BLS12_377, CURVES, decode_scalar, int_to_limbs, limbs_to_int

BLS12_377_G2 = 6
C377 = CURVES[BLS12_377]
P = C377.p
R = C377.r
LQ = 12  # wire words of one Fq component
BETA = P - 5  # u^2
B2 = (0, (-pow(5, -1, P)) % P)  # 1 / u = -u / 5
GEN = ((233578398248691099356572568220835526895379068987715365179118596935057653620464273615301663571204657964920925606294,
        140913150380207355837477652521042157274541796891053068589147167627541651775299824604154852141315666357241556069118),
       (63160294768292073209381361943935198908131692476676907196754037919244929611450776219210369229519898517858833747423,
        149157405641012693445398062341192467754805999074082136895788947234480009303640899064710353187729182149407503257491))
U = (0, 1)


def f2_add(a, b):
    return (a[0] + b[0]) % P, (a[1] + b[1]) % P


def f2_sub(a, b):
    return (a[0] - b[0]) % P, (a[1] - b[1]) % P


def f2_neg(a):
    return (-a[0]) % P, (-a[1]) % P


def f2_mul(a, b):
    return (a[0] * b[0] - 5 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P


def f2_inv(a):
    """0 -> 0, as the library's fe_inv"""
    nrm = (a[0] * a[0] + 5 * a[1] * a[1]) % P
    if nrm == 0:
        return 0, 0
    n = pow(nrm, -1, P)
    return a[0] * n % P, -a[1] * n % P


def is_on_curve(Q) -> bool:
    if Q is None:
        return True
    x, y = Q
    return f2_mul(y, y) == f2_add(f2_mul(f2_mul(x, x), x), B2)


def add(A, Bp):
    """Affine addition on the twist; None is the identity."""
    if A is None:
        return Bp
    if Bp is None:
        return A
    if A[0] == Bp[0]:
        if f2_add(A[1], Bp[1]) == (0, 0):
            return None
        lam = f2_mul(f2_mul((3, 0), f2_mul(A[0], A[0])), f2_inv(f2_add(A[1], A[1])))
    else:
        lam = f2_mul(f2_sub(Bp[1], A[1]), f2_inv(f2_sub(Bp[0], A[0])))
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), A[0]), Bp[0])
    return x3, f2_sub(f2_mul(lam, f2_sub(A[0], x3)), A[1])


def neg(A):
    return None if A is None else (A[0], f2_neg(A[1]))


def mul(k: int, A):
    out = None
    while k:
        if k & 1:
            out = add(out, A)
        A = add(A, A)
        k >>= 1
    return out


# ------------------------------------------------------------------------------------------------- wire encode / decode
def fq_to_wire(v: int) -> np.ndarray:
    return int_to_limbs(v * C377.Rq % P, LQ)


def fq_from_wire(raw) -> int:
    return limbs_to_int(raw) * C377.Rq_inv % P


def f2_to_wire(v) -> np.ndarray:
    return np.concatenate([fq_to_wire(v[0]), fq_to_wire(v[1])])


def f2_from_wire(raw):
    raw = np.ascontiguousarray(raw, dtype=np.uint32).reshape(-1)
    return fq_from_wire(raw[:LQ]), fq_from_wire(raw[LQ:2 * LQ])


def encode_affine(A) -> np.ndarray:
    if A is None:
        return np.zeros(4 * LQ, np.uint32)
    return np.concatenate([f2_to_wire(A[0]), f2_to_wire(A[1])])


def decode_affine(raw):
    raw = np.ascontiguousarray(raw, dtype=np.uint32).reshape(-1)
    if not raw[:2 * LQ].any():
        return None
    return f2_from_wire(raw[:2 * LQ]), f2_from_wire(raw[2 * LQ:4 * LQ])


def encode_jacobian(A) -> np.ndarray:
    if A is None:
        return np.concatenate([f2_to_wire((1, 0)), f2_to_wire((1, 0)), f2_to_wire((0, 0))])
    return np.concatenate([f2_to_wire(A[0]), f2_to_wire(A[1]), f2_to_wire((1, 0))])


def _xyz(raw):
    raw = np.ascontiguousarray(raw, dtype=np.uint32).reshape(-1)
    assert raw.size == 6 * LQ
    return (f2_from_wire(raw[2 * LQ * i:2 * LQ * (i + 1)]) for i in range(3))


def decode_jacobian(raw):
    X, Y, Z = _xyz(raw)
    if Z == (0, 0):
        return None
    zi = f2_inv(Z)
    zi2 = f2_mul(zi, zi)
    return f2_mul(X, zi2), f2_mul(Y, f2_mul(zi2, zi))


def decode_homogeneous(raw):
    X, Y, Z = _xyz(raw)
    if Z == (0, 0):
        return None
    zi = f2_inv(Z)
    return f2_mul(X, zi), f2_mul(Y, zi)


def decode(raw, projective: bool = False):
    w = np.asarray(raw).view(np.uint32)
    return decode_homogeneous(w) if projective else decode_jacobian(w)


def scalar_to_wire(v: int) -> np.ndarray:
    """a scalar of BLS12-377 Fr (reduced mod r) as the 8 Montgomery-form words the MSM entry points take"""
    return int_to_limbs(v % R * C377.Rr % R, 8)


def msm(bases: np.ndarray, scalars: np.ndarray):
    """sum s_i B_i by scalar multiplications (slow: for tens of points)"""
    acc = None
    for b, s in zip(bases, scalars):
        A = decode_affine(b)
        if A is not None:
            acc = add(acc, mul(decode_scalar(C377, s), A))
    return acc
