"""The signed-limb field operations (panda_amd/csrc/fe29.h, "Signed contract") and the signed mixed addition
(curve29.h, xyzz_madd_core_s) compiled for the HOST with FE29_CHECK -- a wide signed shadow of every column accumulator, asserts
on every limb class -- and run as a program of its own (tests/host_check/fe29_signed_host.cpp).  Operands sit at the edges of
the contract; every result is compared with Python's integers mod p.  BN254 Fq: the one field that takes the signed code."""
import os
import subprocess

import numpy as np
import pytest

import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_check", "fe29_signed_host.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "panda_amd", "csrc")

C = pyref.CURVES[pyref.BN254]
P = C.p
N, W = 9, 29
R = 1 << (N * W)
SLIMB_MAX = (1 << 29) + 16
TOPS = [-SLIMB_MAX, SLIMB_MAX, 0, -(1 << 25), 1 << 25]            # both ends of the stated range, and where real values sit
EDGES = [-3, 0, (1 << 29) - 1, (1 << 29) + 1, -SLIMB_MAX, SLIMB_MAX]  # lower limbs: the classes' edges and the contract's own


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fe29_signed") / "fe29_signed_host")
    # FE29_SIGNED_HOST_FLAGS="-fsanitize=address,undefined -fno-sanitize-recover=all" runs the whole module under the sanitizers: the
    # program is stand-alone host code, so signed overflow is then caught by the tool and not only by the shadow accumulator
    extra = os.environ.get("FE29_SIGNED_HOST_FLAGS", "").split()
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", *extra, "-o", exe, SRC], check=True)

    def run(op, records):
        d = os.path.dirname(exe)
        a = np.ascontiguousarray(np.array(records, dtype=np.int64).astype(np.int32))
        a.tofile(os.path.join(d, "in.bin"))
        r = subprocess.run([exe, op, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, f"{op}: {r.stderr[-2000:]}"
        return np.fromfile(os.path.join(d, "out.bin"), dtype=np.int32).astype(object)

    return run


def val(limbs):
    return sum(int(l) << (W * i) for i, l in enumerate(limbs))


def s_tight(v):
    """the one s-tight representation of a signed integer"""
    return [(v >> (W * i)) & ((1 << W) - 1) for i in range(N - 1)] + [v >> (W * (N - 1))]


def s_loose(v, shift):
    """the same value with every lower limb moved by -shift (shift = 3: limbs from -3; shift = -1: limbs up to 2^29)"""
    off = sum(shift << (W * i) for i in range(N - 1))
    t = s_tight(v + off)
    return [l - shift for l in t[:-1]] + [t[-1]]


def pairs_at_edges():
    out = []
    for ea in EDGES:
        for eb in EDGES:
            for ta in TOPS:
                for tb in TOPS:
                    out.append(([ea] * (N - 1) + [ta], [eb] * (N - 1) + [tb]))
    return out


def randoms(rng, n):
    out = []
    for i in range(n):
        if i % 2:
            out.append([int(x) for x in rng.integers(-SLIMB_MAX, SLIMB_MAX + 1, N)])
        else:  # what the addition feeds in: a value within a few p, s-tight
            out.append(s_tight(int.from_bytes(rng.bytes(34), "little") % (16 * P) - 8 * P))
    return out


def check_product(got, T):
    """s-tight, congruent to T / R, and within [T / R, T / R + p): the quotient m is in [0, R)"""
    assert all(0 <= int(l) < (1 << W) for l in got[:-1])
    v = val(got)
    assert (v * R - T) % P == 0
    assert T <= v * R < T + P * R


def test_fe_mul_s(prog):
    rng = np.random.default_rng(1)
    ops = pairs_at_edges() + list(zip(randoms(rng, 3000), randoms(rng, 3000)))
    zero = [0] * N
    out = prog("mul", [a + b + zero + zero for a, b in ops]).reshape(-1, N)
    for (a, b), r in zip(ops, out):
        check_product(r, val(a) * val(b))


def test_fe_sqr_s(prog):
    rng = np.random.default_rng(2)
    ops = [a for a, _ in pairs_at_edges()[:: len(TOPS)]] + randoms(rng, 3000)
    ops += [[e if i % 2 else -e for i in range(N)] for e in (SLIMB_MAX, (1 << 29) - 1)]  # alternating signs: the cross terms cancel least
    zero = [0] * N
    out = prog("sqr", [a + zero + zero + zero for a in ops]).reshape(-1, N)
    for a, r in zip(ops, out):
        check_product(r, val(a) ** 2)


def test_fe_mul_add_s(prog):
    rng = np.random.default_rng(3)
    hi, lo = [SLIMB_MAX] * N, [-SLIMB_MAX] * N
    ops = [(hi, hi, hi, hi), (lo, lo, lo, lo), (hi, lo, hi, lo), (lo, hi, hi, lo), (hi, lo, lo, lo)]  # all four at their limits at once
    e = pairs_at_edges()
    ops += [(a, b, c, d) for (a, b), (c, d) in zip(e, e[::-1])]
    ra, rb, rc, rd = (randoms(rng, 3000) for _ in range(4))
    ops += list(zip(ra, rb, rc, rd))
    out = prog("muladd", [a + b + c + d for a, b, c, d in ops]).reshape(-1, N)
    for (a, b, c, d), r in zip(ops, out):
        check_product(r, val(a) * val(b) + val(c) * val(d))


def test_fe_sub_s_and_norm_s(prog):
    rng = np.random.default_rng(4)
    zero = [0] * N
    cls = [-3, 0, (1 << 29) - 1, 1 << 29]  # s-tight and s-loose lower limbs
    ops = [([ea] * (N - 1) + [ta], [eb] * (N - 1) + [tb]) for ea in cls for eb in cls for ta in TOPS[2:] for tb in TOPS[2:]]
    ops += [(s_loose(int(rng.integers(-8, 8)) * P + int.from_bytes(rng.bytes(31), "little"), 3), s_tight(int.from_bytes(rng.bytes(32), "little"))) for _ in range(2000)]
    out = prog("sub", [a + b + zero + zero for a, b in ops]).reshape(-1, N)
    for (a, b), r in zip(ops, out):
        assert [int(x) for x in r] == [x - y for x, y in zip(a, b)]  # exactly the difference: no multiple of p
    wide = [-3 << 29, -(1 << 29) - 1, -1, 0, (1 << 29) - 1, 1 << 29, (1 << 30) - 1]
    ins = [[e] * (N - 1) + [t] for e in wide for t in TOPS[2:]]
    ins += [[int(x) for x in rng.integers(-3 << 29, 1 << 30, N - 1)] + [int(rng.integers(-(1 << 25), 1 << 25))] for _ in range(2000)]
    out = prog("norm", [a + zero + zero + zero for a in ins]).reshape(-1, N)
    for a, r in zip(ins, out):
        assert val(r) == val(a)
        assert all(-3 <= int(l) < (1 << 29) + 1 for l in r[:-1])


@pytest.mark.parametrize("K,lo,hi", [(4, -3.5, 4.4), (1, -0.5, 2.0)])
def test_fe_from_signed(prog, K, lo, hi):
    """what a reader of a stored signed accumulator does: + K p, one carry pass -> non-negative loose limbs, the value raised by K p"""
    rng = np.random.default_rng(5 + K)
    zero = [0] * N
    lo_v, hi_v = int(lo * P) + 1, int(hi * P) - 1
    vals = [lo_v, hi_v, 0, -1, 1, -P, P] + [lo_v + int.from_bytes(rng.bytes(40), "little") % (hi_v - lo_v) for _ in range(2000)]
    vals = [v for v in vals if lo_v <= v <= hi_v]
    ins = [s_tight(v) for v in vals] + [s_loose(v, 3) for v in vals] + [s_loose(v, -1) for v in vals]
    out = prog(f"unsign{K}", [a + zero + zero + zero for a in ins]).reshape(-1, N)
    for a, r in zip(ins, out):
        assert val(r) == val(a) + K * P
        assert all(0 <= int(l) <= (1 << 29) + 8 for l in r[:-1]) and int(r[-1]) >= 0


def test_fe_is_zero_mod_p_s(prog):
    rng = np.random.default_rng(8)
    zero = [0] * N
    vals = [k * P for k in range(-15, 16)] + [k * P + d for k in range(-15, 16) for d in (-1, 1)]
    vals += [int.from_bytes(rng.bytes(33), "little") % (30 * P) - 15 * P for _ in range(500)]
    ins = [s_tight(v) for v in vals] + [s_loose(v, 3) for v in vals]
    out = prog("zero", [a + zero + zero + zero for a in ins])
    for a, r in zip(ins, out):
        assert int(r) == (1 if val(a) % P == 0 else 0)


def _affine(pt):
    """(X, Y, ZZ, ZZZ) of 9 limbs each, signed or not -> affine ints, None for ZZ == 0.  The internal form's radix cancels in X / ZZ."""
    X, Y, ZZ, ZZZ = (val(pt[N * i: N * i + N]) for i in range(4))
    if ZZ == 0:
        return None
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


def test_signed_madd_chains(prog):
    """xyzz_madd_core_s beside xyzz_madd_core over chains of mixed additions, compared in affine form with each other and with affine
    arithmetic at every step: random rows with half of them negated (p - y), a chain seeded from a negated row, rows equal to the
    running sum (the doubling path) and opposite to it (identity mid-chain), identity rows, and additions on top of the doubled state.
    The program asserts the limb classes of every signed accumulator; the value bounds of SignedBounds are asserted here."""
    rng = np.random.default_rng(9)
    step = pyref.ec_mul(C, 0x1234567, C.g)
    pts, cur = [], pyref.ec_mul(C, 0xABCDEF12345, C.g)
    for _ in range(700):
        pts.append(cur)
        cur = pyref.ec_add(C, cur, step)
    rows, want, run = [], [], None

    def push(pt):
        nonlocal run
        rows.append(pt)
        run = pyref.ec_add(C, run, pt)
        want.append(run)

    neg = lambda pt: (pt[0], P - pt[1])
    it = iter(pts)
    push(neg(next(it)))                    # seeded from a negated row
    for i in range(650):
        pt = next(it)
        if i % 97 == 40:
            push(run)                      # the row is the running sum: P + P
            push(next(it))                 # and an addition on top of the doubled state
            push(neg(next(it)))
        elif i % 97 == 80:
            push(neg(run))                 # P + (-P): the identity mid-chain; the next row seeds the accumulator again
            push(None)                     # an identity row meets an identity accumulator
            push(neg(next(it)))
        elif i % 53 == 7:
            push(None)
        elif i % 61 == 9:
            push(pt)
            push(pt)                       # first row of a run twice: doubling right after the seed
        else:
            push(neg(pt) if rng.integers(0, 2) else pt)
    enc = lambda v: s_tight(v * R % P)
    recs = [[0] * (2 * N) if pt is None else enc(pt[0]) + enc(pt[1]) for pt in rows]
    out = prog("chain", recs).reshape(len(rows), 3, 4 * N)
    for k, (s, u, c) in enumerate(out):
        assert _affine(s) == want[k], f"step {k}: the signed chain differs from affine arithmetic"
        assert _affine(u) == want[k], f"step {k}: the unsigned chain differs from affine arithmetic"
        assert _affine(c) == want[k], f"step {k}: the converted accumulator differs from affine arithmetic"
        if want[k] is None:
            continue
        X, Y, ZZ, ZZZ = (val(s[N * i: N * i + N]) for i in range(4))
        assert -3.2 * P < X < 4.4 * P and abs(Y) < 2 * P and 0 < ZZ < 2 * P and abs(ZZZ) < 2 * P
        cX, cY, cZZ, cZZZ = (val(c[N * i: N * i + N]) for i in range(4))
        assert 0 <= cX < 9 * P and 0 <= cY < 3 * P and cZZ == ZZ and 0 <= cZZZ < 3 * P  # the stored invariants of curve29.h
