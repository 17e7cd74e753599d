"""The XYZZ group law on stored points at the edges of its lazy-reduction contract (xyzz_vectors.py): the op table of
panda_amd/csrc/curve29_debug_ops.h compiled for the host with FE29_CHECK (tests/host_check/curve29_internal_host.cpp) against Python
big integers and the affine group law of pyref, and the device spelling of the same table -- the formulas of curve29.h on the asm
column chains, and the four-lane formulas of curve29_quad.h -- against that host twin (panda_debug_xyzz_internal).

Quad against sequential, limb for limb: ASSERTED.  Read from the code: xyzz_add_quad / xyzz_dbl_quad form the same products, sums and
differences as xyzz_add / xyzz_dbl (same fe_sub / fe_neg parameters, same operand order), with three spellings that differ: a square
is taken as fe_mul(a, a) instead of fe_sqr(a), ZZZ3 = zzz PPP (W ZZZ in the doubling) rides in an fe_mul_add whose second product is
0 * 0, and the products run in different lanes.  Every Montgomery product here (fe29.h: fe_mul, fe_sqr, fe_mul_add, host loops and
device chains alike) is product scanning: its quotient digits and output limbs are functions of the column sums alone, and the column
sums of a * a are those of fe_sqr(a) (cross terms once against the doubled operand), those of a b + 0 * 0 are those of a b.  The Fq2
products are built from these component by component in the same order (fe29_ext2.h).  So both spellings run the same products on the
same limbs, and the device quad result must equal the twin's sequential result bit for bit in all four lanes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import xyzz_vectors as xv

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "panda_amd", "csrc")
CASES = xv.cases()
OPS = xv.OPS


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("curve29_internal") / "libcurve29_internal_host.so")
    # -O0: six fields of fully inlined formulas compile in a third of the time -O1 takes, and the twin's run time does not matter
    subprocess.run(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_check", "curve29_internal_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.h29_xyzz_internal.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.h29_curve_bounds.argtypes = [C.c_uint, C.c_void_p]
    return lib


_CACHE = {}
_HOST = {}


def _case(cid, op):
    if (cid, op) not in _CACHE:
        _CACHE[(cid, op)] = xv.make_case(cid, op)
    return _CACHE[(cid, op)]


def _host(twin, cs):
    """the twin's output, computed once per (curve, op) and left unchanged"""
    key = (cs.cid, cs.op)
    if key not in _HOST:
        out = np.zeros((cs.n, xv.out_width(cs.cid, cs.op)), dtype=np.uint32)
        assert twin.h29_xyzz_internal(cs.cid, cs.op, _ptr(out), _ptr(cs.a), _ptr(cs.b), cs.n) == 0
        out.setflags(write=False)
        _HOST[key] = out
    return _HOST[key]


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_op_numbers_match_the_header():
    txt = open(os.path.join(CSRC, "curve29_debug_ops.h")).read()
    txt = txt[txt.index("enum Xyzz29DebugOp"):]
    txt = txt[: txt.index("};")]
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"XYZZ_DBG_([A-Z0-9_]+) = (\d+)", txt)}
    assert enum.pop("OPS") == len(OPS)
    assert enum == OPS


def test_python_bounds_match_the_header(twin):
    for cid in xv.CURVE_IDS:
        out = (C.c_int * 7)()
        assert twin.h29_curve_bounds(cid, out) == 0
        assert list(out) == xv.curve(cid).bounds(), (cid, list(out))
    assert twin.h29_curve_bounds(5, (C.c_int * 7)()) == 1


def test_unsupported_pairs_are_refused(twin):
    r = np.zeros(1024, dtype=np.uint32)
    for cid in range(8):
        for op in range(len(OPS) + 1):
            rc = twin.h29_xyzz_internal(cid, op, _ptr(r), _ptr(r), _ptr(r), 0)
            assert rc == (0 if xv.supported(cid, op) else 1), (cid, op)
    assert not r.any()
    assert len(CASES) == 13 + 5 * 12   # MADD_NEG_RAW exists exactly where RawOperandOk holds: BN254 G1


@pytest.mark.parametrize("cid,op", CASES, ids=[f"{c}-{xv.OP_NAMES[o]}" for c, o in CASES])
def test_host_twin_against_the_group_law(twin, cid, op):
    """no FE29_CHECK assert fires (one would end the process), and every output is the point the affine group law gives, in a
    representation that meets the stored-point contract: identity, rare and wire words exactly as expected"""
    cs = _case(cid, op)
    xv.check(cs, _host(twin, cs))


@pytest.mark.parametrize("cid", xv.CURVE_IDS)
def test_vectors_sit_at_the_top_of_every_bound(cid):
    """over sweep and top, every coordinate has a vector in the top p of its bound"""
    c = xv.curve(cid)
    for op in (OPS["MADD"], OPS["DBL"], OPS["ADD"], OPS["TO_JACOBIAN_WIRE"]):
        cs = _case(cid, op)
        arrays = [cs.a, cs.b] if op == OPS["ADD"] else [cs.a]
        for arr in arrays:
            for k, bound in enumerate((c.XB, c.YB, 2, 2)):
                hit = [False] * c.D
                for i in cs.where("sweep", "top"):
                    for d, v in enumerate(xv.split(c, arr[i], k)):
                        hit[d] |= (bound - 1) * c.p <= v < bound * c.p
                assert all(hit), (cid, xv.OP_NAMES[op], k)
    cs = _case(cid, OPS["MADD"])   # an affine base: tight, residue + p
    assert any(all(v >= c.p for k in (0, 1) for v in xv.split(c, cs.b[i], k)) for i in cs.where("sweep", "top"))


@pytest.mark.parametrize("cid", xv.CURVE_IDS)
def test_vectors_carry_loose_limbs(cid):
    """The loose copies are loose.  A stored X (fe_sub's output) and a seeded Y have limbs up to 2^29 + 8 in the kernels, and column sums
    and carries depend on that magnitude: for every op that takes a stored point, and for both operands of ADD, some vector has its X
    limbs and some vector its Y limbs AT 2^29 + 8 -- limbs 0 .. N-3 of every component, which is what every representative's range can
    hold (xyzz_vectors.loose_coord) -- and this in the sweep, top, same and opposite families alike; somewhere limb N-2 is there too."""
    c = xv.curve(cid)
    N = c.N

    def at_top(row, k, upto):
        return all(int(x) == xv.LOOSE for d in range(c.D) for x in row[k * c.W + d * N: k * c.W + d * N + upto])

    for op in range(len(OPS)):
        if not xv.supported(cid, op) or op == OPS["DBL_AFFINE"]:   # an affine base is tight by contract
            continue
        cs = _case(cid, op)
        families = ["sweep", "top"] + (["same", "opposite"] if op in xv.MADD_OPS + (OPS["ADD"], OPS["ADD_QUAD"]) else [])
        for arr in ([cs.a, cs.b] if op in (OPS["ADD"], OPS["ADD_QUAD"]) else [cs.a]):
            for fam in families:
                for k in (0, 1):
                    hits = [i for i in cs.where(fam) if at_top(arr[i], k, N - 2)]
                    assert len(hits) >= 2, (cid, xv.OP_NAMES[op], fam, "XY"[k])
            if c.F.P[-1] >= 1:   # a top limb of p below 1 (BLS12-377) leaves no room to choose limb N-2 inside one representative
                assert any(at_top(arr[i], k, N - 1) for k in (0, 1) for i in cs.where("sweep", "top")), (cid, xv.OP_NAMES[op])
        assert all(int(x) <= xv.TIGHT for i in range(cs.n) for kk in (2, 3) for d in range(c.D)
                   for x in cs.a[i][kk * c.W + d * N: kk * c.W + (d + 1) * N - 1])   # ZZ, ZZZ stay tight


@pytest.mark.parametrize("cid", xv.CURVE_IDS)
def test_trace_agrees_with_madd_core(twin, cid):
    """MADD_TRACE repeats the first lines of xyzz_madd_core (the hot function is not edited to export P, R, PP).  On the vectors the two ops
    share, the copy must tell the same story as the function: PP is 0 or p exactly where MADD_CORE returns rare != 0, and R is a multiple
    of p exactly where it returns 1."""
    c = xv.curve(cid)
    tr, co = _case(cid, OPS["MADD_TRACE"]), _case(cid, OPS["MADD_CORE"])
    assert (tr.a == co.a).all() and (tr.b == co.b).all()
    t, r = _host(twin, tr), _host(twin, co)
    seen = set()
    for i in range(tr.n):
        _, R, PP = (xv.split(c, t[i], k) for k in range(3))
        rare = int(r[i][4 * c.W])
        seen.add(rare)
        assert all(v in (0, c.p) for v in PP) == (rare != 0), (i, tr.family[i], rare)
        if rare:
            assert all(v % c.p == 0 for v in R) == (rare == 1), (i, tr.family[i], rare)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("cid", xv.CURVE_IDS)
def test_same_x_vectors_reach_every_multiple_of_p(twin, cid):
    """The reach proof covers the MIXED addition (xyzz_madd_core, the MSM's hot path) only: xyzz_add / xyzz_add_quad form P and R with
    fe_sub<F, 2>, whose three multiples (K2 - 1 to K2 + 1) their same / opposite families reach only as the products leave them.

    MADD_TRACE over the same-x families: P = U2 - X1 + KX p is a multiple of p there, and the vectors take it through EVERY multiple
    the bounds admit -- (KX - XB + 1) p [U2 = residue, X1 = residue + (XB - 1) p] to (KX + 1) p [U2 = residue + p, X1 = residue] --
    in every component; R = S2 - Y1 + KY p likewise from (KY - YB + 1) p to (KY + 1) p where the points are equal.  KX, KY are what
    fe_sub<F, XB> and fe_sub<F, YB> add (KEFF[XB + M], KEFF[YB + M]).

    PP = P^2 / R is seen as p only.  PP = 0 is structurally unreachable and is the one exclusion: a Montgomery product is 0 only for a
    zero operand [out = (T + q p) / R >= T / R > 0], and P = m p has m >= KX - XB + 1 >= M + 1 >= 1 because fe_sub's constant exceeds
    the bound of what it subtracts.  For T = m^2 p^2 the output is a multiple of p in (0, 2p): exactly p (Fq2: each component is a
    multiple k p, k >= 1, going into fe_reduce_small_2p, whose quotient estimate divides by more than p and so stays below k: p again).
    The `0` half of fe_is_zero_2p is therefore dead for PP; it is live for V = (2Y)^2 in the doublings, where the y0 family has Y = 0 p
    (V = 0) next to Y = j p (V = p)."""
    c = xv.curve(cid)
    cs = _case(cid, OPS["MADD_TRACE"])
    out = _host(twin, cs)
    p = c.p
    pm, rm = [set() for _ in range(c.D)], [set() for _ in range(c.D)]
    idx = cs.where(*xv.SAME_X_FAMILIES)
    assert len(idx) > 100
    for i in idx:
        P, R, PP = (xv.split(c, out[i], k) for k in range(3))
        for d in range(c.D):
            assert P[d] % p == 0 and PP[d] == p, (i, cs.family[i])
            pm[d].add(P[d] // p)
            if cs.expect[i] == "same":
                assert R[d] % p == 0
                rm[d].add(R[d] // p)
            elif c.D == 1:
                assert R[d] % p
    for d in range(c.D):
        assert pm[d] == set(range(c.KX - c.XB + 1, c.KX + 2)), (cid, d, sorted(pm[d]))
        assert rm[d] == set(range(c.KY - c.YB + 1, c.KY + 2)), (cid, d, sorted(rm[d]))
    assert c.KX + 2 == c.PB and c.KY + 2 == c.RB   # the top multiples are the last ones below PB p and RB p
    print(f"reach {xv.CURVE_NAMES[cid]}: P/p {min(pm[0])}..{max(pm[0])} of PB = {c.PB}, R/p {min(rm[0])}..{max(rm[0])} of RB = {c.RB}")
    dbl = _case(cid, OPS["DBL"])
    ys = {xv.split(c, dbl.a[i], 1) for i in dbl.where("y0")}
    assert any(v == 0 for y in ys for v in y) and any(all(v >= p for v in y) for y in ys)


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("cid", xv.CURVE_IDS, ids=[xv.CURVE_NAMES[c].replace(" ", "_") for c in xv.CURVE_IDS])
def test_device_matches_host_twin(twin, cid):
    """every op of the table on the device: bit for bit the host twin's limbs -- for the two quad ops in all four lanes (see the module
    docstring for why the four-lane spelling must give the sequential one's limbs) -- and the same group-law and contract checks"""
    from gpu_util import NULL_STREAM, DeviceBuffer

    from panda_amd import gpu_ffi as ffi

    lib = ffi.load()
    for c_, op in CASES:
        if c_ != cid:
            continue
        cs = _case(cid, op)
        want = _host(twin, cs)
        bufs = [DeviceBuffer.from_host(x) if x is not None else None for x in (cs.a, cs.b)]
        dr = DeviceBuffer(want.nbytes)
        try:
            ffi.check(lib.panda_debug_xyzz_internal(cid, op, dr.ptr, *[b.ptr if b else None for b in bufs], cs.n, NULL_STREAM), "op")
            got = dr.to_host().reshape(want.shape)
        finally:
            for b in bufs + [dr]:
                if b:
                    b.free()
        if not (got == want).all():
            i = int(np.nonzero((got != want).any(axis=1))[0][0])
            xv._fail(cs, i, f"device limbs {got[i].tolist()} differ from the host twin's {want[i].tolist()}")
        if op in xv.QUAD_OPS:
            xv.check(cs, got)   # lanes identical, residue, bounds: on the device's own output
    dr = DeviceBuffer(256)
    try:
        for op in range(len(OPS) + 1):
            if not xv.supported(cid, op):
                assert lib.panda_debug_xyzz_internal(cid, op, dr.ptr, dr.ptr, dr.ptr, 0, NULL_STREAM) == 1, op
        for bad in (5, 7):
            assert lib.panda_debug_xyzz_internal(bad, 0, dr.ptr, dr.ptr, dr.ptr, 0, NULL_STREAM) == 1
    finally:
        dr.free()
