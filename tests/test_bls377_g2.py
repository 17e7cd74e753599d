"""BLS12-377 G2 (curve id 6): Fq2 = Fq[u] / (u^2 + 5) over the 14-limb field, the CPU and device MSM entry points, and what the built
code objects must satisfy (no scratch in the hot kernel; no function whose long branches go through its return address).  Everything is
pinned by the pure-Python twist arithmetic of pyref_bls377_g2.py; device results are checked against the linearity identity
sum s_i m_i G for bases m_i G from panda_gen_bases(6, ...)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as po
import pyref
import pyref_bls377_g2 as g2
from gpu_util import gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm
from panda_amd import multi_gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "panda_amd", "csrc")
CURVE = 6
P, R = g2.P, g2.R
NL = 14                      # 29-bit limbs of one Fq component
RINT = 1 << (29 * NL)        # Montgomery radix of the internal form
RINT_INV = pow(RINT, -1, P)
SYMBOLS = ["panda_msm_setup_bls12_377_g2", "panda_msm_execute_bls12_377_g2", "panda_msm_execute_bls12_377_g2_host", "panda_msm_combine_bls12_377_g2",
           "panda_msm_execute_bls12_377_g2_multi", "panda_msm_execute_bls12_377_g2_from_host_multi"]


# ------------------------------------------------------------------------------------------------- the Python reference
def test_reference_is_pinned():
    G = g2.GEN
    assert P % 4 == 1 and pow(P - 1, (P - 1) // 2, P) == 1        # -1 is a square: u^2 = -1 would not give a field
    assert pow(P - 5, (P - 1) // 2, P) == P - 1                    # -5 is not
    assert g2.f2_mul(g2.U, g2.U) == (g2.BETA, 0) == (P - 5, 0)
    assert g2.f2_mul(g2.B2, g2.U) == (1, 0)                        # b' = 1 / u
    assert g2.B2 == (0, 155198655607781456406391640216936120121836107652948796323930557600032281009004493664981332883744016074664192874906)
    assert g2.is_on_curve(G)
    assert g2.mul(R, G) is None
    assert g2.mul(R + 1, G) == G
    assert g2.add(g2.mul(5, G), g2.mul(7, G)) == g2.mul(12, G)
    assert g2.add(g2.mul(R - 1, G), G) is None
    assert g2.add(G, g2.neg(G)) is None
    A = g2.mul(0x1234567, G)
    assert g2.decode_affine(g2.encode_affine(A)) == A and g2.decode_affine(g2.encode_affine(None)) is None
    assert g2.decode_jacobian(g2.encode_jacobian(A)) == A and g2.decode_jacobian(g2.encode_jacobian(None)) is None


def test_python_constants_match_the_library_tables():
    assert pgm.BLS12_377_G2 == CURVE == g2.BLS12_377_G2
    assert pgm._POINT_BYTES[CURVE] == 192 and pgm._RESULT_BYTES[CURVE] == 288
    assert 5 not in pgm._POINT_BYTES and 5 not in pgm._RESULT_BYTES
    lib = ffi.load()
    for s in SYMBOLS:
        assert s in ffi.ADDITIVE_SYMBOLS and hasattr(lib, s)
    assert lib.panda_msm_setup_bls12_377_g2() == 0
    wb, ws = C.c_uint(0), C.c_uint(0)
    for k in (10, 16, 20):
        assert lib.panda_msm_plain_window_plan(CURVE, k, C.byref(wb), C.byref(ws)) == 0 and wb.value > 0 and ws.value > 0
        # the plan is keyed on the scalar field: BLS12-377 Fr, as for curve 1
        wb1, ws1 = C.c_uint(0), C.c_uint(0)
        assert lib.panda_msm_plain_window_plan(1, k, C.byref(wb1), C.byref(ws1)) == 0 and (wb.value, ws.value) == (wb1.value, ws1.value)
    assert lib.panda_msm_plain_window_plan(5, 16, C.byref(wb), C.byref(ws)) == 1
    assert lib.panda_msm_plain_window_plan(7, 16, C.byref(wb), C.byref(ws)) == 1


# ------------------------------------------------------------------------------------------------- Fq2 compiled for the host
@pytest.fixture(scope="module")
def h2(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe29_ext2_377") / "libfe29_ext2_377_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_check", "fe29_ext2_377_host.cpp")], check=True)
    return C.CDLL(so)


def _limbs(v: int, n=NL):
    return [(v >> (29 * i)) & ((1 << 29) - 1) if i < n - 1 else v >> (29 * i) for i in range(n)]


def _val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def _spread(v: int, k: int):
    """v in 14 limbs, each of limbs 0..12 carrying k extra units of 2^29 borrowed from the limb above (same value, wider limbs)"""
    l = _limbs(v)
    for i in range(NL - 1, 0, -1):
        t = min(k, l[i])
        l[i] -= t
        l[i - 1] += t << 29
    assert _val(l) == v
    return l


def _elems(vals, k=0):
    return np.array([_spread(a, k) + _spread(b, k) for a, b in vals], dtype=np.uint32).reshape(len(vals), 2 * NL)


def _from_internal(row):
    c0, c1 = _val(row[:NL]), _val(row[NL:])
    assert all(int(x) < (1 << 29) for i, x in enumerate(row) if i % NL != NL - 1), "not tight"
    assert c0 < 2 * P and c1 < 2 * P
    return c0 * RINT_INV % P, c1 * RINT_INV % P  # the element (Montgomery form, radix 2^406)


def _operands():
    rng = np.random.default_rng(0x377)
    vals = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1), (P - 1, P - 1), (RINT % P, 0), (0, RINT % P)]  # 0, raw 1, u, p - 1, Montgomery one / u
    vals += [(2 * P - 1, 2 * P - 1), (2 * P - 1, 0), (P, P)]          # tight operands at the top of [0, 2p)
    vals += [(int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) ** 4 % (2 * P),
              int(rng.integers(0, 1 << 62)) ** 7 % (2 * P)) for _ in range(200)]
    return vals


def test_fq2_mul_sqr_mul_add_inv_vs_python(h2):
    vals = _operands()
    n = len(vals)
    a = _elems(vals)
    b = _elems(list(reversed(vals)))
    a_wide = _elems(vals, 1)    # the same values with limbs just over 2^29 (loose: what fe_sub / fe_add hand to a product)
    r = np.empty_like(a)
    # internal limbs of value x stand for the element x / 2^406 (Montgomery form): products multiply elements; u^2 = -5 in g2.f2_mul
    el = lambda x: ((x[0] * RINT_INV) % P, (x[1] * RINT_INV) % P)
    ev = [el(x) for x in vals]
    rv = list(reversed(ev))
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p) if arr is not None else None
    for A in (a, a_wide):
        assert h2.h377_fq2_op(0, ptr(r), ptr(A), ptr(b), None, None, C.c_size_t(n)) == 0
        assert [_from_internal(row) for row in r] == [g2.f2_mul(x, y) for x, y in zip(ev, rv)]
        assert h2.h377_fq2_op(1, ptr(r), ptr(A), None, None, None, C.c_size_t(n)) == 0
        assert [_from_internal(row) for row in r] == [g2.f2_mul(x, x) for x in ev]
    c = _elems(vals[3:] + vals[:3], 1)
    d = _elems(vals[7:] + vals[:7])
    cv, dv = ev[3:] + ev[:3], ev[7:] + ev[:7]
    assert h2.h377_fq2_op(2, ptr(r), ptr(a_wide), ptr(b), ptr(c), ptr(d), C.c_size_t(n)) == 0
    assert [_from_internal(row) for row in r] == [g2.f2_add(g2.f2_mul(x, y), g2.f2_mul(z, w)) for x, y, z, w in zip(ev, rv, cv, dv)]
    # inverse (0 -> 0)
    assert h2.h377_fq2_op(3, ptr(r), ptr(a), None, None, None, C.c_size_t(n)) == 0
    for e, row in zip(ev, r):
        got = _from_internal(row)
        if e == (0, 0):
            assert got == (0, 0)
        else:
            assert g2.f2_mul(got, e) == (1, 0)


def test_c0_minus_five_t1_at_its_bound_edges(h2):
    """c0 = t0 - 5 t1 (fe29_ext2.h, ext2_c0) for tight t0, t1 up to 2p - 1 -- the largest t1 a product hands it, whose 5 t1 has limbs
    near 5 2^29 --, down to t0 = 0; output tight, below 2p and congruent"""
    rng = np.random.default_rng(0x5)
    edge = [0, 1, P - 1, P, 2 * P - 1, 2 * P - 2, (1 << 377) - 1, (1 << 377)]
    edge = [v for v in edge if v < 2 * P]
    tight_max = sum(((1 << 29) - 1) << (29 * i) for i in range(NL - 1)) + (((2 * P - 1) >> (29 * (NL - 1))) << (29 * (NL - 1)))
    if tight_max < 2 * P:
        edge.append(tight_max)  # every limb 2^29 - 1 below the top one
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(int.from_bytes(rng.bytes(48), "little") % (2 * P), int.from_bytes(rng.bytes(48), "little") % (2 * P)) for _ in range(500)]
    t0 = np.array([_limbs(a) for a, _ in pairs], dtype=np.uint32)
    t1 = np.array([_limbs(b) for _, b in pairs], dtype=np.uint32)
    assert (t1 * np.uint64(5))[:, :NL - 1].max() > 4 * (1 << 29)      # the subtrahend's limbs really reach past 2^31
    r = np.empty_like(t0)
    assert h2.h377_c0(r.ctypes.data_as(C.c_void_p), t0.ctypes.data_as(C.c_void_p), t1.ctypes.data_as(C.c_void_p), C.c_size_t(len(pairs))) == 0
    for (a, b), row in zip(pairs, r):
        assert all(int(x) < (1 << 29) for x in row[:NL - 1])
        out = _val(row)
        assert out < 2 * P and out % P == (a - 5 * b) % P


def test_reduce_small_2p_zero_top_limb(h2):
    """fe_reduce_small_2p over BLS12-377's Fq (top limb of p = 0: the two-limb quotient estimate against P[12] + 1): input limbs up
    to 2^32 - 1 and values up to just under 2^9 p; output tight, below 2p and congruent to the input."""
    rng = np.random.default_rng(0x2C)
    top = (1 << 9) * P - 1
    vals = [0, 1, P - 1, P, 2 * P - 1, 2 * P, top, top - P, (1 << 9) * P - (1 << 200), 511 * P + P - 1, 256 * P]
    vals += [18 * P - 1, 10 * P + 12345]  # what ext2_c0 hands it
    vals += [int.from_bytes(rng.bytes(49), "little") % top for _ in range(3000)]
    rows = []
    for v in vals:
        rows.append(_spread(v, 7))  # limbs 0..12 near 2^32 wherever the value leaves units to borrow
    a = np.array(rows, dtype=np.uint32)
    assert a[:, :NL - 1].max() > (1 << 31) + (1 << 30)
    r = np.empty_like(a)
    assert h2.h377_reduce_small_2p(r.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), C.c_size_t(len(vals))) == 0
    for v, row in zip(vals, r):
        assert all(int(x) < (1 << 29) for x in row[:NL - 1])
        out = _val(row)
        assert out < 2 * P and out % P == v % P


# ------------------------------------------------------------------------------------------------- the CPU entry point
def _host_case():
    rng = np.random.default_rng(0x64)
    n = 64
    mult = [int(v) for v in rng.integers(1, 1 << 62, n)]
    pts = [g2.mul(m, g2.GEN) for m in mult]
    pts[7] = None                                  # identity base (x == 0 on the wire)
    pts[9] = pts[8]                                # repeated point
    pts[11] = g2.neg(pts[10])                      # P, -P
    bases = np.stack([g2.encode_affine(A) for A in pts])
    scalars = po.gen_scalars(po.F_BLS377_FR, 0x65, n)
    for i, v in enumerate([0, 1, R - 1, 2, (1 << 252) + 12345]):
        scalars[20 + i] = g2.scalar_to_wire(v)
    scalars[9] = scalars[8]
    scalars[11] = scalars[10]
    scalars[30] = scalars[31] = g2.scalar_to_wire(3)  # a repeated point with a repeated scalar
    bases[31] = bases[30]
    return bases, scalars


def test_host_entry_point_vs_python_reference():
    bases, scalars = _host_case()
    want = g2.msm(bases, scalars)
    assert want is not None
    out = pgm.panda_msm_bn254_gpu_host(None, scalars, bases, curve=pgm.BLS12_377_G2)
    assert out.size == 288
    assert g2.decode(out) == want
    lib = ffi.load()
    hom = np.zeros(288, np.uint8)
    cfg = ffi.MSMConfiguration(ffi.PandaMemPool(), ffi.PandaStream(), C.c_void_p(bases.ctypes.data), C.c_void_p(scalars.ctypes.data),
                               C.c_void_p(hom.ctypes.data), 6, pgm.PROJECTIVE)
    ffi.check(lib.panda_msm_execute_bls12_377_g2_host(cfg), "host")
    assert g2.decode(hom, projective=True) == want
    halves = np.stack([pgm.panda_msm_bn254_gpu_host(None, scalars[h * 32:(h + 1) * 32], bases[h * 32:(h + 1) * 32], curve=pgm.BLS12_377_G2).view(np.uint32)
                       for h in range(2)])
    assert g2.decode(multi_gpu.combine_partials(halves, curve=pgm.BLS12_377_G2)) == want
    assert g2.decode(multi_gpu.combine_partials(halves, curve=pgm.BLS12_377_G2, coordinate_type=pgm.PROJECTIVE), projective=True) == want


# ------------------------------------------------------------------------------------------------- the built code objects
def _tool(name):
    p = os.path.join("/opt/rocm/llvm/bin", name)
    return p if os.path.exists(p) else shutil.which(name)


def _device_object(obj, tmp_path):
    objdump = _tool("llvm-objdump")
    assert objdump and _tool("llvm-readelf"), "llvm-objdump / llvm-readelf of the ROCm toolchain not found"
    assert os.path.exists(obj), "build the library first"
    local = tmp_path / os.path.basename(obj)
    shutil.copy(obj, local)
    subprocess.run([objdump, "--offloading", str(local)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if f.startswith(os.path.basename(obj)) and f.endswith("gfx950")]
    assert len(dev) == 1, os.listdir(tmp_path)
    return tmp_path / dev[0]


def _kernel_notes(code_object):
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", str(code_object)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s*- \.", notes):
        m = re.search(r"\.name:\s+(\S+)", block)
        if not m or ".kernarg_segment_size" not in block:
            continue
        kernels[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\s*$", "." + block, flags=re.M)}
    return kernels


def test_accumulate_kernel_has_no_scratch(tmp_path):
    """the one k_accumulate of the BLS12-377 G2 translation unit (its one shipped shape) runs without scratch.  ROCm 7.2 reports a
    handful of spilled VGPRs for it (8), held in AGPRs, not in memory: the same kernel built with BLS12-381's u^2 = -1 arithmetic over
    BLS12-377's Fq reports 12, so they come from the base field's product, not from the -5 (profiles/r08_bls377_g2.txt).  The bound
    keeps that from growing unnoticed."""
    kernels = _kernel_notes(_device_object(os.path.join(CSRC, "msm_bls377g2.o"), tmp_path))
    acc = {k: v for k, v in kernels.items() if "k_accumulate" in k}
    assert len(acc) == 1, sorted(kernels)  # no PERSIST / LDS-row / sector / shared-row variants for this field
    for name, f in acc.items():
        assert "Bls377Fq" in name
        assert f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_spill_count"] <= 8, (name, f)
        assert f["vgpr_count"] <= 512, (name, f)


@pytest.mark.parametrize("obj", ["msm_bls377g2.o", "debug_gen.o"])
def test_no_function_branches_through_its_return_address(obj, tmp_path):
    """A device FUNCTION (not a kernel) returns through s[30:31].  A long-branch expansion that loads its target into s[30:31]
    (s_getpc_b64 s[30:31]) overwrites the return address, and the function's return then jumps back into its own body: the call never
    returns.  hipcc did this to the out-of-line Fq2 point addition when it carried the doubling inline (curve29.h, OutlineRareDoubling)."""
    co = _device_object(os.path.join(CSRC, obj), tmp_path)
    kernels = set(_kernel_notes(co))
    dis = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", str(co)], check=True, capture_output=True, text=True).stdout
    bad, functions = [], 0
    for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        if name in kernels:
            continue
        functions += 1
        if re.search(r"s_getpc_b64 s\[30:31\]", body):
            bad.append(name)
    assert functions > 0
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- on the device
def _expected(seed_b, scalars, first=0):
    k = pyref.limbs_to_int(po.linear_combination(po.BLS12_377, seed_b, scalars, first))
    return g2.mul(k, g2.GEN)


def _device_bases(seed, n, first=0):
    from gpu_util import NULL_STREAM, DeviceBuffer
    db = DeviceBuffer(n * 192)
    ffi.check(ffi.load().panda_gen_bases(CURVE, seed, first, n, db.ptr, NULL_STREAM), "gen")
    bases = db.to_host().reshape(n, 48)
    db.free()
    return bases


@pytest.mark.gpu
def test_device_generator_and_group_law_vs_python():
    """panda_gen_bases(6) = m_i G; panda_debug_curve_op(6, ops 0..4) against affine arithmetic, with P + P, P + (-P) and the identity"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    lib = ffi.load()
    n = 24
    bases = _device_bases(0xC2, n, first=3)
    pts = [g2.decode_affine(b) for b in bases]
    for i in range(n):
        assert pts[i] == g2.mul(po.gen_multiplier(0xC2, 3 + i), g2.GEN)
        assert g2.is_on_curve(pts[i])
    one = g2.f2_to_wire((1, 0))
    jac = np.stack([np.concatenate([b, one]) for b in bases])
    other = _device_bases(0xC3, n)
    opts = [g2.decode_affine(b) for b in other]
    negb = np.stack([g2.encode_affine(g2.neg(A)) for A in pts])
    negj = np.stack([np.concatenate([b, one]) for b in negb])
    ident = np.zeros_like(jac)
    ident[:, :24] = one
    ident[:, 24:48] = one
    zero_base = other.copy()
    zero_base[::5, :24] = 0

    def run(op, A, B):
        dA, dB, dR = DeviceBuffer.from_host(A), DeviceBuffer.from_host(B), DeviceBuffer(n * 288)
        ffi.check(lib.panda_debug_curve_op(CURVE, op, dR.ptr, dA.ptr, dB.ptr, n, NULL_STREAM), "op")
        r = dR.to_host().reshape(n, 72)
        for d in (dA, dB, dR):
            d.free()
        return [g2.decode_jacobian(x) for x in r]

    assert run(0, jac, other) == [g2.add(p, q) for p, q in zip(pts, opts)]
    assert run(0, jac, bases) == [g2.add(p, p) for p in pts]
    assert run(0, jac, negb) == [None] * n
    assert run(0, ident, other) == opts
    assert run(0, jac, zero_base) == [p if i % 5 == 0 else g2.add(p, q) for i, (p, q) in enumerate(zip(pts, opts))]
    ojac = np.stack([np.concatenate([b, one]) for b in other])
    for op in (1, 3):  # full addition, and its four-lane spelling
        assert run(op, jac, ojac) == [g2.add(p, q) for p, q in zip(pts, opts)]
        assert run(op, jac, jac) == [g2.add(p, p) for p in pts]
        assert run(op, jac, negj) == [None] * n
        assert run(op, ident, ojac) == opts and run(op, jac, ident) == pts
    for op in (2, 4):  # doubling, and its four-lane spelling
        assert run(op, jac, jac) == [g2.add(p, p) for p in pts]
        assert run(op, ident, ident) == [None] * n


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 5, 10, 14, 16, pytest.param(18, marks=pytest.mark.gpu_soak), pytest.param(20, marks=pytest.mark.gpu_soak)])
def test_msm_sizes_both_coordinates(gm, k):
    """the device MSM against the linearity identity in both coordinate systems; the CPU entry point agrees at the small sizes"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    lib = ffi.load()
    n = 1 << k
    db, ds, dr = DeviceBuffer(n * 192), DeviceBuffer(n * 32), DeviceBuffer(288)
    try:
        ffi.check(lib.panda_gen_bases(CURVE, 0xD000 + k, 0, n, db.ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_gen_scalars(CURVE, 0xD100 + k, 0, n, ds.ptr, NULL_STREAM), "gen")
        scalars = ds.to_host().reshape(n, 8)
        want = _expected(0xD000 + k, scalars)
        for coord in (pgm.JACOBIAN, pgm.PROJECTIVE):
            cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, db.ptr, ds.ptr, dr.ptr, k, coord)
            ffi.check(lib.panda_msm_execute_bls12_377_g2(cfg), "msm")
            assert g2.decode(dr.to_host(np.uint8), coord == pgm.PROJECTIVE) == want
        assert (ds.to_host().reshape(n, 8) == scalars).all()  # the scalars are never modified
        if k <= 5:  # the CPU entry point: the same affine point (bucket order follows wave scheduling, so raw bytes may differ)
            bases = db.to_host().reshape(n, 48)
            assert g2.decode(pgm.panda_msm_bn254_gpu_host(gm, scalars, bases, curve=pgm.BLS12_377_G2)) == want
    finally:
        for d in (db, ds, dr):
            d.free()


@pytest.mark.gpu
def test_msm_staging_path_edges_and_gpu_vs_cpu(gm):
    """the manager's staging path with identity bases, P / -P, repeated points and edge scalars; GPU and CPU entry points agree"""
    bases, scalars = _host_case()
    want = g2.msm(bases, scalars)
    out = pgm.panda_msm_bn254_gpu(gm, scalars, bases, curve=pgm.BLS12_377_G2)
    assert out.size == 288 and g2.decode(out) == want
    assert g2.decode(pgm.panda_msm_bn254_gpu_host(gm, scalars, bases, curve=pgm.BLS12_377_G2)) == want


@pytest.mark.gpu
def test_msm_tables_registered_and_from_host(gm):
    """registered bases, precomputed tables (tables x n x 192 bytes held, as for the G1 curves), and the upload pipeline at 2 and 4
    ranges: the same point"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    lib = ffi.load()
    k = 16
    n = 1 << k
    db, ds, dr = DeviceBuffer(n * 192), DeviceBuffer(n * 32), DeviceBuffer(288)
    ffi.check(lib.panda_gen_bases(CURVE, 0xD300, 0, n, db.ptr, NULL_STREAM), "gen")
    ffi.check(lib.panda_gen_scalars(CURVE, 0xD301, 0, n, ds.ptr, NULL_STREAM), "gen")
    scalars = np.ascontiguousarray(ds.to_host().reshape(n, 8))
    want = _expected(0xD300, scalars)
    cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, db.ptr, ds.ptr, dr.ptr, k, pgm.JACOBIAN)
    try:
        ffi.check(lib.panda_msm_register_bases(CURVE, db.ptr, k, gm.exec_stream.raw), "register")
        ffi.check(lib.panda_msm_execute_bls12_377_g2(cfg), "msm")
        assert g2.decode(dr.to_host(np.uint8)) == want
        tables, bits, held = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
        ffi.check(lib.panda_msm_registered_info(db.ptr, C.byref(tables), C.byref(bits), C.byref(held)), "info")
        assert tables.value == 1 and held.value == n * 192
        ffi.check(lib.panda_msm_unregister_bases(db.ptr), "unregister")
        ffi.check(lib.panda_msm_precompute_bases(CURVE, db.ptr, k, 0, gm.exec_stream.raw), "precompute")
        ffi.check(lib.panda_msm_registered_info(db.ptr, C.byref(tables), C.byref(bits), C.byref(held)), "info")
        assert tables.value >= 2 and bits.value > 0 and held.value == tables.value * n * 192
        ffi.check(lib.panda_msm_execute_bls12_377_g2(cfg), "msm")
        assert g2.decode(dr.to_host(np.uint8)) == want
        for ranges in (2, 4):
            ffi.check(lib.panda_memset(ds.ptr, 0, n * 32), "memset")
            ffi.check(lib.panda_memset(dr.ptr, 0, 288), "memset")
            ffi.check(lib.panda_msm_execute_from_host(CURVE, cfg, C.c_void_p(scalars.ctypes.data), ranges, gm.h2d_stream.raw), "msm")
            assert g2.decode(dr.to_host(np.uint8)) == want
    finally:
        lib.panda_msm_unregister_bases(db.ptr)
        for d in (db, ds, dr):
            d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 4])
def test_multi_loopback(ranks):
    """panda_msm_execute_bls12_377_g2_multi and _from_host_multi on `ranks` loopback ranks of device 0: 288-byte partials, one point"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    lib = ffi.load()
    k = 12
    n, per, lk = 1 << k, (1 << k) // ranks, k - (ranks.bit_length() - 1)
    mg = multi_gpu.MultiGpu([0] * ranks, ffi.MULTI_LOOPBACK)
    bufs = []
    try:
        db, ds = DeviceBuffer(n * 192), DeviceBuffer(n * 32)
        res = [DeviceBuffer(288) for _ in range(ranks)]
        staging = [DeviceBuffer(per * 32) for _ in range(ranks)]
        bufs += [db, ds] + res + staging
        ffi.check(lib.panda_gen_bases(CURVE, 0xD500 + ranks, 0, n, db.ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_gen_scalars(CURVE, 0xD600 + ranks, 0, n, ds.ptr, NULL_STREAM), "gen")
        scalars = np.ascontiguousarray(ds.to_host().reshape(n, 8))
        want = _expected(0xD500 + ranks, scalars)
        for coord in (pgm.JACOBIAN, pgm.PROJECTIVE):
            cfgs = [ffi.MSMConfiguration(ffi.PandaMemPool(), ffi.PandaStream(), C.c_void_p(db.ptr.value + r * per * 192), C.c_void_p(ds.ptr.value + r * per * 32),
                                         res[r].ptr, lk, coord) for r in range(ranks)]
            total = mg.msm(cfgs, curve=CURVE)
            assert total.size == 288 and g2.decode(total, coord == pgm.PROJECTIVE) == want
        cfgs = [ffi.MSMConfiguration(ffi.PandaMemPool(), ffi.PandaStream(), C.c_void_p(db.ptr.value + r * per * 192), staging[r].ptr, res[r].ptr, lk, pgm.JACOBIAN)
                for r in range(ranks)]
        total = mg.msm_from_host(cfgs, [scalars.ctypes.data + r * per * 32 for r in range(ranks)], 2, curve=CURVE)
        assert total.size == 288 and g2.decode(total) == want
    finally:
        mg.close()
        for d in bufs:
            d.free()


@pytest.mark.gpu
def test_bad_arguments_return_an_error(gm):
    """curve id 5 stays unused, and buffers shorter than log_n implies for id 6 are refused with 1, never read past"""
    from gpu_util import NULL_STREAM, DeviceBuffer
    lib = ffi.load()
    d = DeviceBuffer(4096)
    big = DeviceBuffer(1 << 16)
    small = DeviceBuffer(256)
    try:
        assert lib.panda_msm_precompute_bases(CURVE, d.ptr, 10, 0, gm.exec_stream.raw) == 1      # 2^10 x 192 B > 4 KiB
        assert lib.panda_msm_register_bases(CURVE, d.ptr, 10, gm.exec_stream.raw) == 1
        for bad in (5, 7):
            assert lib.panda_msm_register_bases(bad, d.ptr, 2, gm.exec_stream.raw) == 1
            assert lib.panda_msm_precompute_bases(bad, d.ptr, 2, 0, gm.exec_stream.raw) == 1
            assert lib.panda_gen_bases(bad, 1, 0, 4, d.ptr, NULL_STREAM) == 1
            assert lib.panda_gen_scalars(bad, 1, 0, 4, d.ptr, NULL_STREAM) == 1
            assert lib.panda_debug_curve_op(bad, 0, d.ptr, d.ptr, d.ptr, 1, NULL_STREAM) == 1
            cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, d.ptr, d.ptr, d.ptr, 2, pgm.JACOBIAN)
            assert lib.panda_msm_execute_from_host(bad, cfg, None, 1, gm.h2d_stream.raw) == 1
        mk = lambda b, s, r, k: ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, b.ptr, s.ptr, r.ptr, k, pgm.JACOBIAN)
        assert lib.panda_msm_execute_bls12_377_g2(mk(d, big, big, 5)) == 1      # bases: 2^5 x 192 B = 6 KiB > 4 KiB
        assert lib.panda_msm_execute_bls12_377_g2(mk(big, d, big, 8)) == 1      # scalars: 2^8 x 32 B = 8 KiB > 4 KiB
        assert lib.panda_msm_execute_bls12_377_g2(mk(big, big, small, 4)) == 1  # result: 288 B > 256 B
        assert lib.panda_msm_execute_from_host(CURVE, mk(d, big, big, 5), None, 1, gm.h2d_stream.raw) == 1
        assert lib.panda_msm_execute_bls12_377_g2(ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, None, d.ptr, d.ptr, 2, pgm.JACOBIAN)) == 1
    finally:
        for b in (d, big, small):
            b.free()
