"""The field arithmetic at the edges of its bounds contract, on internal-form limbs (fe29_vectors.py): the op table of
panda_amd/csrc/fe29_debug_ops.h compiled for the host with FE29_CHECK (tests/host_check/fe29_internal_host.cpp) against Python big
integers, and the device spelling of the same table -- the asm column chains of fe29_chain.h that the MSM and NTT kernels run --
against that host twin, bit for bit (panda_debug_fe_internal)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fe29_vectors as fv

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "panda_amd", "csrc")
CASES = fv.cases()


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fe29_internal") / "libfe29_internal_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_check", "fe29_internal_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.h29_fe_internal.argtypes = [C.c_uint, C.c_uint] + [C.c_void_p] * 5 + [C.c_size_t]
    return lib


_CACHE = {}


def _case(fid, op):
    if (fid, op) not in _CACHE:
        _CACHE[(fid, op)] = fv.make_case(fid, op)
    return _CACHE[(fid, op)]


def _host(twin, cs):
    out = np.zeros((cs.n, fv.out_width(cs.fid, cs.op)), dtype=np.uint32)
    assert twin.h29_fe_internal(cs.fid, cs.op, _ptr(out), _ptr(cs.a), _ptr(cs.b), _ptr(cs.c), _ptr(cs.d), cs.n) == 0
    return out


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_op_numbers_match_the_header():
    txt = open(os.path.join(CSRC, "fe29_debug_ops.h")).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"FE29_DBG_([A-Z0-9_]+) = (\d+)", txt)}
    assert enum.pop("OPS") == len(fv.OPS)
    assert enum == fv.OPS


def test_chain_header_is_current():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_chain.py")], check=True, capture_output=True, text=True).stdout
    assert out == open(os.path.join(CSRC, "fe29_chain.h")).read()


def test_python_constants_match_the_params_header():
    txt = open(os.path.join(CSRC, "fe29_params.h")).read()
    names = ["Bn254Fq", "Bn254Fr", "Bls377Fq", "Bls377Fr", "Bls381Fq", "Bls381Fr"]
    for fid, name in enumerate(names):
        F = fv.Field(fid)
        body = txt[txt.index(f"struct {name} {{"):]
        arr = lambda key: [int(x, 16) for x in re.search(key + r"\[\d+\] = \{([^}]*)\}", body).group(1).replace("u", "").split(",")]
        assert arr("P") == F.P and arr("PNEG") == F.PNEG
        kp = re.search(r"KP\[201\]\[\d+\] = \{(.*?)\};", body, re.S).group(1)
        rows = [[int(x, 16) for x in r.replace("u", "").split(",")] for r in re.findall(r"\{([^{}]*)\}", kp)]
        keff = [int(x) for x in re.search(r"KEFF\[201\] = \{([^}]*)\}", body).group(1).split(",")]
        for k in (3, 4, 8, 9, 16):
            assert rows[k] == F.kp_biased(k) and keff[k] == F.keff(k)


def test_unsupported_pairs_are_refused(twin):
    r = np.zeros(64, dtype=np.uint32)
    for fid in range(9):
        for op in range(len(fv.OPS) + 1):
            rc = twin.h29_fe_internal(fid, op, _ptr(r), _ptr(r), _ptr(r), _ptr(r), _ptr(r), 1)
            assert rc == (0 if fv.supported(fid, op) else 1), (fid, op)
    assert twin.h29_fe_internal(9, 0, _ptr(r), _ptr(r), _ptr(r), None, None, 1) == 1
    assert len(CASES) == 4 * 14 + 2 * 6 + 3 * 5  # 9-limb fields, 14-limb fields, Fq2


@pytest.mark.parametrize("fid,op", CASES, ids=[f"{f}-{fv.OP_NAMES[o]}" for f, o in CASES])
def test_host_twin_against_big_integers(twin, fid, op):
    cs = _case(fid, op)
    fv.check(cs, _host(twin, cs))


@pytest.mark.parametrize("fid", range(9))
def test_vectors_reach_past_canonical_columns(fid):
    """the largest column accumulator the field's vectors drive its products to is beyond every column canonical operands (tight,
    below 2p: what test_field_ops_elementwise hands the device through fe_from_wire) can reach"""
    F = fv.base_of(fid)
    peak = max(_case(f, o).peak for f, o in CASES if f == fid)
    assert peak > fv.canonical_column_bound(F), (fid, peak.bit_length())
    assert peak < 1 << 64


def test_column_model_sees_the_headroom_the_contract_spends():
    """the Montgomery product at its limb bounds, the shoup high columns and the un-normalised butterfly difference reach past 2^63:
    the bit a device chain could lose without any canonical operand noticing"""
    for op in ("MUL", "SHOUP", "SHOUP_UNIFORM", "BFLY3"):
        assert max(_case(f, fv.OPS[op]).peak for f in (0, 1, 3, 5)) >= 1 << 63, op


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("fid", range(9), ids=[fv.FIELD_NAMES[f].replace(" ", "_") for f in range(9)])
def test_device_matches_host_twin(twin, fid):
    from gpu_util import NULL_STREAM, DeviceBuffer

    from panda_amd import gpu_ffi as ffi

    lib = ffi.load()
    for f, op in CASES:
        if f != fid:
            continue
        cs = _case(fid, op)
        want = _host(twin, cs)
        bufs = [DeviceBuffer.from_host(x) if x is not None else None for x in (cs.a, cs.b, cs.c, cs.d)]
        dr = DeviceBuffer(want.nbytes)
        try:
            ffi.check(lib.panda_debug_fe_internal(fid, op, dr.ptr, *[b.ptr if b else None for b in bufs], cs.n, NULL_STREAM), "op")
            got = dr.to_host().reshape(want.shape)
        finally:
            for b in bufs + [dr]:
                if b:
                    b.free()
        if not (got == want).all():
            i = int(np.nonzero((got != want).any(axis=1))[0][0])
            fv._fail(cs, i, f"device limbs {got[i].tolist()} differ from the host twin's {want[i].tolist()}")
        fv.check(cs, got)
    dr = DeviceBuffer(256)
    try:
        for op in range(len(fv.OPS) + 1):
            if not fv.supported(fid, op):
                assert lib.panda_debug_fe_internal(fid, op, dr.ptr, dr.ptr, dr.ptr, dr.ptr, dr.ptr, 1, NULL_STREAM) == 1, op
        assert lib.panda_debug_fe_internal(9, 0, dr.ptr, dr.ptr, dr.ptr, None, None, 1, NULL_STREAM) == 1
    finally:
        dr.free()
