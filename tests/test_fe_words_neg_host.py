"""fe_words_neg (panda_amd/csrc/fe29.h): p - y on the packed 32-bit words of a canonical y -- what k_accumulate does to the y of a
table row under a negative digit before it unpacks the row.  A stand-alone host program (tests/host_check/fe_words_neg_host.cpp) is
compiled with g++ (the portable borrow chain) and, where the ROCm clang is installed, with that too (the subtract-with-borrow builtin
the device code of the wider fields is made from), and checked against Python integers: the result is p - y exactly, and fe_unpack
makes tight limbs of it."""
import os
import subprocess

import numpy as np
import pytest

import oracle as po
import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_check", "fe_words_neg_host.cpp")
ROCM_CLANG = "/opt/rocm/llvm/bin/clang++"
FIELDS = {0: ("BN254 Fq", 9), 1: ("BN254 Fr", 9), 2: ("BLS12-377 Fq", 14), 4: ("BLS12-381 Fq", 14)}  # name, 29-bit limbs


def _compilers():
    out = ["g++"]
    if os.path.exists(ROCM_CLANG):
        out.append(ROCM_CLANG)
    return out


@pytest.fixture(scope="module", params=_compilers(), ids=lambda c: os.path.basename(c))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fe_words_neg") / "fe_words_neg_host")
    subprocess.run([request.param, "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC], check=True)
    return exe


def _inputs(p, L, seed):
    top = p.bit_length()
    vals = [1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    # long borrow chains: words of all ones below zero words, zero words below words of all ones, and runs of either in the middle
    for a in range(L):
        for b in range(a + 1, L + 1):
            ones = ((1 << (32 * (b - a))) - 1) << (32 * a)
            vals += [ones, ones + 1, ones - 1, (1 << (top - 1)) | ones, ((1 << (top - 1)) - 1) & ~ones]
    # one word set, the others zero
    rng = np.random.default_rng(seed)
    for i in range(L):
        words = [1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF] + [int(x) for x in rng.integers(1, 1 << 32, 8)]
        vals += [w << (32 * i) for w in words]
    vals += [int.from_bytes(rng.bytes(4 * L + 8), "little") % p for _ in range(10000)]
    return [v for v in vals if 0 < v < p]


@pytest.mark.parametrize("fid", sorted(FIELDS))
def test_words_neg_is_p_minus_y_and_unpacks_tight(program, fid):
    L = po.FIELD_LC[fid]
    N = FIELDS[fid][1]
    p = pyref.limbs_to_int(po.field_info(fid)["p"])
    vals = _inputs(p, L, 0xF00D + fid)
    assert len(vals) > 10000
    text = "".join(" ".join("%08x" % ((v >> (32 * i)) & 0xFFFFFFFF) for i in range(L)) + "\n" for v in vals)
    run = subprocess.run([program, str(fid)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-500:])
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(vals)
    for v, line in zip(vals, lines):
        nums = [int(x, 16) for x in line.split()]
        words, limbs = nums[:L], nums[L:]
        assert sum(w << (32 * i) for i, w in enumerate(words)) == p - v, hex(v)
        assert len(limbs) == N and all(x < (1 << 29) for x in limbs), hex(v)
        assert sum(x << (29 * i) for i, x in enumerate(limbs)) == p - v, hex(v)
