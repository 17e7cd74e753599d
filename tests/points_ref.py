"""What tests/test_points_mul.py and tests/test_kzg_open_all.py share: multiples of the generator in Python integers through tests/pyref.py
(ec_add, encode_affine), the points' wire form, and the guarded device buffers of a curve's calls; scalars come from tests/field_ref.py
(a curve's id is its scalar field's).  Every expected point is k G for a known k, so one table of the doublings of G per curve serves
them all (a multiple then costs its one bits in additions, no doublings)."""
import ctypes as C
import functools

import numpy as np

import pyref
from gpu_util import GuardedBuffers
from panda_amd import gpu_ffi as ffi

CURVES = (0, 1, 2)


def point_bytes(curve):
    return 64 if curve == 0 else 96


@functools.lru_cache(maxsize=None)
def _doublings(curve):
    c = pyref.CURVES[curve]
    t, P = [], c.g
    for _ in range(256):
        t.append(P)
        P = pyref.ec_add(c, P, P)
    return t


@functools.lru_cache(maxsize=None)
def mul_g(curve, k):
    """(k mod r) G as an affine point, None for the identity"""
    c = pyref.CURVES[curve]
    k %= c.r
    R = None
    for b, D in enumerate(_doublings(curve)):
        if (k >> b) & 1:
            R = pyref.ec_add(c, R, D)
    return R


def enc(curve, P):
    """affine point -> wire words; the identity is all-zero bytes"""
    c = pyref.CURVES[curve]
    return np.zeros(2 * c.lc_q, np.uint32) if P is None else pyref.encode_affine(c, P)


def enc_all(curve, pts):
    return np.stack([enc(curve, P) for P in pts])


def enc_multiples(curve, ks):
    return enc_all(curve, [mul_g(curve, k) for k in ks])


def compare(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, "first differing outputs", bad[:8].tolist())


def host_ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Dev(GuardedBuffers):
    """guarded device buffers for the calls of one curve"""

    def __init__(self, gm, curve=0):
        super().__init__()
        self.lib, self.curve, self.stream = ffi.load(), curve, gm.exec_stream.raw
