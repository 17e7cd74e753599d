"""What tests/test_points_mul.py and tests/test_kzg_open_all.py share: multiples of the generator in Python integers through tests/pyref.py
(ec_add, encode_affine), the wire forms, and guarded device buffers.  Every expected point is k G for a known k, so one table of the
doublings of G per curve serves them all (a multiple then costs its one bits in additions, no doublings)."""
import ctypes as C
import functools

import numpy as np

import pyref
from panda_amd import gpu_ffi as ffi

GUARD, GUARD_BYTES = 0xA5, 4096
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


def scalar_wire(curve, v):
    """integer -> the 32-byte Montgomery form of the curve's Fr"""
    c = pyref.CURVES[curve]
    return pyref.int_to_limbs(v % c.r * c.Rr % c.r, 8)


def scalars_wire(curve, vs):
    return np.stack([scalar_wire(curve, v) for v in vs])


def random_scalars(curve, seed, n):
    r = pyref.CURVES[curve].r
    raw = np.random.default_rng(seed).bytes(40 * n)
    return [int.from_bytes(raw[40 * j:40 * j + 40], "little") % r for j in range(n)]


def compare(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, "first differing outputs", bad[:8].tolist())


def host_ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Dev:
    """device buffers with a guard run of a fixed byte behind the data, which no call may touch"""

    def __init__(self, gm, curve=0):
        self.lib, self.curve, self.stream, self.bufs = ffi.load(), curve, gm.exec_stream.raw, []

    def buffer(self, x=None, nbytes=None):
        from gpu_util import DeviceBuffer
        if x is not None:
            x = np.ascontiguousarray(x, np.uint32)
            nbytes = x.nbytes
        d = DeviceBuffer(nbytes + GUARD_BYTES)
        d.data_bytes, d.host = nbytes, x
        self.bufs.append(d)
        ffi.check(self.lib.panda_memset(d.ptr, GUARD, nbytes + GUARD_BYTES), "memset")
        if x is not None and nbytes:
            ffi.check(self.lib.panda_memcpy(d.ptr, C.c_void_p(x.ctypes.data), nbytes), "memcpy")
        return d

    def get(self, d):
        return d.to_host(np.uint32, nbytes=d.data_bytes)

    def guard_intact(self, d):
        return bool((d.to_host(np.uint8, nbytes=GUARD_BYTES, offset=d.data_bytes) == GUARD).all())

    def intact(self, d):
        """the guard behind the data, and the data itself if the buffer was an input"""
        return self.guard_intact(d) and (d.host is None or np.array_equal(self.get(d), d.host.reshape(-1)))

    def untouched(self, d):
        """an output buffer that nothing has written: the fill byte throughout"""
        return bool((d.to_host(np.uint8) == GUARD).all())

    def close(self):
        for d in self.bufs:
            d.free()
        self.bufs = []
