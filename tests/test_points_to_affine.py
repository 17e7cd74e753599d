"""panda_points_to_affine / panda_points_to_affine_plan: n result triples X || Y || Z (Jacobian or homogeneous, identity <=> Z == 0) to n
affine wire points with one field inversion per chunk of points.

The triples are built in Python (tests/pyref.py integers) from known affine points with random Z != 1, the expected output is those
affine points on the wire with the identity as all-zero bytes; outputs are canonical, so every comparison is byte for byte.  The chunk
comes from the plan call, and the sizes sit on its edges.  Every device buffer carries a guard run behind the data; the input must come
back unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import field_ref as fr
import oracle as po
import pyref
from gpu_util import gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm
from test_ec_ntt import CURVES, Dev, _enc, _mul_g, _pb

gpu = pytest.mark.gpu
CAP = 1 << 28


def _plan(lib, n):
    chunk, launches = C.c_uint(0xDEAD), C.c_uint(0xDEAD)
    rc = lib.panda_points_to_affine_plan(n, C.byref(chunk), C.byref(launches))
    return rc, chunk.value, launches.value


@functools.lru_cache(maxsize=None)
def _chunk():
    rc, chunk, launches = _plan(ffi.load(), 1)
    assert rc == 0 and chunk >= 2 and launches == 1
    return chunk


# ------------------------------------------------------------------------------------------------- without a GPU
def test_plan():
    lib = ffi.load()
    seen = set()
    for n in (1, 2, 15, 16, 17, 1000, 1 << 20, CAP - 1, CAP):
        rc, chunk, launches = _plan(lib, n)
        assert rc == 0 and launches == 1, n
        seen.add(chunk)
    assert len(seen) == 1 and 2 <= _chunk() <= 1024, "the chunk depends on nothing"
    assert lib.panda_points_to_affine_plan(5, None, None) == 0
    for n in (0, CAP + 1, 1 << 40, (1 << 64) - 1):
        assert _plan(lib, n) == (1, 0xDEAD, 0xDEAD), n


def _refusals(lib, curve, IN, OUT, n, stream, untouched):
    pb = _pb(curve)
    count = [0]

    def call(curve=curve, d_in=IN, in_type=ffi.JACOBIAN, d_out=OUT, n=n):
        count[0] += 1
        rc = lib.panda_points_to_affine(curve, None if d_in is None else C.c_void_p(d_in), in_type, None if d_out is None else C.c_void_p(d_out), n, stream)
        assert untouched(), "a refused call wrote to a buffer"
        return rc

    for bad_curve in (3, 4, 6, 5, 7, 0xFFFFFFFF):
        assert call(curve=bad_curve) == 1
    assert call(in_type=2) == 1 and call(in_type=-1) == 1 and call(n=0) == 1 and call(n=CAP + 1) == 1 and call(n=1 << 40) == 1
    assert call(d_in=None) == 1 and call(d_out=None) == 1
    in_bytes, out_bytes = n * pb * 3 // 2, n * pb
    for in_type in (ffi.JACOBIAN, ffi.PROJECTIVE):
        for off in (0, 16, in_bytes - 16, -16, -(out_bytes - 16), pb):
            assert call(d_out=IN + off, in_type=in_type) == 1, ("overlap", off)
    return count[0]


def test_bad_arguments_are_refused_before_any_device_call():
    lib = ffi.load()
    mem = np.full(4 << 20, 0x5A, np.uint8)
    base = (mem.ctypes.data + 4095) & ~4095
    for curve in CURVES:
        assert _refusals(lib, curve, base + (1 << 20), base + (2 << 20), 16, ffi.PandaStream(), lambda: bool((mem == 0x5A).all())) > 20


# ------------------------------------------------------------------------------------------------- on the device
@functools.lru_cache(maxsize=None)
def _points(curve, n):
    """(a + j d) G for j < n by repeated additions"""
    c = pyref.CURVES[curve]
    a, d = fr.random_residues(curve, 0xAF00 + curve, 2)
    step, P, pts = _mul_g(curve, d), _mul_g(curve, a), []
    for _ in range(n):
        pts.append(P)
        P = pyref.ec_add(c, P, step)
    return pts


def _triples(curve, pts, homogeneous, seed):
    """wire triples with random Z != 0, 1; None becomes Z == 0 beside nonzero X and Y"""
    c = pyref.CURVES[curve]
    L = c.lc_q
    raw = np.random.default_rng(seed).bytes(48 * len(pts))
    out = np.zeros((len(pts), 3 * L), np.uint32)
    for i, P in enumerate(pts):
        z = 2 + int.from_bytes(raw[48 * i:48 * i + 48], "little") % (c.p - 2)
        if P is None:
            X, Y, z = z, z + 1, 0
        elif homogeneous:
            X, Y = P[0] * z % c.p, P[1] * z % c.p
        else:
            X, Y = P[0] * z * z % c.p, P[1] * z * z * z % c.p
        for k, v in enumerate((X, Y, z)):
            out[i, k * L:(k + 1) * L] = pyref.int_to_limbs(v * c.Rq % c.p, L)
    return out


def _convert(gm, curve, pts, homogeneous, seed, what):
    h = Dev(gm, curve)
    try:
        n = len(pts)
        src, dst = h.buffer(_triples(curve, pts, homogeneous, seed)), h.buffer(nbytes=n * _pb(curve))
        rc = h.lib.panda_points_to_affine(curve, src.ptr, ffi.PROJECTIVE if homogeneous else ffi.JACOBIAN, dst.ptr, n, h.stream)
        assert rc == 0, what
        assert h.intact(src) and h.intact(dst), (what, "guards or input")
        got = h.get(dst).reshape(n, -1)
        want = np.stack([_enc(curve, P) for P in pts])
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (what, "first differing points", bad[:8].tolist())
    finally:
        h.close()


@gpu
@pytest.mark.parametrize("homogeneous", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_sizes_on_the_chunk_edges(gm, curve, homogeneous):
    """n in {1, chunk - 1, chunk, chunk + 1, 3 x 256 x chunk + 5}, without identities and with Z == 0 at the first, the last and runs of
    `chunk` consecutive positions (one run a whole chunk, one across a chunk edge)"""
    chunk = _chunk()
    big = 3 * 256 * chunk + 5
    all_pts = _points(curve, big)
    for n in (1, chunk - 1, chunk, chunk + 1, big):
        pts = list(all_pts[:n])
        _convert(gm, curve, pts, homogeneous, 0xAF10 + n, (curve, homogeneous, n, "no identity"))
        holes = {0, n - 1}
        if n > 3 * chunk:
            holes |= set(range(chunk, 2 * chunk)) | set(range(5 * chunk + chunk // 2, 6 * chunk + chunk // 2)) | set(range(n - 5 - chunk, n - 5))
        elif n >= chunk:
            holes = set(range(chunk))  # the whole first chunk; a point may follow it
        for j in holes:
            pts[j] = None
        _convert(gm, curve, pts, homogeneous, 0xAF20 + n, (curve, homogeneous, n, "identities"))


@gpu
@pytest.mark.parametrize("curve", CURVES)
def test_through_msm_results(gm, curve):
    """the results of one panda_msm_execute_batch (8 members at 2^10) through the conversion equal what the decoders give"""
    c = pyref.CURVES[curve]
    n, batch = 1 << 10, 8
    bases = po.gen_bases(curve, 0xAF40 + curve, n)
    vectors = [po.gen_scalars(po.FR_OF[curve], 0xAF50 + 16 * curve + k, n) for k in range(batch)]
    vectors[3] = np.zeros_like(vectors[3])  # a member whose result is the identity
    idx = gm.add_cached_bases(bases)
    for projective in ((False, True) if curve == 0 else (False,)):
        gm.set_config(ffi.PROJECTIVE if projective else ffi.JACOBIAN)
        try:
            results = pgm.panda_msm_gpu_batch_with_cached_bases(gm, vectors, idx, curve)
        finally:
            gm.set_config(ffi.JACOBIAN)
        decode = pyref.decode_homogeneous if projective else pyref.decode_jacobian
        want = np.stack([_enc(curve, decode(c, r.view(np.uint32))) for r in results])
        assert not want[3].any() and want[0].any()
        got = pgm.panda_points_gpu_to_affine(gm, np.concatenate(results), curve, projective=projective).view(np.uint32).reshape(batch, -1)
        assert np.array_equal(got, want), (curve, projective)


@gpu
def test_refusals_leave_the_guarded_output_untouched(gm):
    from gpu_util import DeviceBuffer
    lib = ffi.load()
    for curve in CURVES:
        h = Dev(gm, curve)
        try:
            pb, n = _pb(curve), 16
            room = h.buffer(np.arange(3 * n * pb * 3 // 2 // 4, dtype=np.uint32))
            out = h.buffer(nbytes=3 * n * pb)
            IN, OUT = room.ptr.value + n * pb * 3 // 2, out.ptr.value + n * pb
            untouched = lambda: h.intact(room) and h.untouched(out)
            assert _refusals(lib, curve, IN, OUT, n, h.stream, untouched) > 20
            short = DeviceBuffer(n * pb)
            try:
                for d_in, d_out, count in ((short.ptr.value, OUT, n), (IN, short.ptr.value, n + 1)):
                    assert lib.panda_points_to_affine(curve, C.c_void_p(d_in), ffi.JACOBIAN, C.c_void_p(d_out), count, h.stream) == 1 and untouched()
            finally:
                short.free()
        finally:
            h.close()
