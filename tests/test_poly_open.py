"""panda_poly_evaluate / panda_poly_divide_linear / panda_poly_plan: the values of `batch` polynomials of n coefficients (ANY n >= 1) at
a few points, and their quotients by X - z, on coefficients resident on the device -- the opening step of a KZG prover.

With S_j = c_j + z S_(j+1), S_n = 0: f(z) = S_0, q_j = S_(j+1) (q_(n-1) = 0 is written too).  The Montgomery wire form is linear, so the
same recurrence holds on the wire residues with the plain integer z.  Outputs are canonical and every comparison is byte for byte.  The
expected values are Python integers (plain Horner; moduli from po.field_info) up to a few tiles; above that the CPU oracle's vector ops
check the COMPLETE characterisation of quotient and remainder -- q_(n-1) = 0, q_(j-1) - z q_j = c_j for 1 <= j < n, r - z q_0 = c_0 --
which (q, r) satisfy if and only if they are the quotient and the remainder.  Every boundary size comes from panda_poly_plan.  Each
device buffer carries a guard run of a fixed byte pattern behind the batch, which no call may touch; the coefficients must come back
unchanged unless the division is in place."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

import field_ref as fr
import oracle as po
import pyref
from gpu_util import GUARD, ROOT, GuardedBuffers, assert_exported, free_bytes, gm  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

sys.path.insert(0, os.path.join(ROOT, "tools"))
import model_poly_scan as mps  # noqa: E402

MAX_POINTS = 8  # PANDA_POLY_MAX_POINTS
MAX_ELEMS = 1 << 28


def _plan(lib, n, batch):
    tile, chunk, le, ld = C.c_uint(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
    rc = lib.panda_poly_plan(n, batch, C.byref(tile), C.byref(chunk), C.byref(le), C.byref(ld))
    return rc, tile.value, chunk.value, le.value, ld.value


@functools.lru_cache(maxsize=None)
def _shape():
    """(tile, carry_chunk) of the library"""
    rc, tile, chunk, _, _ = _plan(ffi.load(), 1, 1)
    assert rc == 0
    return tile, chunk


def _second_level_sizes():
    tile, chunk = _shape()
    return tile * chunk + 1, 2 * tile * chunk + tile + 5


def _horner(field, coeffs, z_plain):
    """(quotient words (n, 8), remainder words (8,)) of one polynomial by plain Horner over Python integers"""
    r = fr.modulus(field)
    c = fr.ints(coeffs)
    q, s = [0] * len(c), 0
    for j in range(len(c) - 1, -1, -1):
        q[j] = s
        s = (c[j] + z_plain * s) % r
    return fr.words(q), fr.words([s])[0]


def _is_quotient(field, coeffs, z_wire, q, rem):
    """the complete characterisation by three vector operations of the CPU oracle (n >= 2)"""
    fid = po.FR_OF[field]
    n = len(coeffs)
    if np.any(q[n - 1]):
        return False
    zq = po.f_vec(fid, po.OP_MUL, q, np.broadcast_to(z_wire, (n, 8)))  # z q_j
    lhs = po.f_vec(fid, po.OP_SUB, np.ascontiguousarray(q[:n - 1]), np.ascontiguousarray(zq[1:]))  # q_(j-1) - z q_j
    if not np.array_equal(lhs, coeffs[1:]):
        return False
    c0 = po.f_vec(fid, po.OP_SUB, rem.reshape(1, 8), np.ascontiguousarray(zq[:1]))
    return np.array_equal(c0[0], coeffs[0])


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, lib = assert_exported(("panda_poly_evaluate", "panda_poly_divide_linear", "panda_poly_plan"))
    assert re.search(r"#define\s+PANDA_POLY_MAX_POINTS\s+%d\b" % MAX_POINTS, header)
    assert ffi.POLY_MAX_POINTS == MAX_POINTS
    assert lib.panda_poly_evaluate.argtypes[2] is C.c_uint64 and lib.panda_poly_divide_linear.argtypes[3] is C.c_uint64
    assert lib.panda_poly_plan.argtypes[0] is C.c_uint64


def test_bad_arguments_are_refused_before_any_device_call():
    """every shape, pointer, point and overlap error returns 1 with the host outputs untouched -- also on a machine with no device"""
    lib = ffi.load()
    mem = np.zeros(2 << 20, np.uint8)  # two disjoint 1 MiB host ranges stand in for the device buffers: nothing may dereference them
    base = mem.ctypes.data
    at = lambda off: C.c_void_p(base + off)
    coeffs, quot = at(0), at(1 << 20)
    stream = ffi.PandaStream()
    out = np.full((4 * MAX_POINTS, 8), 0x5A5A5A5A, np.uint32)
    outp = C.c_void_p(out.ctypes.data)
    for field in range(3):
        r = fr.modulus(field)
        good = np.stack([fr.wire_one(field, 3 + k) for k in range(MAX_POINTS)])
        at_modulus = np.array(pyref.int_to_limbs(r, 8), np.uint32)
        all_ones = np.full(8, 0xFFFFFFFF, np.uint32)
        gp = C.c_void_p(good.ctypes.data)

        def ev(f=field, c=coeffs, n=16, batch=2, pts=gp, k=2, vals=outp):
            return lib.panda_poly_evaluate(f, c, n, batch, pts, k, vals, stream)

        def dv(f=field, c=coeffs, q=quot, n=16, batch=2, pt=gp, rem=outp):
            return lib.panda_poly_divide_linear(f, c, q, n, batch, pt, rem, stream)

        assert ev(f=3) == 1 and dv(f=3) == 1
        assert ev(n=0) == 1 and dv(n=0) == 1
        assert ev(batch=0) == 1 and dv(batch=0) == 1
        assert ev(n=MAX_ELEMS + 1, batch=1) == 1 and dv(n=MAX_ELEMS + 1, batch=1) == 1
        assert ev(n=(MAX_ELEMS >> 1) + 1, batch=2) == 1 and dv(n=(MAX_ELEMS >> 1) + 1, batch=2) == 1
        assert ev(n=1, batch=MAX_ELEMS + 1) == 1 and dv(n=1, batch=MAX_ELEMS + 1) == 1
        assert ev(n=1 << 63, batch=2) == 1 and dv(n=(1 << 64) - 1, batch=1) == 1
        assert ev(k=0) == 1 and ev(k=MAX_POINTS + 1) == 1
        assert ev(c=None) == 1 and ev(pts=None) == 1 and ev(vals=None) == 1
        assert dv(c=None) == 1 and dv(q=None) == 1 and dv(pt=None) == 1
        for bad in (at_modulus, all_ones):
            assert dv(pt=C.c_void_p(bad.ctypes.data)) == 1
            for pos in (0, 1, MAX_POINTS - 1):  # a bad point anywhere in the list
                pts = good.copy()
                pts[pos] = bad
                assert ev(pts=C.c_void_p(pts.ctypes.data), k=pos + 1) == 1
        # 2 polynomials of 16 coefficients are 1024 bytes: every way the two ranges can meet without being equal
        assert dv(q=at(1023)) == 1           # the quotient's first byte is the coefficients' last
        assert dv(c=at((1 << 20) + 1023)) == 1
        assert dv(q=at(32)) == 1             # one element up: the shifted alias a caller might try
        assert dv(c=at(512), q=at(0)) == 1
    assert (out == 0x5A5A5A5A).all(), "a refused call wrote to values / remainders"
    # the exact alias is a legal shape: panda_poly_plan accepts what the refused calls above were refused for only by their pointers
    assert lib.panda_poly_plan(16, 2, None, None, None, None) == 0
    for n, batch in ((0, 1), (1, 0), (MAX_ELEMS + 1, 1), ((MAX_ELEMS >> 1) + 1, 2), (1, MAX_ELEMS + 1), (1 << 63, 2), ((1 << 64) - 1, 1), (1 << 32, 1 << 31)):
        assert lib.panda_poly_plan(n, batch, None, None, None, None) == 1, (n, batch)


def test_poly_plan():
    lib = ffi.load()
    for n in (1, 2, 3, 63, 64, 65, 1000, 2047, 2048, 2049, (1 << 16) + 3, (1 << 20) + 2, 1 << 24, (1 << 27) + 1, 1 << 28):
        seen = set()
        for batch in (1, 2, 3, 16, 256, 1 << 20, 1 << 28):
            if n * batch > MAX_ELEMS:
                assert lib.panda_poly_plan(n, batch, None, None, None, None) == 1
                continue
            rc, tile, chunk, le, ld = _plan(lib, n, batch)
            assert rc == 0 and tile >= 1 and chunk >= 1 and le >= 1 and ld >= le, (n, batch)
            seen.add((tile, chunk, le, ld))
            for i in range(4):  # every out pointer may be NULL, singly
                outs = [C.c_uint(0xDEAD) for _ in range(4)]
                args = [C.byref(o) if j != i else None for j, o in enumerate(outs)]
                assert lib.panda_poly_plan(n, batch, *args) == 0
                assert [o.value for j, o in enumerate(outs) if j != i] == [v for j, v in enumerate((tile, chunk, le, ld)) if j != i]
        assert len(seen) == 1, "none of the four depends on the batch"


def _boundary_sizes():
    """around the thread run E and the wave's WAVE x E (the model's constants mirror csrc/poly.hip), the tile, several tiles and a tail"""
    tile, chunk = _shape()
    e = tile // (mps.WAVE * mps.WAVES)
    sizes = {1, 2, 3, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile - 7, e - 1, e + 1, mps.WAVE * e - 1, mps.WAVE * e + 1}
    return sorted(s for s in sizes if s >= 1)


def test_scan_model_agrees_with_plain_horner():
    """tools/model_poly_scan.py -- the three launches' index maps over exact integers -- with the library's tile and carry chunk, at
    every size the device tests run, out of place and in place; and a scaled-down shape at every n through its third level"""
    tile, chunk = _shape()
    sh = mps.Shape.from_plan(tile, chunk)
    assert (sh.tile, sh.chunk) == (tile, chunk)
    for n in _boundary_sizes() + list(_second_level_sizes()):
        assert mps.check(sh, n)
    for z in (0, 1, mps.P - 1):
        assert mps.check(sh, tile + 1, z=z)
    small = mps.Shape(e=3, wave=4, waves=2, ce=2)
    for n in range(1, 2 * small.tile * small.chunk + small.tile + 6, 7):
        assert mps.check(small, n)


# ------------------------------------------------------------------------------------------------- on the device
@functools.lru_cache(maxsize=None)
def _coeffs(field, n, batch, seed):
    x = po.gen_scalars(po.FR_OF[field], seed, batch * n).reshape(batch, n, 8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _point(field, seed):
    """(wire words, plain integer) of a random point"""
    w = po.gen_scalars(po.FR_OF[field], 0x9000 + seed, 1)[0]
    return w, fr.plain(field, w)[0]


class Harness(GuardedBuffers):
    """the coefficient and the quotient buffer, each with a guard run behind the batch"""

    def __init__(self, gm, field, n, batch):
        super().__init__()
        self.lib, self.gm, self.field, self.n, self.batch = ffi.load(), gm, field, n, batch
        self.bytes = batch * n * 32
        self.c, self.q = self.buffer(nbytes=self.bytes), self.buffer(nbytes=self.bytes)
        self.stream = gm.exec_stream.raw

    def load(self, coeffs):
        """both buffers afresh, the coefficients (batch x n elements) in the first"""
        assert np.asarray(coeffs).nbytes == self.bytes
        self.fill(self.c, coeffs)
        self.fill(self.q)

    def divide(self, coeffs, z_wire, in_place=False, remainders=True):
        """one panda_poly_divide_linear -> (quotients (batch, n, 8), remainders (batch, 8) or None); checks guards and coefficients"""
        self.load(coeffs)
        z = np.ascontiguousarray(z_wire, np.uint32)
        rem = np.full((self.batch, 8), 0x77777777, np.uint32) if remainders else None
        dst = self.c if in_place else self.q
        ffi.check(self.lib.panda_poly_divide_linear(self.field, self.c.ptr, dst.ptr, self.n, self.batch, C.c_void_p(z.ctypes.data),
                                                    C.c_void_p(rem.ctypes.data) if remainders else None, self.stream), "divide")
        assert self.guard_intact(self.c) and self.guard_intact(self.q), "bytes behind the batch were written"
        if in_place:
            assert self.untouched(self.q), "the other buffer was written by a division in place"
        else:
            assert self.intact(self.c), "d_coeffs was written"
        return self.get(dst).reshape(self.batch, self.n, 8), rem

    def evaluate(self, coeffs, points_wire):
        self.load(coeffs)
        pts = np.ascontiguousarray(points_wire, np.uint32).reshape(-1, 8)
        vals = np.full((self.batch, len(pts), 8), 0x77777777, np.uint32)
        ffi.check(self.lib.panda_poly_evaluate(self.field, self.c.ptr, self.n, self.batch, C.c_void_p(pts.ctypes.data), len(pts),
                                               C.c_void_p(vals.ctypes.data), self.stream), "evaluate")
        assert self.intact(self.c), "d_coeffs or the bytes behind the batch were written"
        assert self.untouched(self.q), "an evaluation wrote to an unrelated buffer"
        return vals


def _check_against_horner(h, coeffs, z_wire, z_plain, **kw):
    q, rem = h.divide(coeffs, z_wire, **kw)
    for p in range(h.batch):
        want_q, want_r = _horner(h.field, coeffs[p], z_plain)
        assert np.array_equal(q[p], want_q), (h.field, h.n, p)
        assert rem is None or np.array_equal(rem[p], want_r), (h.field, h.n, p)
    return q, rem


@pytest.mark.gpu
def test_division_bn254_vs_horner(gm):
    """batch 3, random z: n around the thread run E, the wave's 64 E, the tile, several tiles with a ragged tail (the sizes come from the
    plan, so they are walked inside one test and not parametrised at collection, which must not need the library)"""
    for n in _boundary_sizes():
        z_wire, z_plain = _point(0, n)
        h = Harness(gm, 0, n, 3)
        try:
            _check_against_horner(h, _coeffs(0, n, 3, 0xA000 + n), z_wire, z_plain)
        finally:
            h.close()


@pytest.mark.gpu
def test_division_without_remainders(gm):
    tile, _ = _shape()
    n = 2 * tile + 1
    z_wire, z_plain = _point(0, 1)
    h = Harness(gm, 0, n, 3)
    try:
        _check_against_horner(h, _coeffs(0, n, 3, 0xA100), z_wire, z_plain, remainders=False)
    finally:
        h.close()


def _check_by_identity(h, coeffs, z_wire, **kw):
    q, rem = h.divide(coeffs, z_wire, **kw)
    for p in range(h.batch):
        assert _is_quotient(h.field, coeffs[p], z_wire, q[p], rem[p]), (h.field, h.n, p)
    return q, rem


def _second_level_case(gm, field, which, batch, in_place=False):
    n = _second_level_sizes()[which]
    if n > 1 << 23:
        pytest.skip("tile x carry_chunk exceeds 2^23 elements for this plan")
    z_wire, _ = _point(field, 77 + which)
    h = Harness(gm, field, n, batch)
    try:
        return _check_by_identity(h, _coeffs(field, n, batch, 0xB000 + which), z_wire, in_place=in_place)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("which", [0, 1])
def test_second_level(gm, which, batch):
    """more tile totals than one step of the carry kernel takes: one chunk and one total, and two chunks and a ragged third"""
    _second_level_case(gm, 0, which, batch)


@pytest.mark.gpu
@pytest.mark.gpu_soak
def test_division_2_24(gm):
    n = 1 << 24
    z_wire, _ = _point(0, 24)
    h = Harness(gm, 0, n, 1)
    try:
        _check_by_identity(h, _coeffs(0, n, 1, 0xB024), z_wire)
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["z0", "z1", "zm1", "allm1", "zero"])
def test_edge_values(gm, case):
    tile, _ = _shape()
    n, batch, r = tile + 1, 2, fr.modulus(0)
    coeffs = _coeffs(0, n, batch, 0xC000)
    z_plain = {"z0": 0, "z1": 1, "zm1": r - 1, "allm1": r - 1, "zero": _point(0, 5)[1]}[case]
    if case == "allm1":
        coeffs = np.broadcast_to(fr.wire_one(0, r - 1), (batch, n, 8))
    if case == "zero":
        coeffs = np.zeros((batch, n, 8), np.uint32)
    h = Harness(gm, 0, n, batch)
    try:
        q, rem = _check_against_horner(h, coeffs, fr.wire_one(0, z_plain), z_plain)
        if case == "z0":  # q_j = c_(j+1), r = c_0
            assert np.array_equal(q[:, :n - 1], coeffs[:, 1:]) and np.array_equal(rem, coeffs[:, 0])
        if case == "zero":
            assert not q.any() and not rem.any()
    finally:
        h.close()


@pytest.mark.gpu
def test_in_place_equals_out_of_place(gm):
    tile, _ = _shape()
    n, batch = 2 * tile + 1, 3
    z_wire, z_plain = _point(0, 8)
    coeffs = _coeffs(0, n, batch, 0xD000)
    h = Harness(gm, 0, n, batch)
    try:
        q, rem = _check_against_horner(h, coeffs, z_wire, z_plain)
        q2, rem2 = h.divide(coeffs, z_wire, in_place=True)
        assert np.array_equal(q, q2) and np.array_equal(rem, rem2)
    finally:
        h.close()


@pytest.mark.gpu
def test_in_place_at_the_second_level(gm):
    q, rem = _second_level_case(gm, 0, 0, 1)
    q2, rem2 = _second_level_case(gm, 0, 0, 1, in_place=True)
    assert np.array_equal(q, q2) and np.array_equal(rem, rem2)


@pytest.mark.gpu
def test_partial_overlap_of_live_buffers_is_refused(gm):
    tile, _ = _shape()
    n, batch = tile + 1, 2
    z_wire, _ = _point(0, 9)
    h = Harness(gm, 0, n, batch)
    try:
        h.load(_coeffs(0, n, batch, 0xD100))
        rem = np.full((batch, 8), 0x77777777, np.uint32)
        zp, rp = C.c_void_p(z_wire.ctypes.data), C.c_void_p(rem.ctypes.data)
        for c_off, q_off in ((0, 32), (32, 0), (0, h.bytes - 32)):
            rc = h.lib.panda_poly_divide_linear(0, C.c_void_p(h.c.ptr.value + c_off), C.c_void_p(h.c.ptr.value + q_off), n, batch, zp, rp, h.stream)
            assert rc == 1
        assert (rem == 0x77777777).all()
        assert h.intact(h.c) and h.untouched(h.q)
    finally:
        h.close()


@functools.lru_cache(maxsize=None)
def _eval_points(field):
    pts = [_point(field, 100 + k) for k in range(MAX_POINTS)]
    return np.stack([w for w, _ in pts]), [v for _, v in pts]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n_points", [1, 2, 3, 8])
@pytest.mark.parametrize("which", [0, 1])
def test_evaluation_vs_horner_and_division(gm, which, n_points, batch):
    tile, _ = _shape()
    n = (tile + 1, 5 * tile - 7)[which]
    wires, plains = _eval_points(0)
    coeffs = _coeffs(0, n, batch, 0xE000 + which)
    h = Harness(gm, 0, n, batch)
    try:
        vals = h.evaluate(coeffs, wires[:n_points])
        for p in range(batch):
            for k in range(n_points):
                assert np.array_equal(vals[p, k], _horner(0, coeffs[p], plains[k])[1]), (n, p, k)
        for k in range(n_points):
            _, rem = h.divide(coeffs, wires[k])
            assert np.array_equal(rem, vals[:, k]), "the remainders of the division at the same point"
    finally:
        h.close()


@pytest.mark.gpu
def test_evaluation_at_roots_of_unity_equals_the_transform(gm):
    """f(w^k) is element k of the forward transform: ties the feature to panda_ntt_execute_bn254_v1, which the oracle pins"""
    from gpu_util import DeviceBuffer
    log_n, fid = 12, po.F_BN254_FR
    n, r = 1 << log_n, fr.modulus(0)
    omega = po.root_of_unity(fid, log_n)
    w = fr.plain(0, omega)[0]
    ks = (1, 777, n - 1)
    coeffs = _coeffs(0, n, 1, 0xE100)
    h = Harness(gm, 0, n, 1)
    sa, sb = DeviceBuffer(n * 32), DeviceBuffer(n * 32)
    try:
        vals = h.evaluate(coeffs, np.stack([fr.wire_one(0, pow(w, k, r)) for k in ks]))
        flag = C.c_uint(9)
        ffi.check(h.lib.panda_memcpy(sa.ptr, C.c_void_p(np.ascontiguousarray(coeffs[0]).ctypes.data), n * 32), "memcpy")
        cfg = ffi.NttconfigurationV1(gm.mem_pool, gm.exec_stream.raw, sa.ptr, sb.ptr, C.c_void_p(omega.ctypes.data), log_n, C.pointer(flag))
        ffi.check(h.lib.panda_ntt_execute_bn254_v1(cfg), "ntt")
        y = (sb if flag.value else sa).to_host(np.uint32).reshape(n, 8)
        for i, k in enumerate(ks):
            assert np.array_equal(vals[0, i], y[k]), k
    finally:
        sa.free()
        sb.free()
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_other_fields_at_one_tile_and_one(gm, field):
    tile, _ = _shape()
    n, batch = tile + 1, 2
    wires, plains = _eval_points(field)
    coeffs = _coeffs(field, n, batch, 0xF000 + field)
    h = Harness(gm, field, n, batch)
    try:
        _, rem = _check_against_horner(h, coeffs, wires[0], plains[0])
        vals = h.evaluate(coeffs, wires[:3])
        assert np.array_equal(vals[:, 0], rem)
        for p in range(batch):
            for k in range(3):
                assert np.array_equal(vals[p, k], _horner(field, coeffs[p], plains[k])[1])
    finally:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_other_fields_at_the_second_level(gm, field):
    n = _second_level_sizes()[0]
    if n > 1 << 23:
        pytest.skip("tile x carry_chunk exceeds 2^23 elements for this plan")
    batch = 2
    wires, _ = _eval_points(field)
    coeffs = _coeffs(field, n, batch, 0xF100 + field)
    h = Harness(gm, field, n, batch)
    try:
        _, rem = _check_by_identity(h, coeffs, wires[1])
        vals = h.evaluate(coeffs, wires[1:2])
        assert np.array_equal(vals[:, 0], rem)
    finally:
        h.close()


@pytest.mark.gpu
def test_short_device_buffers_are_refused(gm):
    from gpu_util import DeviceBuffer
    tile, _ = _shape()
    n, batch = tile + 1, 3
    z_wire, z_plain = _point(0, 11)
    h = Harness(gm, 0, n, batch)
    short = DeviceBuffer(h.bytes - 32)  # one element short
    try:
        coeffs = _coeffs(0, n, batch, 0xF200)
        h.load(coeffs)
        ffi.check(h.lib.panda_memset(short.ptr, GUARD, h.bytes - 32), "memset")
        out = np.full((batch, 8), 0x77777777, np.uint32)
        zp, op = C.c_void_p(z_wire.ctypes.data), C.c_void_p(out.ctypes.data)
        assert h.lib.panda_poly_divide_linear(0, short.ptr, h.q.ptr, n, batch, zp, op, h.stream) == 1
        assert h.lib.panda_poly_divide_linear(0, h.c.ptr, short.ptr, n, batch, zp, op, h.stream) == 1
        assert h.lib.panda_poly_divide_linear(0, short.ptr, short.ptr, n, batch, zp, op, h.stream) == 1
        assert h.lib.panda_poly_evaluate(0, short.ptr, n, batch, zp, 1, op, h.stream) == 1
        assert (out == 0x77777777).all()
        assert (short.to_host(np.uint8) == GUARD).all() and h.untouched(h.q) and h.intact(h.c), "a refused call wrote to a buffer"
        _check_against_horner(h, coeffs, z_wire, z_plain)
    finally:
        short.free()
        h.close()


@pytest.mark.gpu
def test_scratch_is_reused_and_released(gm):
    tile, _ = _shape()
    n, batch = 5 * tile - 7, 4
    z_wire, _ = _point(0, 12)
    coeffs = _coeffs(0, n, batch, 0xF300)
    h = Harness(gm, 0, n, batch)
    try:
        h.divide(coeffs, z_wire)  # whatever the runtime keeps from a kernel's first launch is there before the baseline is read
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        before = free_bytes(h.lib)
        q1, r1 = h.divide(coeffs, z_wire)
        first = free_bytes(h.lib)
        q2, r2 = h.divide(coeffs, z_wire)
        assert free_bytes(h.lib) == first, "a repeated identical call allocated"
        v = h.evaluate(coeffs, z_wire)  # needs no more scratch than the division
        assert free_bytes(h.lib) == first
        assert np.array_equal(q1, q2) and np.array_equal(r1, r2) and np.array_equal(v[:, 0], r1)
        ffi.check(h.lib.panda_ntt_tear_down(), "tear_down")
        assert free_bytes(h.lib) == before, "panda_ntt_tear_down releases the scratch"
    finally:
        h.close()


@pytest.mark.gpu
def test_gpu_manager_helpers(gm):
    tile, _ = _shape()
    n, batch = tile + 3, 3
    wires, plains = _eval_points(0)
    coeffs = _coeffs(0, n, batch, 0xF400)
    polys = [np.array(c) for c in coeffs]
    vals = pgm.panda_poly_gpu_evaluate(gm, polys, wires[:2])
    assert vals.shape == (batch, 2, 8) and vals.dtype == np.uint32
    quotients, rems = pgm.panda_poly_gpu_divide(gm, polys, wires[0])
    assert len(quotients) == batch and rems.shape == (batch, 8)
    for p in range(batch):
        want_q, want_r = _horner(0, coeffs[p], plains[0])
        assert quotients[p].shape == (n, 8) and np.array_equal(quotients[p], want_q) and np.array_equal(rems[p], want_r)
        assert np.array_equal(vals[p, 0], want_r) and np.array_equal(vals[p, 1], _horner(0, coeffs[p], plains[1])[1])
        assert np.array_equal(polys[p], coeffs[p]), "a helper changed its input"
    empty = pgm.panda_poly_gpu_evaluate(gm, [], wires[:2])
    assert empty.shape == (0, 2, 8)
    q0, r0 = pgm.panda_poly_gpu_divide(gm, [], wires[0])
    assert q0 == [] and r0.shape == (0, 8)
