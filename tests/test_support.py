"""tests/field_ref.py and the guarded buffers of tests/gpu_util.py: the support code the other test modules stand on.

The wire forms are checked against a second route through tests/pyref.py, the generator against values recorded from the per-module
generators it replaced, and the guard checks by writing one byte where they must notice it."""
import ctypes as C

import numpy as np
import pytest

import field_ref as fr
import pyref
from gpu_util import GUARD, GUARD_BYTES, GuardedBuffers, gm  # noqa: F401
from panda_amd import gpu_ffi as ffi

FIELDS = (0, 1, 2)
# (field, seed) -> the first three values of the generators the shared one replaced
RECORDED = {
    (0, 0x2B001): (0x1d73b2b772faa0acfd0c85ae39822b22c8327c0cb239ccac8c57ffe8f7f47a6, 0x116a7b4af1680bafe3ec8684e2004e6a521538225119ead7ff50b977edc77dd6,
                   0x26189bc48836a299a8ce3391de38459b314f9b56f2415d50ead56dac975e8842),
    (1, 0x9A010): (0x4a0c80282a22675951d546a4c68f284b8449f8f15322689d299577d579aa94d, 0xbc07fb312747736ba4ba5edfed1f7b7688497857a8c4a2fca9ce7d96e9c5de1,
                   0x3fb149f8af6888fc70f8fdc79533d778f8ab0c0037b1671f04f6fb0af27991c),
    (2, 7): (0x4f99673b2aba31722657b8b271b0973532cd06068ecb3e55b5fc16db323f3812, 0x43cab898d47db3377aac860502ca1eb494f2ded51196721f9801d5678811b314,
             0x2b72d4b8d65b0524c641a8c95c9664fb882e1e02d23250430af07d3bf66c6308),
    (0, 0): (0x1686a2000bd5e0e7653ac77b7d6438b61c276a66f5ff800466415ccba329ea1c, 0x13422f26d5c9dae5db5e11aa558e6db7ea965e68b3a1f54612011c4bf6e1e3e1,
             0x2522351d9c03eb271600c95f3cbad11d6c77f38aa3b8f56292ffaef09d2655f7),
}


def _values(field):
    r = fr.modulus(field)
    return [0, 1, r - 1, r, fr.W - 1] + [int.from_bytes(np.random.default_rng(0x5EED + field).bytes(32 * 40)[32 * j:32 * j + 32], "little") for j in range(40)]


@pytest.mark.parametrize("field", FIELDS)
def test_moduli_are_the_curves_scalar_fields(field):
    c = pyref.CURVES[field]
    assert fr.modulus(field) == c.r and fr.W % c.r == c.Rr, "a curve's id is its scalar field's"


@pytest.mark.parametrize("field", FIELDS)
def test_words_and_ints_are_inverse(field):
    v = _values(field)
    w = fr.words(v)
    assert w.shape == (len(v), 8) and w.dtype == np.uint32 and fr.ints(w) == v
    assert fr.words([]).shape == (0, 8) and fr.ints(fr.words([])) == []


@pytest.mark.parametrize("field", FIELDS)
def test_wire_and_plain(field):
    r, v = fr.modulus(field), _values(field)
    w = fr.wire(field, v)
    assert fr.plain(field, w) == [x % r for x in v]
    assert all(x < r for x in fr.ints(w)), "wire elements are canonical"
    for x, row in zip(v, w):  # the per-element route
        assert np.array_equal(row, pyref.int_to_limbs(x % r * fr.W % r, 8)), x
        assert pyref.decode_scalar(pyref.CURVES[field], row) == x % r
    one = fr.wire_one(field, v[7])
    assert one.shape == (8,) and one.dtype == np.uint32 and np.array_equal(one, w[7]) and np.array_equal(one, fr.wire(field, v[7:8])[0])
    one[0] ^= 1  # writable, and no view of anything shared
    assert np.array_equal(fr.wire_one(field, v[7]), w[7]) and not w.flags.writeable


def test_random_residues_are_the_recorded_values():
    for (field, seed), first in RECORDED.items():
        assert tuple(fr.random_residues(field, seed, 3)) == first, (field, seed)
        assert tuple(fr.random_residues(field, seed, 50)[:3]) == first, "a longer draw begins with the shorter one"


@pytest.mark.parametrize("field", FIELDS)
def test_random_residues_and_rows(field):
    r = fr.modulus(field)
    flat = fr.random_residues(field, 0x77 + field, 12)
    assert flat == fr.random_residues(field, 0x77 + field, 12) and flat != fr.random_residues(field, 0x78 + field, 12)
    assert len(set(flat)) == 12 and all(0 <= x < r for x in flat)
    assert fr.random_rows(field, 0x77 + field, 3, 4) == [flat[0:4], flat[4:8], flat[8:12]]
    assert fr.random_rows(field, 0x77 + field, 3, 4, nonzero=True) == [flat[0:4], flat[4:8], flat[8:12]], "no zero among them: nothing to map"
    assert fr.random_residues(field, 1, 0) == [] and fr.random_rows(field, 1, 2, 0) == [[], []]


def test_nonzero_maps_zero_to_one(monkeypatch):
    class Zeros:
        def bytes(self, n):
            return b"\0" * (n - 40) + (5).to_bytes(40, "little")

    monkeypatch.setattr(np.random, "default_rng", lambda seed: Zeros())
    assert fr.random_residues(0, 0, 3) == [0, 0, 5] and fr.random_residues(0, 0, 3, nonzero=True) == [1, 1, 5]
    assert fr.random_rows(0, 0, 1, 3, nonzero=True) == [[1, 1, 5]]


@pytest.mark.parametrize("field", FIELDS)
def test_shift_powers(field):
    r = fr.modulus(field)
    pw = fr.shift_powers(field, 9, 5)
    assert pw.shape == (9, 8) and fr.plain(field, pw) == [pow(5, j, r) for j in range(9)] and not pw.flags.writeable
    assert fr.shift_powers(field, 0, 5).shape == (0, 8)


def _poke(d, offset):
    """one byte that is not the guard byte, written by the library's own memset"""
    ffi.check(ffi.load().panda_memset(C.c_void_p(d.ptr.value + offset), GUARD ^ 0xFF, 1), "memset")


@pytest.mark.gpu
def test_guarded_buffers_notice_one_byte(gm):
    h = GuardedBuffers()
    try:
        x = np.arange(8, dtype=np.uint32)
        for data in (x, x[:0]):
            src, out = h.buffer(data), h.buffer(nbytes=data.nbytes)
            assert src.data_bytes == out.data_bytes == data.nbytes and src.nbytes == data.nbytes + GUARD_BYTES
            assert h.intact(src) and h.intact(out) and h.untouched(out) and h.guard_intact(src) and h.guard_intact(out)
            assert np.array_equal(h.get(src), data) and h.get(out).shape == (data.size,)
            assert not h.untouched(src) or data.size == 0, "an uploaded buffer is not the fill byte throughout"
            _poke(out, out.data_bytes)  # the first guard byte: inside the allocation
            assert not h.guard_intact(out) and not h.intact(out) and not h.untouched(out)
            h.fill(out)
            assert h.intact(out) and h.untouched(out), "fill() restores a buffer"
            _poke(src, src.data_bytes + GUARD_BYTES - 1)  # the last one
            assert not h.guard_intact(src) and not h.intact(src)
            h.fill(src, data)
            assert h.intact(src)
        src = h.buffer(x)
        _poke(src, 13)
        assert h.guard_intact(src) and not h.intact(src), "a changed input with its guard whole"
        _poke(out, 0)  # zero-length data: offset 0 is the guard's first byte
        assert not h.guard_intact(out)
        assert len(h.bufs) == 5
    finally:
        h.close()
    assert h.bufs == []
