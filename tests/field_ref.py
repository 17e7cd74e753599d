"""Wire elements of the three scalar fields, in Python integers: what the tests of the scalar-field calls share.

A residue x of field 0, 1 or 2 (the Fr of BN254, BLS12-377, BLS12-381; the field id is the curve id) goes over the wire as the 32
little-endian bytes of w = x W mod r, W = 2^256.  `words` / `ints` move between integers and (n, 8) uint32 rows as they stand, `wire` /
`plain` between plain residues and wire rows."""
import functools

import numpy as np

import oracle as po
import pyref

W = 1 << 256


@functools.lru_cache(maxsize=None)
def modulus(field):
    return pyref.limbs_to_int(po.field_info(po.FR_OF[field])["p"])


def words(vals):
    """256-bit integers -> (len, 8) uint32, read-only"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint32).reshape(-1, 8)


def ints(a):
    """(m, 8) uint32 -> m Python integers (the residues as they stand on the wire)"""
    raw = np.ascontiguousarray(a, np.uint32).reshape(-1, 8).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def wire(field, vals):
    """integers -> their residues' wire words (len, 8), read-only"""
    r = modulus(field)
    return words([v % r * W % r for v in vals])


def wire_one(field, v):
    """one integer -> the (8,) wire words of its residue, writable"""
    return wire(field, [v])[0].copy()


def plain(field, a):
    """wire words (m, 8) -> m plain residues"""
    r = modulus(field)
    winv = pow(W, -1, r)
    return [w * winv % r for w in ints(a)]


def random_residues(field, seed, n, nonzero=False):
    """n plain residues from the seed: 40-byte little-endian draws reduced mod r; nonzero maps 0 to 1"""
    r = modulus(field)
    raw = np.random.default_rng(seed).bytes(40 * n)
    vals = [int.from_bytes(raw[40 * j:40 * j + 40], "little") % r for j in range(n)]
    return [v or 1 for v in vals] if nonzero else vals


def random_rows(field, seed, batch, n, nonzero=False):
    """(batch, n) plain residues as nested lists: random_residues(field, seed, batch * n) cut into rows"""
    vals = random_residues(field, seed, batch * n, nonzero)
    return [vals[p * n:(p + 1) * n] for p in range(batch)]


@functools.lru_cache(maxsize=None)
def shift_powers(field, n, g):
    """g^j, j < n, as wire words (n, 8), read-only"""
    r = modulus(field)
    pw, acc = [], 1
    for _ in range(n):
        pw.append(acc)
        acc = acc * g % r
    return wire(field, pw)
