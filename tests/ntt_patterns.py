"""Structured NTT inputs that drive the transform kernels' lazy-reduction chain to its edges, with closed forms of their outputs.

Uniformly random canonical elements never do: a sum of 2^r of them sits near 2^(r-1) p and never near the 2^r p the bound plan allows, a
difference of two such sums is never near -2^r p (where the bias K p is needed), and no intermediate value is ever a multiple of p.
Constant columns, padding zeros, 0 / 1 indicator columns and single coefficients -- what provers really send -- are all of that.

Patterns are defined on the WIRE value, the 256-bit integer in the buffer.  The kernels keep the caller's Montgomery radix, so the wire
limbs are the internal limbs, and the transform is linear on wire values with the decoded root w:  Y[k] = sum_j X[j] w^(jk) mod r.
Every pattern is canonical (< r).  Nothing in this module calls the CPU oracle or needs a GPU: the closed forms are Python integers.

Families (n = 2^log_n, v one of edge_values()):
    zeros                all zero                                   -> all zero
    const(v)             every x[j] = v                             -> n v at k = 0, exact zeros elsewhere (cancellation in every round)
    delta(j, v)          v at index j, zero elsewhere               -> y[k] = v w^(jk)
    geom(k0, v)          x[j] = v w^(-j k0)                         -> n v at k0, exact zeros elsewhere
    bit(t, v)            v where bit t of j is 0, zero elsewhere    -> zero except at k = 0 and the odd multiples of n / 2^(t+1)
    bit_c(t, v)          v where bit t of j is 1, zero elsewhere    -> likewise; bit + bit_c = const
    mask(seed)           seeded 0 / (r - 1) coin flips
    near_top(seed)       r - 1 - (seeded 16-bit value)
For t = log_n - 1 - rho, round rho of the first pass sees a = 2^rho v and b = 0 under bit(t, v) and the reverse under bit_c(t, v): the
two extremes of the a - b + K p path; const(v) gives the extreme of the sum path and a - b = 0 with a != 0."""
from __future__ import annotations

import collections

import numpy as np

import pyref

FIELDS = (pyref.BN254, pyref.BLS12_377, pyref.BLS12_381)


class Pattern(collections.namedtuple("Pattern", "family args")):
    @property
    def name(self):
        return self.family + "(" + ",".join(str(a) for a in self.args) + ")"


def modulus(field: int) -> int:
    return pyref.CURVES[field].r


def edge_values(field: int) -> dict:
    """the wire values the families are filled with: 1, r - 1, and 2^(bitlen(r) - 1) - 1 (below r, every low limb saturated)"""
    r = modulus(field)
    return {"one": 1, "top": r - 1, "sat": (1 << (r.bit_length() - 1)) - 1}


def _value(field, v):
    return edge_values(field)[v] if isinstance(v, str) else int(v)


def to_limbs(ints) -> np.ndarray:
    """Python integers below 2^256 -> (len, 8) uint32, little-endian limbs"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint32).reshape(-1, 8).copy()


def to_ints(a) -> list:
    """(len, 8) uint32 -> Python integers"""
    buf = np.ascontiguousarray(a, dtype=np.uint32).tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def bit_reverse_permutation(log_n: int) -> np.ndarray:
    idx = np.arange(1 << log_n, dtype=np.int64)
    out = np.zeros_like(idx)
    for b in range(log_n):
        out |= ((idx >> b) & 1) << (log_n - 1 - b)
    return out


def add_mod(a, b, field: int) -> np.ndarray:
    """(a + b) mod r row by row on (len, 8) uint32 limbs of canonical values: exact integer arithmetic (64-bit limb sums with explicit
    carries and borrows), for buffers too long to walk with Python integers; test_ntt_patterns.py pins it to Python integers"""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    r = to_limbs([modulus(field)])[0].astype(np.uint64)
    s = np.empty(a.shape, dtype=np.uint64)
    carry = np.zeros(a.shape[0], dtype=np.uint64)
    for i in range(8):
        t = a[:, i].astype(np.uint64) + b[:, i].astype(np.uint64) + carry
        s[:, i] = t & np.uint64(0xFFFFFFFF)
        carry = t >> np.uint64(32)
    assert not carry.any(), "operands are canonical and r < 2^255: the sum fits 256 bits"
    d = np.empty(a.shape, dtype=np.uint64)
    borrow = np.zeros(a.shape[0], dtype=np.uint64)
    for i in range(8):
        t = s[:, i] + np.uint64(1 << 32) - r[i] - borrow
        d[:, i] = t & np.uint64(0xFFFFFFFF)
        borrow = np.uint64(1) - (t >> np.uint64(32))
    return np.where((borrow == 0)[:, None], d, s).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the inputs
def build(p: Pattern, field: int, log_n: int, w: int | None = None) -> np.ndarray:
    """the pattern as an (n, 8) uint32 array of wire words; `w` is the decoded root of the transform (geom only)"""
    r, n = modulus(field), 1 << log_n
    x = np.zeros((n, 8), dtype=np.uint32)
    if p.family == "zeros":
        return x
    if p.family == "const":
        x[:] = to_limbs([_value(field, p.args[0])])[0]
    elif p.family == "delta":
        x[p.args[0]] = to_limbs([_value(field, p.args[1])])[0]
    elif p.family == "geom":
        step, acc, vals = pow(w, (n - p.args[0]) % n, r), _value(field, p.args[1]), []
        for _ in range(n):
            vals.append(acc)
            acc = acc * step % r
        x = to_limbs(vals)
    elif p.family in ("bit", "bit_c"):
        sel = ((np.arange(n) >> p.args[0]) & 1) == (1 if p.family == "bit_c" else 0)
        x[sel] = to_limbs([_value(field, p.args[1])])[0]
    elif p.family == "mask":
        x[np.random.default_rng(p.args[0]).integers(0, 2, n).astype(bool)] = to_limbs([r - 1])[0]
    elif p.family == "near_top":
        table = to_limbs([r - 1 - d for d in range(1 << 16)])
        x = table[np.random.default_rng(p.args[0]).integers(0, 1 << 16, n)]
    else:
        raise ValueError(p.family)
    return x


# ------------------------------------------------------------------------------------------------------------ the closed forms
def closed_form(p: Pattern, field: int, log_n: int, w: int, inverse: bool = False):
    """Python integers of the output on the wire.  Forward: Y[k] = sum_j X[j] w^(jk); inverse: Y[k] = n^-1 sum_j X[j] w^(-jk), for the SAME
    input (geom is always built with the forward root, so its peak moves to n - k0).  Returns ("sparse", {k: value}) -- every other row is
    zero -- for zeros, const and geom, ("dense", [values]) for delta, None for the families without one."""
    r, n = modulus(field), 1 << log_n
    gain = 1 if inverse else n  # n v forward; n^-1 n v = v inverse
    if p.family == "zeros":
        return "sparse", {}
    if p.family == "const":
        return "sparse", {0: gain * _value(field, p.args[0]) % r}
    if p.family == "geom":
        return "sparse", {((n - p.args[0]) % n if inverse else p.args[0]): gain * _value(field, p.args[1]) % r}
    if p.family == "delta":
        j, v = p.args[0], _value(field, p.args[1])
        step = pow(w, (n - j) % n if inverse else j, r)
        acc, vals = (v * pow(n, -1, r) % r if inverse else v), []
        for _ in range(n):
            vals.append(acc)
            acc = acc * step % r
        return "dense", vals
    return None


def zero_support(p: Pattern, log_n: int):
    """boolean mask over the output rows that are exactly zero under bit / bit_c (forward or inverse, natural order): x depends on bit t of
    j alone, so it has period 2^(t+1) and its spectrum lives on the multiples of n / 2^(t+1); it is a constant plus a square wave that
    changes sign under a shift by 2^t, which has odd harmonics only.  Non-zero exactly at k = 0 and the odd multiples of n / 2^(t+1).
    None for the other families."""
    if p.family not in ("bit", "bit_c"):
        return None
    k, step = np.arange(1 << log_n), (1 << log_n) >> (p.args[0] + 1)
    return ~((k == 0) | ((k % step == 0) & ((k // step) % 2 == 1)))


# ------------------------------------------------------------------------------------------------------------ the sets
def seeded_index(log_n, seed):
    return int(np.random.default_rng(seed).integers(0, 1 << log_n))


def bit_pair(t, v="top"):
    return [Pattern("bit", (t, v)), Pattern("bit_c", (t, v))]


def full_set(log_n: int, seed: int = 0x5EED) -> list:
    """every family at every edge value, every index bit: what the sizes up to 2^13 run"""
    n = 1 << log_n
    out = [Pattern("zeros", ())]
    out += [Pattern("const", (v,)) for v in ("one", "top", "sat")]
    for j in sorted({0, 1 % n, n // 2, n - 1}):
        out += [Pattern("delta", (j, v)) for v in ("one", "top", "sat")]
    for k0 in sorted({1 % n, n // 2, n - 1, seeded_index(log_n, seed)}):
        out += [Pattern("geom", (k0, v)) for v in ("one", "top", "sat")]
    for t in range(log_n):
        for v in ("one", "top", "sat"):
            out += bit_pair(t, v)
    out += [Pattern("mask", (seed + log_n,)), Pattern("near_top", (seed + 64 + log_n,))]
    return out


def reduced_set(log_n: int, seed: int = 0x5EED) -> list:
    """2^16 and above: zeros, the three constants, two geometric and two delta members, bit / bit_c of the top nine bits (every round of a
    radix-256 or radix-512 first pass, and the top round of the second pass) and of bit 0, one mask"""
    n = 1 << log_n
    out = [Pattern("zeros", ())] + [Pattern("const", (v,)) for v in ("top", "one", "sat")]
    out += [Pattern("geom", (1, "top")), Pattern("geom", (seeded_index(log_n, seed), "sat"))]
    out += [Pattern("delta", (1, "top")), Pattern("delta", (n - 1, "sat"))]
    for t in list(range(log_n - 1, log_n - 10, -1)) + [0]:
        out += bit_pair(t)
    out.append(Pattern("mask", (seed + log_n,)))
    return out


def field_set(log_n: int, first_pass_bits: int, seed: int = 0x5EED) -> list:
    """the other two fields: zeros, const(r - 1), const(saturated), one geom, bit / bit_c of the top bit and of the top bit of the second
    pass (where there is one), one mask"""
    out = [Pattern("zeros", ()), Pattern("const", ("top",)), Pattern("const", ("sat",)), Pattern("geom", (seeded_index(log_n, seed), "top"))]
    out += bit_pair(log_n - 1)
    if log_n - 1 - first_pass_bits >= 0:
        out += bit_pair(log_n - 1 - first_pass_bits)
    out.append(Pattern("mask", (seed + log_n,)))
    return out


def single_set(log_n: int, seed: int = 0x5EED) -> list:
    """what also goes through the single calls: const(r - 1), zeros, one geom, bit / bit_c of the top bit and of bit 0"""
    out = [Pattern("const", ("top",)), Pattern("zeros", ()), Pattern("geom", (seeded_index(log_n, seed), "top"))]
    for t in sorted({log_n - 1, 0}):
        out += bit_pair(t)
    return out


# ------------------------------------------------------------------------------------------------------------ what a pattern reaches
def first_pass_chain(tile) -> list:
    """A plain un-reduced radix-2 DIF over one tile of the first pass (Python integers, tile[i] = X[column + i n / 2^d]), followed along
    its twiddle-free chain: round rho pairs position 0 of the running sums with its partner 2^(d-1-rho) (i = 0 and i = 128 >> rho
    (mod 256 >> rho) in the radix-256 kernel's indexing), both of which have only been added so far.  Returns [(a, b)] per round."""
    s, out = [int(v) for v in tile], []
    while len(s) > 1:
        half = len(s) // 2
        out.append((s[0], s[half]))
        s = [s[q] + s[q + half] for q in range(half)]
    return out


def chain_columns(log_n: int, first_pass_bits: int, seed: int = 0x5EED) -> list:
    """the columns of the first pass the reach tests look at: those holding index 0, 1 and n - 1, and one seeded"""
    stride = 1 << (log_n - first_pass_bits)
    return sorted({0, 1 % stride, stride - 1, seeded_index(log_n - first_pass_bits, seed)})


def reach(x, log_n: int, first_pass_bits: int, columns) -> list:
    """per round of the first pass, the (a, b) pairs of first_pass_chain over the given columns of the (n, 8) input x"""
    stride = 1 << (log_n - first_pass_bits)
    rounds = [[] for _ in range(first_pass_bits)]
    for c in columns:
        for rho, ab in enumerate(first_pass_chain(to_ints(x[c::stride]))):
            rounds[rho].append(ab)
    return rounds
