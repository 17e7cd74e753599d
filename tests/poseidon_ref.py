"""Poseidon in Python integers: the permutation, the sponge and the Merkle tree of panda_poseidon_* from their definitions in
include/panda_interface.h, on plain residues, and the parameter generator of the Poseidon paper (the Grain LFSR of its reference
script), so that known answers need no fixture file.

    round r of R_F + R_P:  s[j] += c[r][j];  s[j] <- s[j]^alpha for every j in a full round, for j = 0 in a partial one;  s <- M s

With n = 254, R_F = 8, alpha = 5 and R_P = 56, 57, 56, 60 for t = 2, 3, 4, 5 on BN254 the generator gives circomlib's constants, and
`hash` of [1], [1, 2], ... its published values (KNOWN_ANSWERS; tests/test_poseidon.py pins them)."""
import functools

import numpy as np

import field_ref as fr

ALPHAS = (5, 7, 11, 17)
# circomlib's partial rounds for t = 2 .. 5 (R_F = 8, alpha = 5, BN254) and poseidon([1 .. t - 1])
CIRCOMLIB_PARTIAL = {2: 56, 3: 57, 4: 56, 5: 60}
KNOWN_ANSWERS = {
    2: 0x29176100eaa962bdc1fe6c654d6a3c130e96a4d1168b33848b897dc502820133,
    3: 0x115cc0f5e7d690413df64c6b9662e9cf2a3617f2743245519e19607a4417189a,
    4: 0x0e7732d89e6939c0ff03d5e58dab6302f3230e269dc5b968f725df34ab36d732,
    5: 0x299c867db6c1fdd79dcefa40e4510b9837e60ebb1ce0663dbaa525df65250465,
}


class Params:
    """a parameter set on plain residues: rc[r][j], mds[i][j]"""

    def __init__(self, field, t, alpha, full_rounds, partial_rounds, rc, mds):
        self.field, self.p, self.t, self.alpha, self.rf, self.rp = field, fr.modulus(field), t, alpha, full_rounds, partial_rounds
        self.rc, self.mds = [list(row) for row in rc], [list(row) for row in mds]
        assert len(self.rc) == full_rounds + partial_rounds and all(len(row) == t for row in self.rc + self.mds) and len(self.mds) == t

    def rc_wire(self):
        return fr.wire(self.field, [c for row in self.rc for c in row])

    def mds_wire(self):
        return fr.wire(self.field, [m for row in self.mds for m in row])


def _grain_bits(n, t, rf, rp):
    """the generator's output bits: 80-bit state `1` in 2 bits, `0` in 4, n and t in 12 each, R_F and R_P in 10 each, thirty ones, MSB
    first; feedback b62 ^ b51 ^ b38 ^ b23 ^ b13 ^ b0 shifted in at the end; 160 bits discarded; then bits in pairs, the second of a pair
    is output iff the first is 1"""
    state = []
    for value, width in ((1, 2), (0, 4), (n, 12), (t, 12), (rf, 10), (rp, 10), ((1 << 30) - 1, 30)):
        state += [(value >> (width - 1 - k)) & 1 for k in range(width)]
    assert len(state) == 80
    pos = [0]  # the state is a window of a growing list

    def step():
        i = pos[0]
        bit = state[i + 62] ^ state[i + 51] ^ state[i + 38] ^ state[i + 23] ^ state[i + 13] ^ state[i]
        state.append(bit)
        pos[0] = i + 1
        return bit

    for _ in range(160):
        step()
    while True:
        first, second = step(), step()
        if first:
            yield second


@functools.lru_cache(maxsize=None)
def grain_params(field, t, rf, rp, alpha=5, n=None):
    """the paper's parameter set for the field: round constants of n bits big-endian, redrawn while >= p; then 2 t further draws taken
    mod p without redrawing, xs the first t, ys the last t, M[i][j] = 1 / (xs[i] + ys[j])"""
    p = fr.modulus(field)
    n = p.bit_length() if n is None else n
    bits = _grain_bits(n, t, rf, rp)

    def draw():
        v = 0
        for _ in range(n):
            v = (v << 1) | next(bits)
        return v

    rc = []
    while len(rc) < (rf + rp) * t:
        v = draw()
        if v < p:
            rc.append(v)
    xs = [draw() % p for _ in range(t)]
    ys = [draw() % p for _ in range(t)]
    mds = [[pow(xs[i] + ys[j], -1, p) for j in range(t)] for i in range(t)]
    return Params(field, t, alpha, rf, rp, [rc[r * t:(r + 1) * t] for r in range(rf + rp)], mds)


def circomlib(t):
    return grain_params(0, t, 8, CIRCOMLIB_PARTIAL[t], 5, 254)


def alpha_admissible(field, alpha):
    return alpha in ALPHAS and (fr.modulus(field) - 1) % alpha != 0


def random_params(field, seed, t, alpha, rf, rp):
    """random constants and a random matrix (the library does not ask for an MDS one)"""
    assert alpha_admissible(field, alpha)
    vals = fr.random_residues(field, seed, (rf + rp) * t + t * t)
    rc, m = vals[:(rf + rp) * t], vals[(rf + rp) * t:]
    return Params(field, t, alpha, rf, rp, [rc[r * t:(r + 1) * t] for r in range(rf + rp)], [m[i * t:(i + 1) * t] for i in range(t)])


def permute(P, state):
    p, t, s = P.p, P.t, [v % P.p for v in state]
    assert len(s) == t
    for r in range(P.rf + P.rp):
        s = [(s[j] + P.rc[r][j]) % p for j in range(t)]
        if r < P.rf // 2 or r >= P.rf // 2 + P.rp:
            s = [pow(v, P.alpha, p) for v in s]
        else:
            s[0] = pow(s[0], P.alpha, p)
        s = [sum(P.mds[i][j] * s[j] for j in range(t)) % p for i in range(t)]
    return s


def hash(P, message, tag=0):
    """the sponge: state (tag, 0, ..), chunks of t - 1 added into state[1 ..], the last one zero-padded, permuted after every chunk"""
    assert len(message) >= 1
    s = [tag % P.p] + [0] * (P.t - 1)
    for j0 in range(0, len(message), P.t - 1):
        for k, m in enumerate(message[j0:j0 + P.t - 1]):
            s[1 + k] = (s[1 + k] + m) % P.p
        s = permute(P, s)
    return s[0]


def merkle_levels(P, leaves, tag=0):
    """[level 1, level 2, .., [root]] of the tree of arity t - 1 over the leaves"""
    a, level, levels = P.t - 1, list(leaves), []
    while len(level) > 1:
        assert len(level) % a == 0
        level = [permute(P, [tag] + level[k:k + a])[0] for k in range(0, len(level), a)]
        levels.append(level)
    return levels


def wire_rows(field, vals):
    """plain residues -> (len, 8) uint32 wire rows, writable"""
    return np.array(fr.wire(field, vals))
