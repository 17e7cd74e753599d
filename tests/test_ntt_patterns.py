"""ntt_patterns.py without a GPU: its closed forms against the CPU oracle and against pyref's integers, and that the structured inputs
drive the first pass's lazy-reduction chain to the bounds the plan allows, where uniformly random inputs stay well inside them."""
import ctypes as C

import numpy as np
import pytest

import ntt_patterns as pat
import oracle as po
import pyref
from panda_amd import gpu_ffi as ffi


def _root(field, log_n):
    omega = po.root_of_unity(po.FR_OF[field], log_n)
    return omega, pyref.decode_scalar(pyref.CURVES[field], omega)


def _first_pass_bits(log_n):
    passes, bits = C.c_uint(0), (C.c_uint * 4)()
    ffi.check(ffi.load().panda_ntt_pass_plan(log_n, C.byref(passes), bits), "plan")
    return bits[0]


def _dense(cf, n):
    kind, vals = cf
    if kind == "dense":
        return pat.to_limbs(vals)
    out = np.zeros((n, 8), np.uint32)
    for k, v in vals.items():
        out[k] = pat.to_limbs([v])[0]
    return out


def test_edge_values_are_canonical_and_saturated():
    for field in pat.FIELDS:
        r, ev = pat.modulus(field), pat.edge_values(field)
        assert r == pyref.limbs_to_int(po.field_info(po.FR_OF[field])["p"])
        assert 0 < ev["one"] < ev["sat"] < ev["top"] == r - 1
        assert (pat.to_limbs([ev["sat"]])[0, :7] == 0xFFFFFFFF).all()


def test_add_mod_is_python_integer_addition():
    for field in pat.FIELDS:
        r = pat.modulus(field)
        vals = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, (1 << 32) - 1, 1 << 32, (1 << 224) - 1, pat.edge_values(field)["sat"]]
        vals += pat.to_ints(po.gen_scalars(po.FR_OF[field], 0x7A00 + field, 200))
        a = [u for u in vals for _ in vals]
        b = [v for _ in vals for v in vals]
        got = pat.to_ints(pat.add_mod(pat.to_limbs(a), pat.to_limbs(b), field))
        assert got == [(u + v) % r for u, v in zip(a, b)]


def test_bit_reverse_permutation():
    for log_n in (0, 1, 5, 11):
        want = [int(format(k, f"0{log_n}b")[::-1], 2) if log_n else 0 for k in range(1 << log_n)]
        assert pat.bit_reverse_permutation(log_n).tolist() == want


@pytest.mark.parametrize("field", pat.FIELDS)
@pytest.mark.parametrize("log_n", [1, 3, 8, 12])
def test_closed_forms_agree_with_the_oracle(field, log_n):
    """every member of the full set: the closed form where there is one (forward, and inverse through Y_inv[k] = n^-1 Y[-k]), the zero
    support of bit / bit_c, bit + bit_c = const, all patterns canonical"""
    fid, n, r = po.FR_OF[field], 1 << log_n, pat.modulus(field)
    omega, w = _root(field, log_n)
    ninv = pow(n, -1, r)
    back = (-np.arange(n)) % n
    outs = {}
    for p in pat.full_set(log_n):
        x = pat.build(p, field, log_n, w)
        assert x.shape == (n, 8) and x.dtype == np.uint32
        assert max(pat.to_ints(x)) < r, p.name
        y = po.ntt(fid, x, omega, log_n)
        outs[p] = y
        cf = pat.closed_form(p, field, log_n, w)
        if p.family in ("zeros", "const", "delta", "geom"):
            assert cf is not None
            assert np.array_equal(_dense(cf, n), y), p.name
            y_inv = pat.to_limbs([v * ninv % r for v in pat.to_ints(y[back])])
            assert np.array_equal(_dense(pat.closed_form(p, field, log_n, w, inverse=True), n), y_inv), p.name
        else:
            assert cf is None
        zs = pat.zero_support(p, log_n)
        if zs is not None:
            assert not y[zs].any(), p.name
            assert y[~zs].any(axis=1).all(), p.name  # and nowhere else
    for p, y in outs.items():
        if p.family == "bit":
            q = pat.Pattern("bit_c", p.args)
            assert np.array_equal(pat.add_mod(y, outs[q], field), outs[pat.Pattern("const", (p.args[1],))]), p.name


@pytest.mark.parametrize("field", pat.FIELDS)
def test_closed_forms_agree_with_pyref_integers(field):
    """pyref.dft on the wire integers with the decoded root, no oracle: the whole full set at 2^3 and 2^5, and at 2^10 (where the
    quadratic sum costs a second per dense input) the delta, geom and const members with v = r - 1"""
    c = pyref.CURVES[field]
    for log_n in (3, 5, 10):
        n = 1 << log_n
        _, w = _root(field, log_n)
        pw = [pow(w, e, c.r) for e in range(n)]
        for p in pat.full_set(log_n):
            cf = pat.closed_form(p, field, log_n, w)
            if cf is None or (log_n == 10 and (p.args[-1:] != ("top",) or (p.family == "delta" and p.args[0] != n - 1) or (p.family == "geom" and p.args[0] != 1))):
                continue
            x = pat.to_ints(pat.build(p, field, log_n, w))
            if log_n == 10:  # the same sum as pyref.dft over a power table, skipping the zero inputs
                nz = [(j, v) for j, v in enumerate(x) if v]
                want = [sum(v * pw[j * k % n] for j, v in nz) % c.r for k in range(n)]
            else:
                want = pyref.dft(c, x, w)
            assert pat.to_ints(_dense(cf, n)) == want, (p.name, log_n)


def test_const_and_geom_closed_forms_at_2_16():
    field, log_n = pyref.BN254, 16
    omega, w = _root(field, log_n)
    for p in (pat.Pattern("const", ("top",)), pat.Pattern("const", ("sat",)), pat.Pattern("geom", (1, "top")), pat.Pattern("geom", ((1 << 15) + 12345, "sat"))):
        y = po.ntt(po.FR_OF[field], pat.build(p, field, log_n, w), omega, log_n)
        (k, v), = pat.closed_form(p, field, log_n, w)[1].items()
        assert pat.to_ints(y[k:k + 1]) == [v] and v != 0
        y[k] = 0
        assert not y.any(), p.name


# ------------------------------------------------------------------------------------------------------------ reach
REACH_SIZES = [("full", k) for k in (1, 3, 8, 10, 11, 13)] + [("reduced", 16), ("reduced", 17)]


@pytest.mark.parametrize("field", pat.FIELDS)
@pytest.mark.parametrize("which,log_n", REACH_SIZES)
def test_patterns_reach_the_bounds_of_every_first_pass_round(field, which, log_n):
    """In every round rho the first pass runs at this size, over the twiddle-free chain of an un-reduced DIF: some pattern drives the sum
    to 2^(rho+1) (r - 1), some drive a - b to +2^rho (r - 1) and to -2^rho (r - 1), and some make a - b = 0 with a != 0."""
    r = pat.modulus(field)
    d = _first_pass_bits(log_n)
    assert d == (9 if log_n in (17, 18) else min(8, log_n))
    _, w = _root(field, log_n)
    cols = pat.chain_columns(log_n, d)
    rounds = [[] for _ in range(d)]
    for p in (pat.full_set(log_n) if which == "full" else pat.reduced_set(log_n)):
        for rho, pairs in enumerate(pat.reach(pat.build(p, field, log_n, w), log_n, d, cols)):
            rounds[rho] += pairs
    for rho, pairs in enumerate(rounds):
        assert max(a + b for a, b in pairs) == (2 << rho) * (r - 1), rho
        assert max(a - b for a, b in pairs) == (1 << rho) * (r - 1), rho
        assert min(a - b for a, b in pairs) == -(1 << rho) * (r - 1), rho
        assert any(a == b and a != 0 for a, b in pairs), rho


@pytest.mark.parametrize("field", pat.FIELDS)
@pytest.mark.parametrize("log_n", [3, 8, 11, 13])
def test_random_vectors_do_not(field, log_n):
    """64 seeded gen_scalars vectors (what every other whole-transform test feeds the kernels) over the same chain and columns: the sum
    stays below 2^(rho+1) (r - 1), the difference inside +-2^rho (r - 1), and no difference is zero.  How close they come is taken from
    the vectors themselves; from round 3 on the observed reach has to leave a tenth of the bound unused (a sum of 16 uniform residues has
    mean 8 r and standard deviation 1.16 r, so 0.9 of 16 r is more than five deviations out; the differences likewise)."""
    r = pat.modulus(field)
    d = _first_pass_bits(log_n)
    cols = pat.chain_columns(log_n, d)
    xs = po.gen_scalars(po.FR_OF[field], 0x7B00 + 16 * field + log_n, 64 << log_n).reshape(64, 1 << log_n, 8)
    rounds = [[] for _ in range(d)]
    for x in xs:
        for rho, pairs in enumerate(pat.reach(x, log_n, d, cols)):
            rounds[rho] += pairs
    for rho, pairs in enumerate(rounds):
        top = (1 << rho) * (r - 1)
        s_reach = max(a + b for a, b in pairs) / (2 * top)
        d_reach = max(abs(a - b) for a, b in pairs) / top
        msg = f"round {rho}: random sums reach {s_reach:.4f} of 2^{rho + 1} (r - 1), random differences {d_reach:.4f} of 2^{rho} (r - 1)"
        assert s_reach < 1 and d_reach < 1, msg
        assert all(a != b for a, b in pairs), msg
        if rho >= 3:
            assert s_reach < 0.9 and d_reach < 0.9, msg
