"""The NTT kernels on the structured inputs of ntt_patterns.py: constants, zeros, single coefficients, geometric sequences, 0 / v indicator
columns of every index bit, 0 / (r - 1) masks.  They drive the lazy-reduction chain of the passes (the compile-time bound plan, the
carry schedule by round parity, the unit-twiddle path that keeps a - b + K p, the final reductions) to the edges uniformly random
inputs never come near (test_ntt_patterns.py shows both), and most of their outputs are exact zeros reached through cancellation.

Every comparison is bit-exact on whole buffers.  Expected values: the CPU oracle's transform of every member; the Python-integer
closed forms of ntt_patterns.py where there is one; the device's own outputs of bit + bit_c against its output of const; and the
inverse of every forward output against the input.  Expected zeros are asserted as whole rows, so a stray p shows as such.

Sizes are the smallest that reach each kernel instance (test_sizes_cover_every_kernel_instance asserts it from the library's plan):
2^1 .. 2^10 k_ntt_pass (one pass and 8 + 2), 2^11 first k_ntt_pass8 + k_ntt_small<3>, 2^12 / 2^13 a shortened last k_ntt_pass8, 2^16 8 + 8,
2^17 / 2^18 k_ntt_pass9 first and last (k_ntt_small<2> in 2^18's bit-reversed plan), 2^19 a middle pass with the inter-pass product in
both spellings (streamed table and two small tables); the slab steps run k_ntt_small<1 .. 3> as the size-G transform."""
import collections
import concurrent.futures
import ctypes as C
import functools
import os

import numpy as np
import pytest

import field_ref as fr
import ntt_patterns as pat
import oracle as po
import pyref
import test_ntt_batch as tb
import test_ntt_lde as tl
from gpu_util import gm  # noqa: F401
from panda_amd import gpu_ffi as ffi

FORWARD, INVERSE, BITREV_OUT, INVERSE_BITREV_IN, COSET, COSET_INVERSE = tb.KINDS
INVERSE_OF = {FORWARD: INVERSE, BITREV_OUT: INVERSE_BITREV_IN, COSET: COSET_INVERSE}
INVERSE_KINDS = (INVERSE, INVERSE_BITREV_IN, COSET_INVERSE)
SHIFT = tb.SHIFT
SMALL_SIZES = (1, 3, 8, 9, 10, 11, 12, 13)
LARGE_SIZES = (16, 17, 18, 19)
FIELD_SIZES = (3, 10, 11, 12, 16, 17, 19)
SLAB_SHAPES = ((1, 6), (2, 12), (3, 15))
ONE_PROCESS_SHAPE = (3, 18)
DENSE_CLOSED_FORM_MAX = 13  # above 2^13 points the dense (delta) closed form is built for FORWARD only; the oracle covers the rest


def _plan(log_n):
    passes, bits = C.c_uint(0), (C.c_uint * 4)()
    ffi.check(ffi.load().panda_ntt_pass_plan(log_n, C.byref(passes), bits), "plan")
    return [bits[j] for j in range(passes.value)]


def _launches(log_n, kind):
    rc, launches, _ = tb._plan(ffi.load(), log_n, kind, 1)
    assert rc == 0
    return launches


def test_sizes_cover_every_kernel_instance():
    """a later change of plan_passes cannot silently empty the matrix: from 2^11 on a pass of 8 (9) bits is k_ntt_pass8 (k_ntt_pass9), a
    last pass of 4 .. 7 bits k_ntt_pass8 with its first rounds off, a last pass of 1 .. 3 bits k_ntt_small"""
    plans = {k: _plan(k) for k in set(SMALL_SIZES + LARGE_SIZES + FIELD_SIZES)}
    regs = {k: p for k, p in plans.items() if k >= 11}
    assert {k for k, p in plans.items() if k < 11 and len(p) == 1} >= {1, 3, 8} and plans[9] == [8, 1] and plans[10] == [8, 2]  # k_ntt_pass
    assert {k for k, p in regs.items() if p[0] == 8 and len(p) > 1} >= {11, 12, 16, 19}, "first radix-256 pass"
    assert [k for k, p in regs.items() if len(p) >= 3 and p[1] == 8] == [19], "middle radix-256 pass"
    assert {k for k, p in regs.items() if p[-1] == 8} >= {16, 17}, "last radix-256 pass"
    assert {k for k, p in regs.items() if p[0] == 9} == {17, 18}, "first radix-512 pass"
    assert {k for k, p in regs.items() if p[-1] == 9} == {18}, "last radix-512 pass"
    assert _launches(17, INVERSE_BITREV_IN) == 2 and _launches(17, BITREV_OUT) == 2  # 8 + 9 and 9 + 8
    assert {k: p[-1] for k, p in regs.items() if 4 <= p[-1] <= 7} == {12: 4, 13: 5}, "shortened last pass"
    assert plans[11] == [8, 3] and plans[19] == [8, 8, 3], "radix 8 in k_ntt_small"
    assert _launches(18, BITREV_OUT) == 3 and _launches(18, INVERSE_BITREV_IN) == 3, "radix 4 in k_ntt_small: 2^18 bit-reversed is 8 + 8 + 2"
    assert {g for g, _ in SLAB_SHAPES + (ONE_PROCESS_SHAPE,)} == {1, 2, 3}, "radix 2, 4, 8 in k_ntt_small as the slab steps' size-G transform"
    assert set(FIELD_SIZES) >= {3, 10, 11, 12, 16, 17, 19}


# ------------------------------------------------------------------------------------------------------------ expected values
def _root(field, log_n):
    omega = po.root_of_unity(po.FR_OF[field], log_n)
    return omega, pyref.decode_scalar(pyref.CURVES[field], omega)


def _oracle_many(fid, xs, omega, log_n):
    """po.ntt of every member; po_ntt keeps no shared mutable state (its buffers are its own, the field tables constant), and ctypes
    releases the interpreter lock, so the members run in a pool of at most 16 threads"""
    xs = [np.ascontiguousarray(x) for x in xs]
    workers = max(1, min(16, len(xs), os.cpu_count() or 1))
    if workers == 1 or log_n < 12:
        return np.stack([po.ntt(fid, x, omega, log_n) for x in xs])
    with concurrent.futures.ThreadPoolExecutor(workers) as pool:
        return np.stack(list(pool.map(lambda x: po.ntt(fid, x, omega, log_n), xs)))


def _patterns(field, log_n, which, part):
    if which == "full":
        return pat.full_set(log_n)
    if which == "field":
        return pat.field_set(log_n, _plan(log_n)[0])
    full = pat.reduced_set(log_n)
    bits = [p for p in full if p.family in ("bit", "bit_c")]
    if part == 0:
        return [p for p in full if p.family not in ("bit", "bit_c")]
    return [pat.Pattern("const", ("top",))] + (bits[:10] if part == 1 else bits[10:])  # the constant the pairs have to add up to


Case = collections.namedtuple("Case", "field log_n patterns x y")


@functools.lru_cache(maxsize=2)
def _case(field, log_n, which, part=0):
    """the inputs of one batch and the oracle's forward transform of each, computed once and shared by the kinds, read-only"""
    omega, w = _root(field, log_n)
    pats = _patterns(field, log_n, which, part)
    x = np.stack([pat.build(p, field, log_n, w) for p in pats])
    y = _oracle_many(po.FR_OF[field], x, omega, log_n)
    x.setflags(write=False)
    y.setflags(write=False)
    return Case(field, log_n, pats, x, y)


@functools.lru_cache(maxsize=2)
def _coset_oracle(field, log_n, which):
    """the oracle's transform of x[j] g^j"""
    cs = _case(field, log_n, which)
    fid = po.FR_OF[field]
    pw = fr.shift_powers(field, 1 << log_n, SHIFT)
    omega, _ = _root(field, log_n)
    return _oracle_many(fid, [po.f_vec(fid, po.OP_MUL, np.ascontiguousarray(m), pw) for m in cs.x], omega, log_n)


def _wire_const(field, value, n):
    """`value` (a plain integer: a factor on wire values) as n rows of Montgomery-form words, the second operand of the oracle's product"""
    return np.tile(fr.wire_one(field, value), (n, 1))


@functools.lru_cache(maxsize=8)
def _inverse_shift_powers(field, n):
    r = pat.modulus(field)
    gi, acc, vals = pow(SHIFT, -1, r), 1, []
    for _ in range(n):
        vals.append(acc * (1 << 256) % r)
        acc = acc * gi % r
    return pat.to_limbs(vals)


def _expected(cs, which, kind):
    """the oracle's value of `kind` on cs.x, natural order: the inverse kinds through Y_inv[k] = n^-1 Y[-k mod n]"""
    fid, n = po.FR_OF[cs.field], 1 << cs.log_n
    if kind in (FORWARD, BITREV_OUT):
        return cs.y
    if kind == COSET:
        return _coset_oracle(cs.field, cs.log_n, which)
    back = (-np.arange(n)) % n
    ninv = _wire_const(cs.field, pow(n, -1, pat.modulus(cs.field)), n)
    out = np.stack([po.f_vec(fid, po.OP_MUL, np.ascontiguousarray(m[back]), ninv) for m in cs.y])
    if kind == COSET_INVERSE:
        out = np.stack([po.f_vec(fid, po.OP_MUL, m, _inverse_shift_powers(cs.field, n)) for m in out])
    return out


@functools.lru_cache(maxsize=8)
def _dense_closed(field, log_n, p, kind):
    return pat.to_limbs(_closed(p, field, log_n, kind)[1])


def _closed(p, field, log_n, kind):
    """ntt_patterns' closed form carried to `kind`: the coset kinds multiply input j (output k of the inverse) by g^j (g^-k)"""
    r = pat.modulus(field)
    _, w = _root(field, log_n)
    if kind == COSET:
        if p.family == "zeros":
            return "sparse", {}
        if p.family == "delta":
            f = pow(SHIFT, p.args[0], r)
            return "dense", [v * f % r for v in pat.closed_form(p, field, log_n, w)[1]]
        return None
    cf = pat.closed_form(p, field, log_n, w, inverse=kind in INVERSE_KINDS)
    if cf is None or kind != COSET_INVERSE:
        return cf
    gi = pow(SHIFT, -1, r)
    if cf[0] == "sparse":
        return "sparse", {k: v * pow(gi, k, r) % r for k, v in cf[1].items()}
    acc, vals = 1, []
    for v in cf[1]:
        vals.append(v * acc % r)
        acc = acc * gi % r
    return "dense", vals


def _check_member(p, got, field, log_n, kind):
    """one member's natural-order output against what is known without the oracle"""
    n = 1 << log_n
    if p.family == "delta" and (log_n <= DENSE_CLOSED_FORM_MAX or kind == FORWARD):
        assert np.array_equal(got, _dense_closed(field, log_n, p, kind)), (p.name, kind)
    elif p.family != "delta":
        cf = _closed(p, field, log_n, kind)
        if cf is not None:
            zero = np.ones(n, bool)
            for k, v in cf[1].items():
                zero[k] = False
                assert pat.to_ints(got[k:k + 1]) == [v], (p.name, kind, k)
            assert not got[zero].any(), f"{p.name}, kind {kind}: a row that is exactly zero came back non-zero"
    zs = pat.zero_support(p, log_n)
    if zs is not None and kind not in (COSET, COSET_INVERSE):
        assert not got[zs].any(), f"{p.name}, kind {kind}: a row that is exactly zero came back non-zero"


def _check_pairs(cs, got):
    """the device's outputs of bit and bit_c add, mod r, to its output of const (the transform is linear in every kind)"""
    index = {p: m for m, p in enumerate(cs.patterns)}
    for p, m in index.items():
        if p.family == "bit":
            other, whole = index[pat.Pattern("bit_c", p.args)], index[pat.Pattern("const", (p.args[1],))]
            assert np.array_equal(pat.add_mod(got[m], got[other], cs.field), got[whole]), p.name


def _run_kind(h, cs, which, kind, single=()):
    """one batch call of `kind` over the whole case, every check; the members in `single` also through the single call.  Returns the
    output as the device left it."""
    perm = pat.bit_reverse_permutation(cs.log_n)
    data = cs.x[:, perm] if kind == INVERSE_BITREV_IN else cs.x
    flag, raw = h.batch_call(kind, data)
    assert flag == h.expected_flag(kind)
    got = raw[:, perm] if kind == BITREV_OUT else raw
    want = _expected(cs, which, kind)
    for m, p in enumerate(cs.patterns):  # the closed forms first: they name a stray p, or a zero row that is not, as such
        _check_member(p, got[m], cs.field, cs.log_n, kind)
        assert np.array_equal(got[m], want[m]), (p.name, kind)
    _check_pairs(cs, got)
    for m, p in enumerate(cs.patterns):
        if p in single:
            sflag, out = h.single_call(kind, data[m])
            assert sflag == flag and np.array_equal(out, raw[m]), (p.name, kind, "single call")
    return raw


def _run_case(gm, cs, which, kinds, single):
    h = tb.Harness(gm, cs.field, cs.log_n, len(cs.patterns))
    try:
        for kind in kinds:
            raw = _run_kind(h, cs, which, kind, single)
            if kind in INVERSE_OF:  # the inverse of the device's output is the input, byte for byte
                flag, back = h.batch_call(INVERSE_OF[kind], raw)
                assert flag == h.expected_flag(INVERSE_OF[kind])
                assert np.array_equal(back, cs.x), kind
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------ whole transforms
@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [(FORWARD, INVERSE), (BITREV_OUT, INVERSE_BITREV_IN), (COSET, COSET_INVERSE)], ids=["natural", "bitrev", "coset"])
@pytest.mark.parametrize("log_n", SMALL_SIZES)
def test_bn254_full_set(gm, log_n, kinds):
    """every family at every edge value and index bit as the members of one batch call per kind; const(r - 1), zeros, one geom and bit /
    bit_c of the top bit and of bit 0 through the single calls (BATCH = false instances) as well"""
    _run_case(gm, _case(0, log_n, "full"), "full", kinds, set(pat.single_set(log_n)))


def _with_policy(policy, fn):
    lib = ffi.load()
    try:
        if policy == "two_tables":
            ffi.check(lib.panda_ntt_set_streamed_tables(0), "option")
        fn()
    finally:
        lib.panda_ntt_set_streamed_tables(0xFFFFFFFF)


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,policy", [(16, "built_in"), (17, "built_in"), (18, "built_in"), (19, "built_in"), (19, "two_tables")])
@pytest.mark.parametrize("part", [0, 1, 2], ids=["closed_forms_and_mask", "top_bits", "lower_bits_and_bit_0"])
def test_bn254_reduced_set(gm, log_n, policy, part):
    """2^16 .. 2^19 in three batches (the oracle's share of each stays within a few seconds): zeros, constants, geom, delta and a mask; bit /
    bit_c of the top five bits; of the next four and bit 0.  2^19 with the streamed inter-pass table and with the two small tables."""
    cs = _case(0, log_n, "reduced", part)
    single = {pat.Pattern("const", ("top",))} | set(pat.bit_pair(log_n - 1))
    _with_policy(policy, lambda: _run_case(gm, cs, "reduced", (FORWARD, INVERSE, BITREV_OUT), single))


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,policy", [(k, "built_in") for k in FIELD_SIZES] + [(19, "two_tables")])
@pytest.mark.parametrize("field", [1, 2], ids=["bls12_377", "bls12_381"])
def test_other_fields(gm, field, log_n, policy):
    """BLS12-377 and BLS12-381 Fr, batch and single calls; BLS12-381 at 2^19 under the built-in policy is the one instance whose inter-pass
    product reduces first (63 of 70 units of headroom spent)"""
    cs = _case(field, log_n, "field")
    _with_policy(policy, lambda: _run_case(gm, cs, "field", (FORWARD, INVERSE), set(cs.patterns)))


# ------------------------------------------------------------------------------------------------------------ low-degree extension
@pytest.mark.gpu
@pytest.mark.parametrize("order", tl.ORDERS, ids=["coset_major", "natural"])
@pytest.mark.parametrize("field,log_n,log_blowup", [(0, 11, 2), (0, 8, 4), (2, 11, 1)])
def test_lde(gm, field, log_n, log_blowup, order):
    """the constant polynomial r - 1 (every evaluation on every coset is r - 1), all coefficients r - 1, only the top coefficient, the
    zero polynomial; expected from the oracle's transform of the zero-padded, g^j-scaled coefficients at log2 N"""
    fid, n, log_big = po.FR_OF[field], 1 << log_n, log_n + log_blowup
    top = pat.to_limbs([pat.modulus(field) - 1])[0]
    coeffs = np.zeros((4, n, 8), np.uint32)
    coeffs[0, 0] = top
    coeffs[1, :] = top
    coeffs[2, n - 1] = top
    omega = po.root_of_unity(fid, log_big)
    pw = fr.shift_powers(field, n, SHIFT)
    padded = np.zeros((4, 1 << log_big, 8), np.uint32)
    for j in range(4):
        padded[j, :n] = po.f_vec(fid, po.OP_MUL, np.ascontiguousarray(coeffs[j]), pw)
    natural = _oracle_many(fid, padded, omega, log_big)
    h = tl.Harness(gm, field, log_n, log_blowup, 4)
    try:
        got = h.lde(coeffs, order)
        want = natural if order == tl.NATURAL else tl._to_coset_major(natural, log_n, log_blowup)
        assert np.array_equal(got, want)
        assert (got[0] == top).all(), "the constant polynomial r - 1 evaluates to r - 1 everywhere"
        assert not got[3].any(), "the zero polynomial"
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------ sharded steps
def _slab_patterns(log_ranks, log_n):
    """const(r - 1), zeros, one geom, bit / bit_c of the top log_ranks bits (half of every slab zero, the size-G transform's inputs
    cancel) and of the low log_ranks bits (whole slabs zero or constant: rank r holds x[r + G j])"""
    out = [pat.Pattern("const", ("top",)), pat.Pattern("zeros", ()), pat.Pattern("geom", (pat.seeded_index(log_n, 0x51AB), "top"))]
    for t in sorted(set(range(log_n - log_ranks, log_n)) | set(range(log_ranks))):
        out += pat.bit_pair(t)
    return out


def _slab_case(log_ranks, log_n):
    omega, w = _root(0, log_n)
    pats = _slab_patterns(log_ranks, log_n)
    x = np.stack([pat.build(p, 0, log_n, w) for p in pats])
    return Case(0, log_n, pats, x, _oracle_many(po.F_BN254_FR, x, omega, log_n))


def _slab_transform(gm, x, omega, log_ranks, log_n):
    """panda_ntt_slab_step1 / step2 with the all-to-all done on the host, every rank through this GPU one after the other"""
    from gpu_util import DeviceBuffer
    from panda_amd import multi_gpu
    lib = ffi.load()
    G, m = 1 << log_ranks, (1 << log_n) >> log_ranks

    def step(fn, host, rank):
        d_slab, d_scr = DeviceBuffer.from_host(host), DeviceBuffer(m * 32)
        try:
            flag = C.c_uint(7)
            cfg = ffi.NttSlabConfiguration(gm.exec_stream.raw, d_slab.ptr, d_scr.ptr, C.c_void_p(omega.ctypes.data), log_n, log_ranks, rank, C.pointer(flag))
            ffi.check(fn(cfg), "slab step")
            return (d_scr if flag.value else d_slab).to_host().reshape(m, 8)
        finally:
            d_slab.free()
            d_scr.free()

    after1 = [step(lib.panda_ntt_slab_step1_bn254, multi_gpu.slab_of(x, G, r), r) for r in range(G)]
    outs = [step(lib.panda_ntt_slab_step2_bn254, np.concatenate([after1[j][q * (m // G):(q + 1) * (m // G)] for j in range(G)]), q) for q in range(G)]
    return multi_gpu.natural_from_slab_outputs(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("log_ranks,log_n", SLAB_SHAPES)
def test_slab_steps(gm, log_ranks, log_n):
    """k_slab_twiddle and k_ntt_small as the size-G transform on slabs that are zero, constant or half zero"""
    cs = _slab_case(log_ranks, log_n)
    omega, _ = _root(0, log_n)
    got = np.stack([_slab_transform(gm, x, omega, log_ranks, log_n) for x in cs.x])
    for m, p in enumerate(cs.patterns):
        _check_member(p, got[m], 0, log_n, FORWARD)
        assert np.array_equal(got[m], cs.y[m]), p.name
    _check_pairs(cs, got)


@pytest.mark.gpu
def test_sharded_one_process(gm):
    """ntt_sharded_one_process and its inverse at (log_ranks, log_n) = (3, 18), every buffer on the device"""
    import torch
    from panda_amd import multi_gpu
    log_ranks, log_n = ONE_PROCESS_SHAPE
    G, m = 1 << log_ranks, (1 << log_n) >> log_ranks
    cs = _slab_case(log_ranks, log_n)
    omega, _ = _root(0, log_n)
    dev = torch.device("cuda", 0)
    got = []
    for x in cs.x:
        slabs = [torch.from_numpy(multi_gpu.slab_of(x, G, r).view(np.uint8).reshape(-1).copy()).to(dev) for r in range(G)]
        outs = multi_gpu.ntt_sharded_one_process(slabs, [torch.empty_like(t) for t in slabs], omega, log_n)
        got.append(multi_gpu.natural_from_slab_outputs([o.cpu().numpy().view(np.uint32).reshape(m, 8) for o in outs]))
        back = multi_gpu.intt_sharded_one_process([o.clone() for o in outs], [torch.empty_like(t) for t in outs], omega, log_n)
        for r in range(G):
            assert np.array_equal(back[r].cpu().numpy().view(np.uint32).reshape(m, 8), multi_gpu.slab_of(x, G, r)), r
    got = np.stack(got)
    for j, p in enumerate(cs.patterns):
        _check_member(p, got[j], 0, log_n, FORWARD)
        assert np.array_equal(got[j], cs.y[j]), p.name
    _check_pairs(cs, got)
