"""panda_poseidon_create / _destroy / _permute / _hash / _merkle_tree / _plan: Poseidon over the scalar fields.

    round r of R_F + R_P:  s[j] += c[r][j];  s[j] <- s[j]^alpha for every j in a full round, for j = 0 in a partial one;  s <- M s

Expected values are Python integers (tests/poseidon_ref.py: the definition on plain residues, and the Poseidon paper's parameter generator,
pinned here to circomlib's published hashes).  Results are canonical wire elements, so every comparison is byte for byte; there is no
tolerance anywhere.  The device routine also runs on the CPU (tests/host_check/poseidon_host.cpp builds panda_amd/csrc/poseidon.h for the
host with every bound asserted).  On the device every buffer carries a guard run behind the data, which no call may touch; inputs must
come back unchanged unless they are the output.  The permutations one workgroup covers (W) and the levels the single-workgroup kernel of
the tree takes come from the plan call.  The reference's values are computed once per parameter set and shared."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import field_ref as fr
import poseidon_ref as pr
from gpu_util import GuardedBuffers, assert_exported, free_bytes, gm, run_host_check  # noqa: F401
from panda_amd import gpu_ffi as ffi
from panda_amd import gpu_manager as pgm

CAP = 1 << 28
NAMES = ("panda_poseidon_create", "panda_poseidon_destroy", "panda_poseidon_permute", "panda_poseidon_hash", "panda_poseidon_merkle_tree",
         "panda_poseidon_plan")
STREAM = ffi.PandaStream()


def _plan(lib, width, height, offsets=True):
    per, nodes, top, launches = C.c_uint(0xDEAD), C.c_uint64(0xDEAD), C.c_uint(0xDEAD), C.c_uint(0xDEAD)
    off = (C.c_uint64 * max(height, 1))(*([0xDEAD] * max(height, 1)))
    rc = lib.panda_poseidon_plan(width, height, C.byref(per), C.byref(nodes), off if offsets else None, C.byref(top), C.byref(launches))
    return rc, per.value, nodes.value, list(off), top.value, launches.value


@functools.lru_cache(maxsize=None)
def _per_workgroup():
    rc, per, _, _, _, _ = _plan(ffi.load(), 3, 1)
    assert rc == 0 and per >= 64
    return per


@functools.lru_cache(maxsize=None)
def _top_levels(width):
    rc, _, _, _, top, _ = _plan(ffi.load(), width, 20 if width == 3 else 10)
    assert rc == 0 and top >= 2
    return top


@functools.lru_cache(maxsize=None)
def _set(name):
    """the parameter sets of the device tests: circomlib's for t = 2, 3, 5 on BN254, one random set on each other field"""
    if name.startswith("circomlib"):
        return pr.circomlib(int(name[-1]))
    return {"bls377": pr.random_params(1, 0x50001, 4, 17, 4, 3), "bls381": pr.random_params(2, 0x50002, 3, 5, 6, 9)}[name]


SETS = ("circomlib2", "circomlib3", "circomlib5", "bls377", "bls381")


def _create(P, field=None, **change):
    """-> (return code, handle) of panda_poseidon_create on the set P; `change` replaces struct fields"""
    rc_w, mds_w = P.rc_wire(), P.mds_wire()
    args = dict(width=P.t, alpha=P.alpha, full_rounds=P.rf, partial_rounds=P.rp, round_constants=rc_w.ctypes.data, mds=mds_w.ctypes.data)
    args.update(change)
    params = ffi.PoseidonParams(**args)
    handle = ffi.PandaPoseidon(0x7777)
    rc = ffi.load().panda_poseidon_create(P.field if field is None else field, C.byref(params), C.byref(handle))
    return rc, handle


# ------------------------------------------------------------------------------------------------- without a GPU
def test_symbols_in_header_ffi_and_library():
    header, _ = assert_exported(NAMES)
    assert int(re.search(r"#define\s+PANDA_POSEIDON_MAX_WIDTH\s+(\d+)", header).group(1)) == ffi.POSEIDON_MAX_WIDTH == 5
    assert re.search(r"typedef\s+struct\s+panda_poseidon_params", header) and re.search(r"typedef\s+struct\s+panda_poseidon\s*\{\s*void\s*\*handle;", header)
    assert [f[0] for f in ffi.PoseidonParams._fields_] == ["width", "alpha", "full_rounds", "partial_rounds", "round_constants", "mds"]
    assert C.sizeof(ffi.PoseidonParams) == 32 and ffi.PoseidonParams.round_constants.offset == 16 and C.sizeof(ffi.PandaPoseidon) == 8
    assert pgm.PandaPoseidon is not None


def test_reference_gives_circomlibs_published_values():
    for t in (2, 3, 4, 5):
        assert pr.hash(pr.circomlib(t), list(range(1, t))) == pr.KNOWN_ANSWERS[t], t
        assert pr.permute(pr.circomlib(t), list(range(t)))[0] == pr.KNOWN_ANSWERS[t], t
    P = pr.circomlib(3)
    first, m00 = "%064x" % P.rc[0][0], "%064x" % P.mds[0][0]
    assert first.startswith("0ee9a592") and first.endswith("cd8e6e") and m00.startswith("109b7f41")
    assert [[a for a in (3, 5, 7, 11, 13, 17) if pr.alpha_admissible(f, a)] for f in (0, 1, 2)] == [[5, 7, 11, 17], [11, 17], [5, 7, 17]]


def test_plan():
    lib = ffi.load()
    W = _per_workgroup()
    for width, heights in ((3, (1, 2, 8, 9, 10, 24, 28)), (4, (1, 5, 6, 17)), (5, (1, 4, 5, 10, 14))):
        a = width - 1
        for height in heights:
            rc, per, nodes, off, top, launches = _plan(lib, width, height)
            assert rc == 0 and per == W, (width, height)
            counts = [a ** (height - l) for l in range(1, height + 1)]
            assert nodes == sum(counts) == (a ** height - 1) // (a - 1)
            assert off == [sum(counts[:l]) for l in range(height)] and off[-1] == nodes - 1
            assert top == sum(c <= W for c in counts) >= 1 and launches == height - top + 1
    assert lib.panda_poseidon_plan(3, 4, None, None, None, None, None) == 0
    assert _plan(lib, 3, 24)[5] == 16, "a tree of 24 levels is not 24 launches"
    for width, height in ((2, 4), (1, 4), (0, 4), (6, 4), (3, 0), (3, 29), (4, 18), (5, 15), (3, 0xFFFFFFFF), (0xFFFFFFFF, 1)):
        per, nodes, top, launches = C.c_uint(0xDEAD), C.c_uint64(0xDEAD), C.c_uint(0xDEAD), C.c_uint(0xDEAD)
        off = (C.c_uint64 * 64)(*([0xDEAD] * 64))
        assert lib.panda_poseidon_plan(width, height, C.byref(per), C.byref(nodes), off, C.byref(top), C.byref(launches)) == 1, (width, height)
        assert (per.value, nodes.value, top.value, launches.value) == (0xDEAD,) * 4 and set(off) == {0xDEAD}, (width, height)


def test_bad_parameters_are_refused_before_any_device_call():
    """every refusal of create, and of the other calls on a handle that is not live, returns 1 -- also on a machine with no device -- and
    writes nothing"""
    lib = ffi.load()
    P = pr.random_params(0, 0x51001, 3, 5, 4, 2)
    count = [0]

    def refused(P=P, field=None, **change):
        rc, handle = _create(P, field, **change)
        count[0] += 1
        return rc == 1 and handle.handle == 0x7777

    assert refused(field=3) and refused(field=0xFFFFFFFF)
    assert lib.panda_poseidon_create(0, None, C.byref(ffi.PandaPoseidon())) == 1
    rc_w, mds_w = P.rc_wire(), P.mds_wire()
    good = ffi.PoseidonParams(3, 5, 4, 2, rc_w.ctypes.data, mds_w.ctypes.data)
    assert lib.panda_poseidon_create(0, C.byref(good), None) == 1
    for width in (0, 1, 6, 0xFFFFFFFF):
        assert refused(width=width), width
    for alpha in (0, 1, 2, 3, 4, 6, 9, 13, 19, 25):
        assert refused(alpha=alpha), alpha
    for field, alpha in ((1, 5), (1, 7), (2, 11)):  # alpha divides p - 1
        assert (fr.modulus(field) - 1) % alpha == 0
        assert refused(pr.random_params(field, 0x51002, 3, 17, 4, 2), alpha=alpha), (field, alpha)
    for rf in (0, 1, 3, 18, 17, 0xFFFFFFFE):
        assert refused(full_rounds=rf), rf
    assert refused(partial_rounds=129) and refused(partial_rounds=0xFFFFFFFF)
    assert refused(round_constants=None) and refused(mds=None)
    p = fr.modulus(0)
    for where in (0, 7, 17):  # a round constant >= the modulus
        for value in (p, fr.W - 1):
            bad = np.array(P.rc_wire())
            bad[where] = fr.words([value])[0]
            assert refused(round_constants=bad.ctypes.data), (where, value)
    for where in (0, 8):
        bad = np.array(P.mds_wire())
        bad[where] = fr.words([p])[0]
        assert refused(mds=bad.ctypes.data), where
    # the other calls on NULL and on a handle that was never created: host memory stands in for the buffers
    mem = np.full(1 << 16, 0x5A, np.uint8)
    a, b = mem.ctypes.data, mem.ctypes.data + (1 << 15)
    tag = fr.wire_one(0, 1)
    for handle in (ffi.PandaPoseidon(), ffi.PandaPoseidon(mem.ctypes.data + 64)):
        assert lib.panda_poseidon_permute(handle, a, b, 4, STREAM) == 1
        assert lib.panda_poseidon_hash(handle, a, 2, 2, 1, tag.ctypes.data, b, 4, STREAM) == 1
        assert lib.panda_poseidon_merkle_tree(handle, a, 2, tag.ctypes.data, b, None, STREAM) == 1
        assert lib.panda_poseidon_destroy(handle) == 1
    assert (mem == 0x5A).all() and count[0] > 35


def test_host_program_checks_the_bounds(tmp_path):
    """tests/host_check/poseidon_host.cpp: poseidon.h on the host under FE29_CHECK against 256-bit arithmetic of its own -- three fields,
    t = 2 and 5, every admissible alpha, constants and states at p - 1, 0 and 1, R_P = 0, R_F = 2 and the largest shape"""
    assert run_host_check(tmp_path, "poseidon_host.cpp") >= 1000


def _host_permute(tmp_path, P, states, name):
    path = tmp_path / (name + ".txt")
    vals = fr.ints(P.rc_wire()) + fr.ints(P.mds_wire()) + fr.ints(fr.wire(P.field, [v for s in states for v in s]))
    path.write_text("%d %d %d %d %d %d\n" % (P.field, P.t, P.alpha, P.rf, P.rp, len(states)) + "\n".join("%064x" % v for v in vals) + "\n")
    out = run_host_check(tmp_path, "poseidon_host.cpp", str(path))
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = [int(line, 16) for line in out.stdout.split()]
    return [got[k * P.t:(k + 1) * P.t] for k in range(len(states))]


def test_device_routine_on_the_host_equals_the_reference(tmp_path):
    """the routine the kernels run, compiled for the CPU, on circomlib's four sets (with their known answers) and on random sets of the
    other two fields"""
    cases = [("circomlib%d" % t, pr.circomlib(t)) for t in (2, 3, 4, 5)]
    cases += [("bls377_t4_a11", pr.random_params(1, 0x52001, 4, 11, 6, 5)), ("bls377_t2_a17", pr.random_params(1, 0x52002, 2, 17, 2, 0)),
              ("bls381_t5_a7", pr.random_params(2, 0x52003, 5, 7, 4, 11)), ("bls381_t3_a17", pr.random_params(2, 0x52004, 3, 17, 8, 1))]
    for name, P in cases:
        states = [list(range(P.t)), [0] * P.t, [P.p - 1] * P.t] + [fr.random_residues(P.field, 0x52100 + k, P.t) for k in range(3)]
        got = _host_permute(tmp_path, P, states, name)
        want = [fr.ints(fr.wire(P.field, pr.permute(P, s))) for s in states]
        assert got == want, name
        if name.startswith("circomlib"):
            assert fr.plain(0, fr.words(got[0][:1])) == [pr.KNOWN_ANSWERS[P.t]], name


# ------------------------------------------------------------------------------------------------- on the device
class Dev(GuardedBuffers):
    """a handle, guarded device buffers, and the calls over them"""

    def __init__(self, gm, P):
        super().__init__()
        self.lib, self.P, self.stream = ffi.load(), P, gm.exec_stream.raw
        rc, self.handle = _create(P)
        assert rc == 0 and self.handle.handle not in (None, 0, 0x7777)

    def elems(self, vals):
        return self.buffer(fr.wire(self.P.field, vals))

    def tag(self, v):
        return fr.wire_one(self.P.field, v)

    def permute(self, d_in, d_out, n, in_off=0, out_off=0):
        return self.lib.panda_poseidon_permute(self.handle, C.c_void_p(d_in.ptr.value + in_off), C.c_void_p(d_out.ptr.value + out_off), n, self.stream)

    def hash(self, d_in, length, msg_stride, elem_stride, tag, d_out, n, out_off=0):
        t = None if tag is None else C.c_void_p(tag.ctypes.data)
        return self.lib.panda_poseidon_hash(self.handle, d_in.ptr, length, msg_stride, elem_stride, t, C.c_void_p(d_out.ptr.value + out_off), n, self.stream)

    def tree(self, d_leaves, height, tag, d_nodes, root=None, nodes_off=0):
        t = None if tag is None else C.c_void_p(tag.ctypes.data)
        r = None if root is None else C.c_void_p(root.ctypes.data)
        return self.lib.panda_poseidon_merkle_tree(self.handle, d_leaves.ptr, height, t, C.c_void_p(d_nodes.ptr.value + nodes_off), r, self.stream)

    def drop(self):
        """free the buffers, keep the handle"""
        super().close()

    def close(self):
        if self.handle.handle:
            assert self.lib.panda_poseidon_destroy(self.handle) == 0
            self.handle = ffi.PandaPoseidon()
        super().close()


@functools.lru_cache(maxsize=None)
def _states(name):
    """3 W + 7 states of the set and their permutations, plain: 0 .. t - 1 (circomlib's known answer), all 0, all p - 1, mixed, random"""
    P = _set(name)
    n = 3 * _per_workgroup() + 7
    vals = fr.random_residues(P.field, 0x53000 + SETS.index(name), n * P.t)
    states = [vals[k * P.t:(k + 1) * P.t] for k in range(n)]
    states[0], states[1], states[2] = list(range(P.t)), [0] * P.t, [P.p - 1] * P.t
    states[3] = [(0, P.p - 1, 1)[j % 3] for j in range(P.t)]
    states[-1] = [P.p - 1] * P.t
    return states, [pr.permute(P, s) for s in states]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_permute(gm, name):
    P, W = _set(name), _per_workgroup()
    states, want = _states(name)
    if name.startswith("circomlib"):
        assert want[0][0] == pr.KNOWN_ANSWERS[P.t], "the device has circomlib's published hash to reproduce"
    flat = lambda rows: [v for s in rows for v in s]
    h = Dev(gm, P)
    try:
        for n in (1, 63, 64, 65, W, W + 1, 3 * W + 7):
            src, out = h.elems(flat(states[:n])), h.buffer(nbytes=n * P.t * 32)
            assert h.permute(src, out, n) == 0, n
            expect = fr.wire(P.field, flat(want[:n]))
            bad = np.nonzero((h.get(out).reshape(-1, 8) != expect).any(axis=1))[0]
            assert bad.size == 0, (name, n, "elements", bad[:8].tolist())
            assert h.intact(src) and h.intact(out), (name, n, "an input or a guard was written")
            assert h.permute(src, src, n) == 0, n  # in place
            assert np.array_equal(h.get(src).reshape(-1, 8), expect) and h.guard_intact(src), (name, n, "in place")
            h.drop()
    finally:
        h.close()


@functools.lru_cache(maxsize=None)
def _messages(name):
    """W + 1 messages of 2 (t - 1) + 1 elements, a tag, and for each len the reference's hashes of the messages' first len elements"""
    P = _set(name)
    n, longest = _per_workgroup() + 1, 2 * (P.t - 1) + 1
    vals = fr.random_residues(P.field, 0x54000 + SETS.index(name), n * longest)
    msgs = [vals[k * longest:(k + 1) * longest] for k in range(n)]
    msgs[0], msgs[1] = [P.p - 1] * longest, [0] * longest
    tag = 0x1234567 + (P.p >> 1)
    lens = sorted({1, P.t - 1, P.t, longest})
    return msgs, tag, {length: [pr.hash(P, m[:length], tag) for m in msgs] for length in lens}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("circomlib3", "circomlib2", "bls377"))
def test_hash_both_layouts(gm, name):
    P, W = _set(name), _per_workgroup()
    msgs, tag, want = _messages(name)
    assert set(want) == {1, P.t - 1, P.t, 2 * (P.t - 1) + 1}
    h = Dev(gm, P)
    try:
        for length, hashes in want.items():
            for n in (65, W + 1):
                rows = [m[:length] for m in msgs[:n]]
                contiguous = h.elems([v for m in rows for v in m])
                columns = h.elems([rows[i][j] for j in range(length) for i in range(n)])
                a, b = h.buffer(nbytes=n * 32), h.buffer(nbytes=n * 32)
                assert h.hash(contiguous, length, length, 1, h.tag(tag), a, n) == 0, (length, n)
                assert h.hash(columns, length, 1, n, h.tag(tag), b, n) == 0, (length, n)
                expect = fr.wire(P.field, hashes[:n])
                assert np.array_equal(h.get(a).reshape(-1, 8), expect), (name, length, n, "contiguous")
                assert np.array_equal(h.get(b), h.get(a)), (name, length, n, "the column layout gives other bytes")
                assert all(h.intact(d) for d in (contiguous, columns, a, b)), (name, length, n)
                h.drop()
        if name == "circomlib3":  # len <= t - 1 and tag 0 is circomlib's hash
            src, out = h.elems([1, 2]), h.buffer(nbytes=32)
            assert h.hash(src, 2, 2, 1, h.tag(0), out, 1) == 0
            assert fr.plain(0, h.get(out).reshape(-1, 8)) == [pr.KNOWN_ANSWERS[3]]
    finally:
        h.close()


@functools.lru_cache(maxsize=None)
def _tree(width):
    """(set, leaves, tag, reference levels) of the tallest tree of the arity: heights top + 2 (arity 2) and 5 (arity 4)"""
    P = _set("circomlib%d" % width)
    a = width - 1
    height = _top_levels(width) + 2 if width == 3 else 5
    leaves = fr.random_residues(0, 0x55000 + width, a ** height)
    leaves[0], leaves[1] = P.p - 1, 0
    tag = 0x7A6 + width
    return P, leaves, tag, pr.merkle_levels(P, leaves, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("width", (3, 5))
def test_merkle_tree(gm, width):
    """the tree over the first a^height leaves is the left corner of the tallest one: one reference for all heights"""
    P, leaves, tag, levels = _tree(width)
    a, top, W = width - 1, _top_levels(width), _per_workgroup()
    heights = (1, 2, top, top + 1, top + 2) if width == 3 else (1, 5)
    assert a ** (heights[-1] - 1) > W or width == 5, "the tallest tree has levels wider than a workgroup"
    h = Dev(gm, P)
    try:
        for height in heights:
            rc, _, n_nodes, offsets, _, launches = _plan(h.lib, width, height)
            assert rc == 0 and launches == max(height - top, 0) + 1
            src, nodes = h.elems(leaves[:a ** height]), h.buffer(nbytes=n_nodes * 32)
            root = np.full(8, 0xA5A5A5A5, np.uint32)
            assert h.tree(src, height, h.tag(tag), nodes, root) == 0, height
            got = h.get(nodes).reshape(-1, 8)
            below = src
            for l in range(1, height + 1):
                count = a ** (height - l)
                level = got[offsets[l - 1]:offsets[l - 1] + count]
                assert np.array_equal(level, fr.wire(0, levels[l - 1][:count])), (width, height, "level", l)
                # the level is panda_poseidon_hash over the level below: len = a, contiguous, the same tag
                again = h.buffer(nbytes=count * 32)
                assert h.hash(below, a, a, 1, h.tag(tag), again, count) == 0
                assert np.array_equal(h.get(again).reshape(-1, 8), level) and h.intact(again), (width, height, "hash of level", l - 1)
                below = h.buffer(level)
            assert np.array_equal(root, got[-1]) and fr.plain(0, root.reshape(1, 8)) == [levels[height - 1][0]], (width, height, "root")
            assert h.intact(src) and h.intact(nodes), (width, height)
            rootless = h.buffer(nbytes=n_nodes * 32)
            assert h.tree(src, height, h.tag(tag), rootless, None) == 0 and np.array_equal(h.get(rootless), h.get(nodes))
            h.drop()
    finally:
        h.close()


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(gm):
    P, W = _set("bls381"), _per_workgroup()
    t, p = P.t, P.p
    h, h2 = Dev(gm, P), Dev(gm, pr.random_params(0, 0x56001, 2, 5, 2, 1))
    try:
        n = 40
        src, out = h.elems(fr.random_residues(P.field, 0x56002, n * t)), h.buffer(nbytes=n * t * 32)
        good, over, big = h.tag(5), fr.words([p])[0].copy(), fr.words([fr.W - 1])[0].copy()
        # permute
        assert h.permute(src, out, 0) == 1 and h.permute(src, out, CAP + 1) == 1 and h.permute(src, out, 1 << 40) == 1
        assert h.lib.panda_poseidon_permute(h.handle, None, out.ptr, n, h.stream) == 1 and h.lib.panda_poseidon_permute(h.handle, src.ptr, None, n, h.stream) == 1
        assert h.permute(src, src, n - 1, out_off=32) == 1 and h.permute(src, src, n - 1, in_off=32) == 1, "a partial overlap"
        assert h.permute(src, out, n + 200) == 1, "buffers of the library's allocator that are too short"
        # hash: n messages of t elements in src
        assert h.hash(src, 0, t, 1, good, out, n) == 1 and h.hash(src, t, t, 1, good, out, 0) == 1
        assert h.hash(src, 1 << 14, 1, 1, good, out, (1 << 14) + 1) == 1, "n x len over the cap"
        assert h.hash(src, t, t, 1, None, out, n) == 1 and h.hash(src, t, t, 1, over, out, n) == 1 and h.hash(src, t, t, 1, big, out, n) == 1, "the tag"
        assert h.hash(src, t, CAP + 1, 1, good, out, n) == 1 and h.hash(src, t, t, CAP + 1, good, out, n) == 1, "the strides"
        assert h.hash(src, t, t, 1, good, src, n, out_off=32 * (n * t - 1)) == 1 and h.hash(src, t, t, 1, good, src, 1) == 1, "d_out inside the input extent"
        assert h.hash(src, t, t + 300, 1, good, out, n) == 1 and h.hash(src, t, 1, n + 300, good, out, n) == 1, "an input extent beyond the buffer"
        assert h.hash(src, 1, 1, 1, good, out, n * t + 200) == 1, "d_out too short"
        assert h.lib.panda_poseidon_hash(h.handle, None, t, t, 1, C.c_void_p(good.ctypes.data), out.ptr, n, h.stream) == 1
        assert h.lib.panda_poseidon_hash(h.handle, src.ptr, t, t, 1, C.c_void_p(good.ctypes.data), None, n, h.stream) == 1
        # the tree: 32 leaves of arity 2 in src, 31 nodes
        root = np.full(8, 0xA5A5A5A5, np.uint32)
        assert h.tree(src, 0, good, out, root) == 1 and h.tree(src, 29, good, out, root) == 1 and h.tree(src, 0xFFFFFFFF, good, out, root) == 1
        assert h.tree(src, 5, None, out, root) == 1 and h.tree(src, 5, over, out, root) == 1, "the tag"
        assert h.tree(src, 5, good, src, root, nodes_off=32 * 31) == 1 and h.tree(src, 5, good, src, root) == 1, "d_nodes overlaps d_leaves"
        assert h.tree(src, 12, good, out, root) == 1, "leaves and nodes too short"
        assert h.lib.panda_poseidon_merkle_tree(h.handle, None, 5, C.c_void_p(good.ctypes.data), out.ptr, None, h.stream) == 1
        assert h.lib.panda_poseidon_merkle_tree(h.handle, src.ptr, 5, C.c_void_p(good.ctypes.data), None, None, h.stream) == 1
        assert h2.tree(src, 5, h2.tag(5), out, root) == 1, "width 2 has no tree"
        # a destroyed handle
        dead = ffi.PandaPoseidon(h2.handle.handle)
        h2.close()
        assert h.lib.panda_poseidon_permute(dead, src.ptr, out.ptr, n, h.stream) == 1 and h.lib.panda_poseidon_destroy(dead) == 1
        assert h.lib.panda_poseidon_hash(dead, src.ptr, 1, 1, 1, C.c_void_p(good.ctypes.data), out.ptr, n, h.stream) == 1
        assert h.untouched(out) and h.intact(src) and (root == 0xA5A5A5A5).all(), "a refused call wrote"
        # and the same buffers serve a valid call
        assert h.permute(src, out, n) == 0 and not h.untouched(out) and h.intact(out)
    finally:
        h.close()
        h2.close()


@pytest.mark.gpu
def test_two_handles_and_the_table_goes_back(gm):
    lib = ffi.load()
    P1, P2 = _set("circomlib3"), pr.random_params(0, 0x57001, 3, 7, 4, 5)
    states = _states("circomlib3")[0][:70]
    flat = [v for s in states for v in s]
    h1 = Dev(gm, P1)
    try:
        src, a, b, c = h1.elems(flat), h1.buffer(nbytes=70 * 3 * 32), h1.buffer(nbytes=70 * 3 * 32), h1.buffer(nbytes=70 * 3 * 32)
        assert h1.permute(src, a, 70) == 0
        h2 = Dev(gm, P2)
        try:
            assert lib.panda_poseidon_permute(h2.handle, src.ptr, b.ptr, 70, h1.stream) == 0
            assert np.array_equal(h1.get(b).reshape(-1, 8), fr.wire(0, [v for s in states for v in pr.permute(P2, s)])), "the second handle's parameters"
            assert h1.permute(src, c, 70) == 0 and np.array_equal(h1.get(c), h1.get(a)), "a second handle disturbed the first"
        finally:
            h2.close()
        h1.fill(c)
        assert h1.permute(src, c, 70) == 0 and np.array_equal(h1.get(c), h1.get(a)), "destroying the second handle disturbed the first"
        assert np.array_equal(h1.get(a).reshape(-1, 8), fr.wire(0, [v for s in _states("circomlib3")[1][:70] for v in s]))
        assert all(h1.intact(d) for d in (src, a, b, c))
        # create + destroy gives the table back
        rc, warm = _create(P2)
        assert rc == 0 and lib.panda_poseidon_destroy(warm) == 0
        before = free_bytes(lib)
        rc, again = _create(P2)
        assert rc == 0 and lib.panda_poseidon_destroy(again) == 0
        assert free_bytes(lib) == before
        assert lib.panda_poseidon_destroy(again) == 1, "destroyed twice"
    finally:
        h1.close()


@pytest.mark.gpu
def test_python_wrapper(gm):
    P = _set("circomlib3")
    states, want = _states("circomlib3")
    psd = pgm.PandaPoseidon(gm, P.rc_wire().reshape(-1, 3, 8), P.mds_wire().reshape(3, 3, 8), P.alpha, P.rf, P.rp)
    try:
        assert psd.width == 3 and psd.per_workgroup == _per_workgroup()
        got = psd.permute(np.array(fr.wire(0, [v for s in states[:9] for v in s])).reshape(9, 3, 8))
        assert np.array_equal(got.reshape(-1, 8), fr.wire(0, [v for s in want[:9] for v in s]))
        msgs = np.array(fr.wire(0, [v for s in states[:9] for v in s])).reshape(9, 3, 8)
        rows = psd.hash(msgs, tag=fr.wire_one(0, 11))
        assert np.array_equal(rows, fr.wire(0, [pr.hash(P, s, 11) for s in states[:9]]))
        assert np.array_equal(psd.hash_columns(np.ascontiguousarray(msgs.transpose(1, 0, 2)), tag=fr.wire_one(0, 11)), rows)
        leaves = [s[0] for s in states[:8]]
        nodes, root = psd.merkle_tree(fr.wire(0, leaves))
        levels = pr.merkle_levels(P, leaves)
        assert np.array_equal(nodes, fr.wire(0, [v for level in levels for v in level])) and np.array_equal(root, nodes[-1])
        with pytest.raises(pgm.PandaGpuError):
            psd.merkle_tree(fr.wire(0, leaves[:6]))
    finally:
        psd.close()
    with pytest.raises(pgm.PandaGpuError):
        psd.permute(np.zeros((1, 3, 8), np.uint32))
