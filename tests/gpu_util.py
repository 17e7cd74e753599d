"""Small helpers for the tests: device buffers through the C ABI's own panda_malloc/panda_memcpy, plain and guarded, the device fixture,
the checks every feature's test module makes of its exports and of its host-check program, and the protocol that runs a call on scratch
filled through panda_debug_scratch_fill (independent_of_scratch)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from panda_amd import gpu_ffi as ffi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def has_gpu() -> bool:
    try:
        n = C.c_int(0)
        return ffi.load().panda_get_device_number(C.byref(n)) == 0 and n.value > 0
    except Exception:
        return False


class DeviceBuffer:
    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = C.c_void_p()
        ffi.check(ffi.load().panda_malloc(C.byref(self.ptr), max(self.nbytes, 16)), "CreateContextError")

    @classmethod
    def from_host(cls, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        buf = cls(a.nbytes)
        ffi.check(ffi.load().panda_memcpy(buf.ptr, C.c_void_p(a.ctypes.data), a.nbytes), "CreateContextError")
        return buf

    def to_host(self, dtype=np.uint32, nbytes=None, offset=0) -> np.ndarray:
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        ffi.check(ffi.load().panda_memcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.ptr.value + offset), nbytes), "CreateContextError")
        return out

    def free(self):
        if self.ptr:
            ffi.load().panda_free(self.ptr)
            self.ptr = C.c_void_p()


NULL_STREAM = ffi.PandaStream()
GUARD, GUARD_BYTES = 0xA5, 4096


class GuardedBuffers:
    """Device buffers with a run of GUARD_BYTES guard bytes behind the data, which no call may touch.  A buffer is a DeviceBuffer `d`
    with d.data_bytes, the length of its data, and d.host, the array uploaded into it (None for an output).  The harness of a test
    module derives from this class and adds the calls it makes over the buffers."""

    def __init__(self):
        self.bufs = []

    def buffer(self, x=None, nbytes=None):
        """a buffer that holds the array x, or nbytes of the guard byte where an output will go"""
        d = DeviceBuffer((nbytes if x is None else np.ascontiguousarray(x, np.uint32).nbytes) + GUARD_BYTES)
        self.bufs.append(d)
        self.fill(d, x, nbytes)
        return d

    def fill(self, d, x=None, nbytes=None):
        """back to the state of a new buffer: the guard byte throughout, then x uploaded and remembered; without x, nbytes (by default as
        many as before) of the guard byte stand for the data"""
        d.host = None if x is None else np.ascontiguousarray(x, np.uint32)
        d.data_bytes = d.host.nbytes if x is not None else d.data_bytes if nbytes is None else nbytes
        assert d.data_bytes + GUARD_BYTES <= d.nbytes
        ffi.check(ffi.load().panda_memset(d.ptr, GUARD, d.nbytes), "memset")
        if d.host is not None and d.data_bytes:
            ffi.check(ffi.load().panda_memcpy(d.ptr, C.c_void_p(d.host.ctypes.data), d.data_bytes), "memcpy")

    def get(self, d):
        """the data, as flat uint32"""
        return d.to_host(np.uint32, nbytes=d.data_bytes) if d.data_bytes else np.zeros(0, np.uint32)

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


@pytest.fixture(scope="module")
def gm():
    from panda_amd import gpu_manager as pgm
    m = pgm.PandaGpuManager(0)
    yield m
    m.deinit()


def free_bytes(lib):
    free, total = C.c_size_t(0), C.c_size_t(0)
    ffi.check(lib.panda_mem_get_info(C.byref(free), C.byref(total)), "mem_info")
    return free.value


# ------------------------------------------------------------------------------------------------- what a call finds in its scratch
# panda_debug_scratch_fill's patterns: every byte 0x00, every byte 0xFF, word i = scratch_hash(i ^ seed).  Both constants are needed: a
# block that must start as zeros and its neighbour that must start as all-ones each meet what they expect under one of the two.
SCRATCH_PATTERNS = ((0, 0x00), (0, 0xFF), (1, 0x5CA7C4ED))


def scratch_hash(x):
    """the header's h(x) of panda_debug_scratch_fill, mode 1, on Python integers"""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = x * 0x7FEB352D & 0xFFFFFFFF
    x ^= x >> 15
    x = x * 0x846CA68B & 0xFFFFFFFF
    return x ^ (x >> 16)


def scratch_pattern_bytes(mode, value, first_word, words):
    """what a fill leaves in `words` 32-bit words from word `first_word` of the arena, as uint8"""
    if mode == 0:
        return np.full(4 * words, value & 0xFF, np.uint8)
    return np.array([scratch_hash((first_word + i) ^ value) for i in range(words)], np.uint32).view(np.uint8)


def scratch_fill(mode, value):
    """fill the calling thread's scratch arena and mailbox -> (base, capacity) of the arena, (None, 0) without one"""
    base, capacity = C.c_void_p(0xDEAD), C.c_size_t(0xDEAD)
    ffi.check(ffi.load().panda_debug_scratch_fill(mode, value, C.byref(base), C.byref(capacity)), "scratch_fill")
    return base.value, capacity.value


def same_bytes(a, b):
    """two outputs of a call -- arrays, numbers, bytes or tuples / lists of them -- are identical byte for byte"""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_bytes(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b


def independent_of_scratch(call, check, exact, arena=True):
    """The output of call() does not depend on what its scratch held.  call() runs once, which grows the arena to what the call needs, and
    check(output) compares that output with the reference; then, for every pattern of SCRATCH_PATTERNS, the whole arena and the mailbox are
    filled, call() runs again on them, and its output is checked again -- and, where `exact` (the call documents a deterministic or
    canonical output), must be the first run's byte for byte.  The arena's (base, capacity) read with each fill must be what the fill
    behind the call reads: the call ran on the filled memory, not on a fresh allocation.  arena=False: the call takes no scratch of the
    arena (the fills then only have to leave its output alone).  Returns the first output."""
    first = call()
    check(first)
    fills = list(SCRATCH_PATTERNS) + [SCRATCH_PATTERNS[0]]
    where = scratch_fill(*fills[0])
    for k, pattern in enumerate(SCRATCH_PATTERNS):
        assert not arena or (where[0] and where[1] > 0), "the call left no scratch arena to fill"
        out = call()
        after = scratch_fill(*fills[k + 1])
        assert after == where, ("the call did not run on the filled arena", pattern, where, after)
        check(out)
        assert not exact or same_bytes(out, first), ("the output depends on what the scratch held", pattern)
    return first


def run_host_check(tmp_path, source, *args):
    """compile tests/host_check/<source> and run it -> the N of its `ok N` line; with arguments -> the completed process of that run.
    The program is built once per tmp_path."""
    exe = str(tmp_path / source[:-len(".cpp")])
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "host_check", source)], check=True)
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    if args:
        return out
    assert out.returncode == 0, out.stderr[-2000:]
    assert re.fullmatch(r"ok (\d+)\n", out.stdout), out.stdout[-2000:]
    return int(out.stdout.split()[1])


def assert_exported(names):
    """every name is declared in the header, listed as an additive symbol, exported by the library and given its argument types ->
    (the header's text, the loaded library)"""
    header = open(os.path.join(ROOT, "include", "panda_interface.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = ffi.load()
    for name in names:
        assert re.search(r"panda_error\s+%s\s*\(" % name, header)
        assert name in ffi.ADDITIVE_SYMBOLS and name in ffi.ALL_SYMBOLS
        assert re.search(r"\sT\s+%s$" % name, exported, re.M)
        assert getattr(lib, name).argtypes is not None
    return header, lib
