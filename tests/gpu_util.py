"""Small helpers for the tests: device buffers through the C ABI's own panda_malloc/panda_memcpy, plain and guarded, the device fixture,
and the checks every feature's test module makes of its exports and of its host-check program."""
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
