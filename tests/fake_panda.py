"""A stand-in for the object gpu_ffi.load() returns, for tests of panda_amd/gpu_manager.py that need neither a GPU nor the built library.

Every attribute is a callable that records its name and arguments and returns 0.  The allocation and create calls write a fresh fake
address or handle through their byref argument (panda_malloc_host hands out real host memory, because the wrappers memmove into pinned
buffers and read them back); the release calls take their argument out of the live set, and releasing what is not live is an error of
the test.  `fail_at = k` makes the k-th non-release call return 1, `fail_release = j` the j-th release call; a failed call does nothing
else.  Arguments are recorded by meaning, not by value: a stream by its label, a pointer as the allocation it lies in plus an offset
("d1+256"), any other address as "host", a structure field by field."""
import bisect
import ctypes as C

from panda_amd import gpu_ffi as ffi

RELEASES = ("panda_free", "panda_free_host", "panda_event_destroy", "panda_stream_destroy", "panda_mem_pool_destroy")
_DEVICE_BASE = 0x0D00000000000000  # above every address the host hands out
_HANDLE_BASE = 0x0E00000000000000


def _key(a):
    return a.handle if isinstance(a, C.Structure) else getattr(a, "value", a)


class FakePanda:
    def __init__(self):
        self.live = {}  # address or handle -> name, of everything allocated or created and not yet released
        self.streams = {}  # stream handle -> label, set by the test from the manager's four streams
        self.calls, self.releases = [], []  # what begin() started to record: [name, argument, ...] per call
        self.fail_at = self.fail_release = None
        self._names = {}  # handle -> name, kept after the release
        self._extents = []  # sorted (start, end, name) of the allocations; a pinned one leaves with its release, its address may come back
        self._pinned = {}
        self._count = {}
        self._prefix = "pre_"
        self._next_device, self._next_handle = _DEVICE_BASE, _HANDLE_BASE

    def begin(self, fail_at=None, fail_release=None):
        """start of the call under test: record from here, name what it allocates d0, h0, e0, ... and fail where asked"""
        self.calls, self.releases, self._count, self._prefix = [], [], {}, ""
        self.fail_at, self.fail_release = fail_at, fail_release

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        record = [name] + [self._describe(a) for a in args]
        if name in RELEASES:
            self.releases.append(record)
            if len(self.releases) == self.fail_release:
                return 1
            key = _key(args[0])
            if key is None:  # a null pointer: nothing to release, as in the library
                return 0
            assert key in self.live, f"{name}({record[1]}): not live"
            del self.live[key]
            if self._pinned.pop(key, None) is not None:
                self._extents = [e for e in self._extents if e[0] != key]
            return 0
        self.calls.append(record)
        if len(self.calls) == self.fail_at:
            return 1
        effect = getattr(self, "_do_" + name, None)
        if effect is not None:
            effect(*args)
        return 0

    # ------------------------------------------------------------------ the calls that write through an argument

    def _name(self, letter):
        k = self._count.get(letter, 0)
        self._count[letter] = k + 1
        return f"{self._prefix}{letter}{k}"

    def _extent(self, start, nbytes, letter):
        self.live[start] = name = self._name(letter)
        bisect.insort(self._extents, (start, start + max(nbytes, 1), name))
        return start

    def _handle(self, letter):
        self._next_handle += 16
        self.live[self._next_handle] = self._names[self._next_handle] = self._name(letter)
        return self._next_handle

    def _do_panda_malloc(self, ref, nbytes, *_):
        ref._obj.value = self._extent(self._next_device, nbytes, "d")
        self._next_device += (max(nbytes, 1) + 255) & ~255

    _do_panda_malloc_from_pool_async = _do_panda_malloc

    def _do_panda_malloc_host(self, ref, nbytes):
        buf = (C.c_uint8 * max(nbytes, 1))()
        self._pinned[C.addressof(buf)] = buf
        ref._obj.value = self._extent(C.addressof(buf), nbytes, "h")

    def _do_panda_stream_create(self, ref, *_):
        ref._obj.handle = self._handle("s")

    def _do_panda_event_create(self, ref, *_):
        ref._obj.handle = self._handle("e")

    def _do_panda_mem_pool_create(self, ref, *_):
        ref._obj.handle = self._handle("pool")

    def _do_panda_get_device_number(self, ref):
        ref._obj.value = 1

    # ------------------------------------------------------------------ arguments, by meaning

    def _where(self, v):
        i = bisect.bisect_right(self._extents, (v, float("inf"), "")) - 1
        if i >= 0 and self._extents[i][0] <= v < self._extents[i][1]:
            start, _, name = self._extents[i]
            return name if v == start else f"{name}+{v - start}"
        return "host" if v >= 1 << 32 else v

    def _describe(self, a):
        if a is None or isinstance(a, (bool, str)):
            return a
        if isinstance(a, int):
            return self._where(a)
        if isinstance(a, (ffi.PandaStream, ffi.PandaEvent, ffi.PandaMemPool)):
            return self.streams.get(a.handle) or self._names.get(a.handle, "null")
        if isinstance(a, C.Structure):
            return {f[0]: self._describe(getattr(a, f[0])) for f in a._fields_}
        if isinstance(a, C.Array):
            return [self._describe(x) for x in a]
        if isinstance(a, C._Pointer):
            return "pointer" if a else None
        if isinstance(a, C._SimpleCData):
            return self._describe(a.value)
        if hasattr(a, "_obj"):  # byref(...)
            return "&"
        raise TypeError(f"argument of a type the fake does not know: {a!r}")
