"""Host-side mirror of the reference's Rust `gpu_manager` (src/gpu_manager/wrapper.rs, unit.rs, common.rs).

Same names, argument meaning and staging protocol as the Rust layer, over the same C ABI:
`PandaGpuManager` owns the device id, the memory pool and the four streams
(wrapper.rs:8-19, 31-53); `panda_msm_bn254_gpu*` / `panda_ntt_bn254_gpu*` stage byte slices to the
device, fill the by-value configuration struct, call the library and copy the answer back
(unit.rs:10-101, 103-188, 190-361, 363-416, 418-543).  Byte slices are numpy uint8/uint32 arrays.

Differences, all deliberate:
  * errors raise PandaGpuError instead of returning Err / unwrapping;
  * every buffer and event a call takes is released on every way out (`_Buffers`; the reference leaks the pinned result buffer,
    unit.rs:67-100, and whatever was staged when a later step fails);
  * cached scalars survive reuse, because the library no longer de-Montgomeryizes in place.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import gpu_ffi as ffi
from .gpu_ffi import JACOBIAN, PROJECTIVE, PandaGpuError  # noqa: F401

FIELD_ELEMENT_LEN = 32  # gpu_manager/mod.rs:14
BN254, BLS12_377, BLS12_381, BN254_G2, BLS12_381_G2, BLS12_377_G2 = 0, 1, 2, 3, 4, 6  # id 5 is unused
_POINT_BYTES = {BN254: 64, BLS12_377: 96, BLS12_381: 96, BN254_G2: 128, BLS12_381_G2: 192, BLS12_377_G2: 192}
_RESULT_BYTES = {BN254: 96, BLS12_377: 144, BLS12_381: 144, BN254_G2: 192, BLS12_381_G2: 288, BLS12_377_G2: 288}


def _msm_entry(lib, curve: int, host: bool = False):
    names = {BN254: "bn254", BLS12_377: "bls12_377", BLS12_381: "bls12_381", BN254_G2: "bn254_g2", BLS12_381_G2: "bls12_381_g2",
             BLS12_377_G2: "bls12_377_g2"}
    return getattr(lib, f"panda_msm_execute_{names[curve]}" + ("_host" if host else ""))


def log_2(num: int) -> int:  # gpu_manager/common.rs:5-15
    assert num > 0
    return num.bit_length() - 1


def _as_bytes(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


class PandaStreamHandle:
    """PandaStream::new/sync/wait/destroy (gpu_ffi/common.rs:46-87)."""

    def __init__(self):
        self.raw = ffi.PandaStream()
        ffi.check(ffi.load().panda_stream_create(C.byref(self.raw), True), "StremCreateErr")

    def sync(self):
        ffi.check(ffi.load().panda_stream_synchronize(self.raw), "StreamSyncErr")

    def wait(self, event: "PandaEventHandle"):
        ffi.check(ffi.load().panda_stream_wait_event(self.raw, event.raw), "StreamWaitEventErr")

    def destroy(self):
        ffi.check(ffi.load().panda_stream_destroy(self.raw), "StreamDestroyErr")


class PandaEventHandle:
    """PandaEvent::new/record/sync/destroy (gpu_ffi/common.rs:95-132)."""

    def __init__(self):
        self.raw = ffi.PandaEvent()
        ffi.check(ffi.load().panda_event_create(C.byref(self.raw), True, True), "EventCreateErr")

    def record(self, stream: PandaStreamHandle):
        ffi.check(ffi.load().panda_event_record(self.raw, stream.raw), "EventRecordErr")

    def sync(self):
        ffi.check(ffi.load().panda_event_sync(self.raw), "EventSyncErr")

    def destroy(self):
        ffi.check(ffi.load().panda_event_destroy(self.raw), "EventDestroyErr")


def get_device_number() -> int:  # wrapper.rs:315-323
    n = C.c_int(0)
    ffi.check(ffi.load().panda_get_device_number(C.byref(n)), "GetDeviceCountError")
    return n.value


def set_device(device_id: int) -> None:  # wrapper.rs:340-347
    ffi.check(ffi.load().panda_set_device(device_id), "SetDeviceError")


def device_info(device_id: int) -> dict:  # wrapper.rs:325-338
    set_device(device_id)
    free, total = C.c_size_t(0), C.c_size_t(0)
    ffi.check(ffi.load().panda_mem_get_info(C.byref(free), C.byref(total)), "DeviceGetDeviceMemoryInfoError")
    return {"free": free.value, "total": total.value}


class PandaGpuManager:
    def __init__(self, device_id: int = 0):  # PandaGpuManager::new, wrapper.rs:32-53
        if get_device_number() == 0:
            raise PandaGpuError("GetDeviceCountError")
        self.device_id = device_id
        self.mem_pool = self.init_hardware(device_id)
        self.default_stream = PandaStreamHandle()
        self.h2d_stream = PandaStreamHandle()
        self.d2h_stream = PandaStreamHandle()
        self.exec_stream = PandaStreamHandle()
        self.d_bases: list[int] = []
        self.d_scalars: list[int] = []
        self.scalars_len: list[int] = []
        self.msm_result_coordinate_type = JACOBIAN
        self._bases_bytes: dict[int, int] = {}
        self._registered: list[int] = []

    def add_cached_bases(self, bases) -> int:
        """init_msm_cached_bases + push onto d_bases (what callers of the reference do by hand); returns the index."""
        self.d_bases.append(self.init_msm_cached_bases(bases))
        self._bases_bytes[len(self.d_bases) - 1] = _as_bytes(bases).size
        return len(self.d_bases) - 1

    @classmethod
    def init_all(cls, device_id, bases=None, omega=None):  # wrapper.rs:55-113
        gm = cls(device_id)
        if bases is not None:
            gm.d_bases = cls.init_msm(bases)
        if omega is not None:
            cls.init_ntt(omega)
        if bases is None and omega is None:
            raise PandaGpuError("MSMBasesAddrError")
        return gm

    @staticmethod
    def init_hardware(device_id: int) -> ffi.PandaMemPool:  # wrapper.rs:115-120
        set_device(device_id)
        pool = ffi.PandaMemPool()
        ffi.check(ffi.load().panda_mem_pool_create(C.byref(pool), device_id), "MemPoolCreateErr")
        return pool

    @staticmethod
    def init_msm_cached_bases(bases) -> int:  # wrapper.rs:154-169
        with _Buffers() as b:
            return b.keep(b.upload_sync(bases)).value

    init_msm_cached_scalars = init_msm_cached_bases  # wrapper.rs:171-186: same staging

    def register_cached_bases(self, index: int, curve: int = 0) -> None:
        """Additive: let the library keep the radix-converted copy of cached base set `index` between calls
        (panda_msm_register_bases).  The buffer must stay unmodified until deinit()."""
        d = self.get_params_bases_ptr_mut(index)
        if d is None:
            raise PandaGpuError("BasesIndexErr")
        nbytes = self._bases_bytes[index]
        log_n = log_2(nbytes // _POINT_BYTES[curve])
        ffi.check(ffi.load().panda_msm_register_bases(curve, C.c_void_p(d), log_n, self.exec_stream.raw), "CreateContextError")
        self._registered.append(d)

    def precompute_cached_bases(self, index: int, curve: int = 0, window_bits: int = 0) -> tuple[int, int, int]:
        """Additive: register cached base set `index` together with its window tables (panda_msm_precompute_bases).
        Returns (tables, window_bits, device bytes held)."""
        d = self.get_params_bases_ptr_mut(index)
        if d is None:
            raise PandaGpuError("BasesIndexErr")
        nbytes = self._bases_bytes[index]
        log_n = log_2(nbytes // _POINT_BYTES[curve])
        lib = ffi.load()
        ffi.check(lib.panda_msm_precompute_bases(curve, C.c_void_p(d), log_n, window_bits, self.exec_stream.raw), "CreateContextError")
        self._registered.append(d)
        tables, bits, held = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
        ffi.check(lib.panda_msm_registered_info(C.c_void_p(d), C.byref(tables), C.byref(bits), C.byref(held)), "CreateContextError")
        return tables.value, bits.value, held.value

    @classmethod
    def init_msm(cls, bases_list) -> list[int]:  # wrapper.rs:122-152
        ptrs = [cls.init_msm_cached_bases(b) for b in bases_list]
        ffi.check(ffi.load().panda_msm_setup_bn254(), "CreateContextError")
        return ptrs

    @staticmethod
    def init_ntt(omega) -> None:  # wrapper.rs:199-210
        o = _as_bytes(omega)
        ffi.check(ffi.load().panda_ntt_setup_bn254(_ptr(o)), "CreateContextError")

    def set_config(self, coordinate_type: int):  # wrapper.rs:212-214
        self.msm_result_coordinate_type = coordinate_type

    def get_params_bases_ptr_mut(self, index: int):  # wrapper.rs:240-245
        return self.d_bases[index] if 0 <= index < len(self.d_bases) else None

    def get_params_scalars_ptr_mut(self, index: int):
        return self.d_scalars[index] if 0 <= index < len(self.d_scalars) else None

    def get_params_scalars_len(self, index: int) -> int:
        return self.scalars_len[index] if 0 <= index < len(self.scalars_len) else 0

    def wait_h2d(self):  # wrapper.rs:260-266
        with _Buffers(self) as b:
            b.wait_h2d()

    def sync(self):  # wrapper.rs:285-291
        self.h2d_stream.sync()
        self.exec_stream.sync()
        self.d2h_stream.sync()

    def deinit(self):  # wrapper.rs:297-312
        lib = ffi.load()
        for d in self._registered:
            lib.panda_msm_unregister_bases(C.c_void_p(d))  # "not registered" (the caller already undid it) is not an error here
        self._registered = []
        for d in self.d_bases + self.d_scalars:
            ffi.check(lib.panda_free(C.c_void_p(d)), "DestroyContextErr")
        self.d_bases, self.d_scalars, self.scalars_len = [], [], []
        ffi.check(lib.panda_msm_tear_down(), "DestroyContextErr")
        ffi.check(lib.panda_mem_pool_destroy(self.mem_pool), "DestroyContextErr")
        for s in (self.default_stream, self.h2d_stream, self.d2h_stream, self.exec_stream):
            s.destroy()


# ---------------------------------------------------------------------------- gpu_manager/common.rs

def _vp(d) -> C.c_void_p:
    return d if isinstance(d, C.c_void_p) else C.c_void_p(d)


class _Buffers:
    """What one call takes from the library -- device, pool and pinned buffers, events -- released on every way out: in reverse order,
    each release attempted whatever the others return, an exception already on its way never replaced; a release that fails on an
    otherwise clean exit raises CreateContextError.  The only place in this file that allocates or frees (deinit, PandaSparseMatrix.free,
    PandaKzgOpenAll.close and PandaPoseidon.close release what keep() handed over).  tests/test_gpu_manager_buffers.py runs every wrapper over it."""

    def __init__(self, gm: "PandaGpuManager | None" = None):
        self.gm, self.lib, self._owned = gm, ffi.load(), []

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        codes = [release(handle) for release, handle in reversed(self._owned)]
        self._owned = []
        if exc_type is None and any(codes):
            raise PandaGpuError("CreateContextError")

    def _own(self, release, handle):
        self._owned.append((release, handle))
        return handle

    def keep(self, d):
        """hand `d` over to an owner that outlives the call: the scope no longer releases it"""
        self._owned = [(release, handle) for release, handle in self._owned if handle is not d]
        return d

    def device(self, nbytes: int, kind: str = "AsyncPoolMallocErr") -> C.c_void_p:
        d = C.c_void_p()
        ffi.check(self.lib.panda_malloc(C.byref(d), nbytes), kind)
        return self._own(self.lib.panda_free, d)

    def pool(self, nbytes: int, stream: PandaStreamHandle) -> C.c_void_p:
        d = C.c_void_p()
        ffi.check(self.lib.panda_malloc_from_pool_async(C.byref(d), nbytes, self.gm.mem_pool, stream.raw), "AsyncPoolMallocErr")
        return self._own(self.lib.panda_free, d)

    def pinned(self, nbytes: int) -> C.c_void_p:
        h = C.c_void_p()
        ffi.check(self.lib.panda_malloc_host(C.byref(h), nbytes), "CreateContextError")
        return self._own(self.lib.panda_free_host, h)

    def event(self) -> PandaEventHandle:
        ev = PandaEventHandle()
        self._own(self.lib.panda_event_destroy, ev.raw)
        return ev

    def wait_h2d(self):  # wrapper.rs:260-266
        ev = self.event()
        ev.record(self.gm.h2d_stream)
        self.gm.exec_stream.wait(ev)

    def send(self, d, a: np.ndarray, offset: int = 0):
        """host array -> d + offset, asynchronously on the h2d stream; returns d"""
        ffi.check(self.lib.panda_memcpy_async(C.c_void_p(d.value + offset), _ptr(a), a.nbytes, self.gm.h2d_stream.raw), "AsyncMemcopyErr")
        return d

    def fill(self, d, bufs):
        """equal-length host arrays -> d, member after member, and the exec stream waits for the copies; returns d"""
        for k, a in enumerate(bufs):
            self.send(d, a, k * a.nbytes)
        self.wait_h2d()
        return d

    def upload(self, arrays):
        """equal-length arrays of field elements -> (one device buffer holding them member after member, batch, n)"""
        bufs = [_as_bytes(a) for a in arrays]
        size = bufs[0].size
        if size == 0 or size % FIELD_ELEMENT_LEN or any(a.size != size for a in bufs):
            raise PandaGpuError("SchedulingErr")
        return self.fill(self.device(len(bufs) * size), bufs), len(bufs), size // FIELD_ELEMENT_LEN

    def upload_sync(self, a) -> C.c_void_p:
        """one array -> a device buffer of its own, synchronously"""
        a = _as_bytes(a)
        d = self.device(a.size, "CreateContextError")
        ffi.check(self.lib.panda_memcpy(d, _ptr(a), a.size), "CreateContextError")
        return d

    def upload_pool(self, a, stream: PandaStreamHandle) -> C.c_void_p:  # common.rs:54-65
        """one array -> a pool allocation, asynchronously on `stream`"""
        a = _as_bytes(a)
        d = self.pool(a.size, stream)
        ffi.check(self.lib.panda_memcpy_async(d, _ptr(a), a.size, stream.raw), "AsyncMemcopyErr")
        return d

    def read(self, out: np.ndarray, d) -> np.ndarray:
        """device -> the host array `out`, synchronously; returns out"""
        ffi.check(self.lib.panda_memcpy(_ptr(out), _vp(d), out.nbytes), "CreateContextError")
        return out

    def download(self, d, nbytes: int) -> np.ndarray:
        return self.read(np.empty(nbytes, np.uint8), d)

    def download_vectors(self, d, batch: int, n: int) -> list:
        """the `batch` vectors of n elements at d -> a list of (n, 8) uint32 arrays"""
        size = n * FIELD_ELEMENT_LEN
        return [self.download(d.value + k * size, size).view(np.uint32).reshape(-1, 8) for k in range(batch)]


def memory_alloc_and_copy(gm: PandaGpuManager, h_values, stream: PandaStreamHandle) -> int:  # common.rs:54-65; the caller frees
    with _Buffers(gm) as b:
        return b.keep(b.upload_pool(h_values, stream)).value


# ---------------------------------------------------------------------------- gpu_manager/unit.rs

def _msm_device(b: _Buffers, d_scalars, d_bases, log_n, curve):
    """the run and the copy back that the four MSM calls share; what the caller staged in `b` goes back with the rest at its exit"""
    gm, lib = b.gm, b.lib
    nres = _RESULT_BYTES[curve]
    d_result = b.pool(nres, gm.h2d_stream)
    b.wait_h2d()
    cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, d_bases, d_scalars, d_result, log_n, gm.msm_result_coordinate_type)
    ffi.check(_msm_entry(lib, curve)(cfg), "SchedulingErr")
    ev = b.event()
    ev.record(gm.exec_stream)
    ev.sync()
    host = b.pinned(nres)
    ffi.check(lib.panda_memcpy(host, d_result, nres), "CreateContextError")
    return np.frombuffer((C.c_uint8 * nres).from_address(host.value), dtype=np.uint8).copy()


def panda_msm_bn254_gpu(gm: PandaGpuManager, scalars, bases, curve: int = BN254) -> np.ndarray:
    """unit.rs:10-101: stage scalars and bases, run, return the 96-byte X||Y||Z."""
    s = _as_bytes(scalars)
    with _Buffers(gm) as b:
        d_scalars = b.upload_pool(s, gm.h2d_stream)
        b.wait_h2d()
        d_bases = b.upload_pool(bases, gm.h2d_stream)
        b.wait_h2d()
        return _msm_device(b, d_scalars, d_bases, log_2(s.size // FIELD_ELEMENT_LEN), curve)


def pipeline_chunks(log_n: int) -> int:
    """Point ranges a single call's upload / execute pipeline is cut into: n/2^(R-1), n/2^(R-1), n/2^(R-2), ..., n/2 points (the
    library lowers R until the first range holds 2^16 points)."""
    return 5 if log_n >= 24 else (4 if log_n >= 22 else (3 if log_n >= 20 else (2 if log_n >= 18 else 1)))


def panda_msm_bn254_gpu_with_cached_bases(gm: PandaGpuManager, scalars, bases_index: int, curve: int = BN254) -> np.ndarray:
    """unit.rs:103-188.  When the cached base set is registered with the library (register_cached_bases /
    precompute_cached_bases) the upload and the execution are pipelined inside the one call: the scalars cross
    PCIe range by range on the h2d stream while the previous range is already being accumulated on the exec stream
    (panda_msm_execute_from_host); otherwise the reference's order -- upload everything, then execute."""
    s = _as_bytes(scalars)
    d_bases = gm.get_params_bases_ptr_mut(bases_index)
    if d_bases is None:
        raise PandaGpuError("BasesIndexErr")
    log_n = log_2(s.size // FIELD_ELEMENT_LEN)
    chunks = pipeline_chunks(log_n)
    with _Buffers(gm) as b:
        if d_bases in gm._registered and chunks > 1:
            nres = _RESULT_BYTES[curve]
            d_scalars = b.pool((1 << log_n) * FIELD_ELEMENT_LEN, gm.h2d_stream)
            d_result = b.pool(nres, gm.h2d_stream)
            b.wait_h2d()
            cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, d_bases, d_scalars, d_result, log_n, gm.msm_result_coordinate_type)
            ffi.check(b.lib.panda_msm_execute_from_host(curve, cfg, _ptr(s), chunks, gm.h2d_stream.raw), "SchedulingErr")
            return b.download(d_result, nres)
        d_scalars = b.upload_pool(s, gm.h2d_stream)
        b.wait_h2d()
        return _msm_device(b, d_scalars, d_bases, log_n, curve)


def panda_msm_bn254_gpu_with_cached_bases_batched(gm: PandaGpuManager, scalars_batches, bases_index: int, curve: int = BN254) -> list:
    """Additive: a run of MSMs over one cached base set, using the manager's three streams the way
    wrapper.rs:12-14 intends them: the scalars of batch k+1 cross PCIe on the h2d stream while batch k executes on the
    exec stream; an event orders each execute after its own upload.  Two device buffers and one pinned staging buffer
    per slot, allocated once.  Returns the results in order; each equals panda_msm_bn254_gpu_with_cached_bases."""
    batches = [_as_bytes(b) for b in scalars_batches]
    if not batches:
        return []
    d_bases = gm.get_params_bases_ptr_mut(bases_index)
    if d_bases is None:
        raise PandaGpuError("BasesIndexErr")
    size = batches[0].size
    if any(b.size != size for b in batches):
        raise PandaGpuError("SchedulingErr")
    log_n = log_2(size // FIELD_ELEMENT_LEN)
    nres = _RESULT_BYTES[curve]
    results = []
    with _Buffers(gm) as b:
        lib = b.lib
        fn = _msm_entry(lib, curve)
        try:
            slots = [(b.device(size), b.event(), b.pinned(size), b.pinned(nres)) for _ in range(min(2, len(batches)))]

            def upload(k):
                dev, ev, pin, _ = slots[k & 1]
                C.memmove(pin, _ptr(batches[k]), size)  # pageable -> pinned, on the host while the GPU works
                ffi.check(lib.panda_memcpy_async(dev, pin, size, gm.h2d_stream.raw), "AsyncMemcopyErr")
                ev.record(gm.h2d_stream)

            upload(0)
            for k in range(len(batches)):
                dev, ev, _, res = slots[k & 1]
                gm.exec_stream.wait(ev)
                if k + 1 < len(batches):
                    upload(k + 1)  # the other slot: its previous execute has returned, so its buffers are free
                cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, d_bases, dev, res, log_n, gm.msm_result_coordinate_type)
                ffi.check(fn(cfg), "SchedulingErr")  # synchronous: the result is in `res` on return
                results.append(np.frombuffer((C.c_uint8 * nres).from_address(res.value), dtype=np.uint8).copy())
        finally:
            gm.h2d_stream.sync()  # no copy may still be on its way into a buffer that the exit frees
    return results


def panda_msm_gpu_batch_with_cached_bases(gm: PandaGpuManager, scalars_batches, bases_index: int, curve: int = BN254) -> list:
    """Additive: a run of MSMs over one cached base set in ONE library call (panda_msm_execute_batch).  The vectors are uploaded into one
    device buffer, member after member; against precomputed tables (precompute_cached_bases) the library fuses groups of members into one
    sort + accumulate each, otherwise it runs them one after the other.  Returns the results in order; each is the same group element
    as panda_msm_bn254_gpu_with_cached_bases on that vector."""
    batches = [_as_bytes(b) for b in scalars_batches]
    if not batches:
        return []
    d_bases = gm.get_params_bases_ptr_mut(bases_index)
    if d_bases is None:
        raise PandaGpuError("BasesIndexErr")
    size = batches[0].size
    if any(b.size != size for b in batches):
        raise PandaGpuError("SchedulingErr")
    log_n = log_2(size // FIELD_ELEMENT_LEN)
    nres = _RESULT_BYTES[curve]
    out = np.zeros(len(batches) * nres, dtype=np.uint8)  # pageable host memory: the library copies the results out itself
    with _Buffers(gm) as b:
        dev = b.fill(b.device(len(batches) * size), batches)
        cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, d_bases, dev, _ptr(out), log_n, gm.msm_result_coordinate_type)
        ffi.check(b.lib.panda_msm_execute_batch(curve, cfg, len(batches)), "SchedulingErr")
    return [out[k * nres:(k + 1) * nres].copy() for k in range(len(batches))]


def panda_msm_bn254_gpu_with_cached_scalars(gm: PandaGpuManager, scalars_index: int, bases, curve: int = BN254) -> np.ndarray:
    """unit.rs:190-275: n comes from the bases length (len / 64, unit.rs:203)."""
    h = _as_bytes(bases)
    with _Buffers(gm) as b:
        d_bases = b.upload_pool(h, gm.h2d_stream)
        b.wait_h2d()
        d_scalars = gm.get_params_scalars_ptr_mut(scalars_index)
        if d_scalars is None:
            raise PandaGpuError("BasesIndexErr")
        return _msm_device(b, d_scalars, d_bases, log_2(h.size // _POINT_BYTES[curve]), curve)


def panda_msm_bn254_gpu_with_cached_input(gm: PandaGpuManager, scalars_index: int, bases_index: int, curve: int = BN254) -> np.ndarray:
    """unit.rs:277-361."""
    d_scalars = gm.get_params_scalars_ptr_mut(scalars_index)
    d_bases = gm.get_params_bases_ptr_mut(bases_index)
    if d_scalars is None or d_bases is None:
        raise PandaGpuError("BasesIndexErr")
    log_n = log_2(gm.get_params_scalars_len(scalars_index) // FIELD_ELEMENT_LEN)
    with _Buffers(gm) as b:
        return _msm_device(b, d_scalars, d_bases, log_n, curve)


def panda_msm_bn254_gpu_host(gm, scalars, bases, curve: int = BN254) -> np.ndarray:
    """unit.rs:363-416: the CPU host-debug entry point; every pointer is a host pointer.  `gm` may be None
    (the reference needs a live device only because of init_all, wrapper.rs:61-66)."""
    s, b = _as_bytes(scalars), _as_bytes(bases)
    lib = ffi.load()
    out = np.zeros(_RESULT_BYTES[curve], dtype=np.uint8)
    coord = gm.msm_result_coordinate_type if gm is not None else JACOBIAN
    cfg = ffi.MSMConfiguration(ffi.PandaMemPool(), ffi.PandaStream(), _ptr(b), _ptr(s), _ptr(out), log_2(s.size // FIELD_ELEMENT_LEN), coord)
    fn = _msm_entry(lib, curve, host=True)
    ffi.check(fn(cfg), "SchedulingErr")
    return out


def _ntt(gm, scalars: np.ndarray, log_n: int, call, omega=None):
    buf = _as_bytes(scalars)
    assert buf.size == (1 << log_n) * 32  # unit.rs:423
    flag = C.c_uint(0)
    with _Buffers(gm) as b:
        d_src = b.upload_pool(buf, gm.h2d_stream)
        d_dst = b.pool(buf.size, gm.h2d_stream)
        if omega is None:
            cfg = ffi.NTTConfiguration(gm.mem_pool, gm.exec_stream.raw, d_src, d_dst, log_n, C.pointer(flag))
        else:
            o = _as_bytes(omega)
            cfg = ffi.NttconfigurationV1(gm.mem_pool, gm.exec_stream.raw, d_src, d_dst, _ptr(o), log_n, C.pointer(flag))
        ffi.check(call(cfg), "SchedulingErr")
        b.read(buf, d_src if flag.value == 0 else d_dst)  # unit.rs:521-532
    return flag.value


def panda_ntt_bn254_gpu(gm: PandaGpuManager, scalars: np.ndarray, log_n: int) -> int:
    """unit.rs:418-479: in place on the caller's buffer, omega from init_ntt; returns the flag for inspection."""
    return _ntt(gm, scalars, log_n, ffi.load().panda_ntt_execute_bn254)


def panda_ntt_bn254_gpu_v1(gm: PandaGpuManager, scalars: np.ndarray, omega, log_n: int) -> int:
    """unit.rs:481-543."""
    return _ntt(gm, scalars, log_n, ffi.load().panda_ntt_execute_bn254_v1, omega)


def panda_coset_ntt_bn254_gpu(gm: PandaGpuManager, scalars: np.ndarray, omega, shift, log_n: int, inverse: bool = False) -> int:
    """Additive: coset transform, in place.  Forward y[k] = sum_j x[j] g^j w^(jk); inverse undoes it (n^-1 and g^-j fused)."""
    lib = ffi.load()
    g = _as_bytes(shift)
    fn = lib.panda_ntt_execute_bn254_coset_inverse if inverse else lib.panda_ntt_execute_bn254_coset
    return _ntt(gm, scalars, log_n, lambda cfg: fn(cfg, _ptr(g)), omega)


def panda_ntt_bls12_381_gpu_v1(gm: PandaGpuManager, scalars: np.ndarray, omega, log_n: int, inverse: bool = False) -> int:
    """Additive: the v1 transform over the BLS12-381 scalar field (two-adicity 32)."""
    lib = ffi.load()
    return _ntt(gm, scalars, log_n, lib.panda_ntt_execute_bls12_381_inverse if inverse else lib.panda_ntt_execute_bls12_381_v1, omega)


def panda_ntt_bls12_377_gpu_v1(gm: PandaGpuManager, scalars: np.ndarray, omega, log_n: int, inverse: bool = False) -> int:
    """Additive: the same staging for the BLS12-377 scalar field."""
    lib = ffi.load()
    return _ntt(gm, scalars, log_n, lib.panda_ntt_execute_bls12_377_inverse if inverse else lib.panda_ntt_execute_bls12_377_v1, omega)


def panda_ntt_bls12_377_gpu_bitrev(gm: PandaGpuManager, scalars: np.ndarray, omega, log_n: int, inverse: bool = False, field: str = "bls12_377") -> int:
    """Additive: the bit-reversed orderings of panda_ntt_bn254_gpu_bitrev over the BLS12-377 (or, field="bls12_381", BLS12-381) scalar field."""
    lib = ffi.load()
    return _ntt(gm, scalars, log_n, getattr(lib, f"panda_ntt_execute_{field}_inverse_bitrev_in" if inverse else f"panda_ntt_execute_{field}_bitrev_out"), omega)


def panda_coset_ntt_bls12_377_gpu(gm: PandaGpuManager, scalars: np.ndarray, omega, shift, log_n: int, inverse: bool = False, field: str = "bls12_377") -> int:
    """Additive: coset transform over the BLS12-377 (or BLS12-381) scalar field (as panda_coset_ntt_bn254_gpu)."""
    lib = ffi.load()
    g = _as_bytes(shift)
    fn = getattr(lib, f"panda_ntt_execute_{field}_coset_inverse" if inverse else f"panda_ntt_execute_{field}_coset")
    return _ntt(gm, scalars, log_n, lambda cfg: fn(cfg, _ptr(g)), omega)


def panda_intt_bn254_gpu(gm: PandaGpuManager, scalars: np.ndarray, omega, log_n: int) -> int:
    """Additive: inverse transform with the n^-1 scaling fused (panda_ntt_execute_bn254_inverse)."""
    return _ntt(gm, scalars, log_n, ffi.load().panda_ntt_execute_bn254_inverse, omega)


def panda_ntt_bn254_gpu_bitrev(gm: PandaGpuManager, scalars: np.ndarray, omega, log_n: int, inverse: bool = False) -> int:
    """Additive: forward transform leaving y[k] at bitrev(k), or (inverse=True) the inverse of a buffer in that order back to
    natural-order coefficients with n^-1 fused.  In place on the caller's buffer like panda_ntt_bn254_gpu_v1."""
    lib = ffi.load()
    return _ntt(gm, scalars, log_n, lib.panda_ntt_execute_bn254_inverse_bitrev_in if inverse else lib.panda_ntt_execute_bn254_bitrev_out, omega)


def panda_ntt_gpu_batch(gm: PandaGpuManager, polys, omega, log_n: int, field: int = 0, kind: int = 0, shift=None) -> int:
    """Additive: transforms of one size, field (0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr), kind (ffi.NTT_FORWARD ...) and root in ONE
    library call (panda_ntt_execute_batch).  The equal-length host arrays are staged into one device buffer, member after member, and
    each is overwritten in place with its result, which is what the single call of that kind writes for it.  `shift` is the coset
    generator of the coset kinds.  Returns the flag; an empty list returns 0 without a call."""
    bufs = [_as_bytes(p) for p in polys]
    if not bufs:
        return 0
    size = (1 << log_n) * FIELD_ELEMENT_LEN
    if any(b.size != size for b in bufs):
        raise PandaGpuError("SchedulingErr")
    o = _as_bytes(omega)
    g = _as_bytes(shift) if shift is not None else None
    flag = C.c_uint(0)
    with _Buffers(gm) as b:
        d_src, d_dst = b.device(len(bufs) * size), b.device(len(bufs) * size)
        b.fill(d_src, bufs)
        cfg = ffi.NttconfigurationV1(gm.mem_pool, gm.exec_stream.raw, d_src, d_dst, _ptr(o), log_n, C.pointer(flag))
        ffi.check(b.lib.panda_ntt_execute_batch(field, kind, cfg, len(bufs), _ptr(g) if g is not None else None), "SchedulingErr")
        res = d_src.value if flag.value == 0 else d_dst.value
        for k, buf in enumerate(bufs):
            b.read(buf, res + k * size)
    return flag.value


def panda_ntt_gpu_lde(gm: PandaGpuManager, polys, omega_N, log_n: int, log_blowup: int, shift, field: int = 0, order: int = 0):
    """Additive: the low-degree extension of equal-length coefficient arrays of 2^log_n elements (field 0 BN254 Fr, 1 BLS12-377 Fr,
    2 BLS12-381 Fr) to the coset shift * H of the 2^log_blowup times larger domain with root `omega_N`, in ONE library call
    (panda_ntt_execute_lde).  The host arrays are staged into one device buffer, polynomial after polynomial, and are not changed.
    Returns a list of 2^(log_n + log_blowup)-element arrays (uint32, 8 words per element) in `order` (ffi.NTT_LDE_COSET_MAJOR: the
    2^log_blowup cosets of the small domain one after the other; ffi.NTT_LDE_NATURAL: the order of a coset transform of the padded
    polynomial); an empty list returns an empty list without a call."""
    bufs = [_as_bytes(p) for p in polys]
    if not bufs:
        return []
    size = (1 << log_n) * FIELD_ELEMENT_LEN
    if any(b.size != size for b in bufs):
        raise PandaGpuError("SchedulingErr")
    o, g = _as_bytes(omega_N), _as_bytes(shift)
    big = size << log_blowup
    flag = C.c_uint(0)
    with _Buffers(gm) as b:
        d_coeffs, d_src, d_dst = b.device(len(bufs) * size), b.device(len(bufs) * big), b.device(len(bufs) * big)
        b.fill(d_coeffs, bufs)
        cfg = ffi.NttconfigurationV1(gm.mem_pool, gm.exec_stream.raw, d_src, d_dst, _ptr(o), log_n, C.pointer(flag))
        ffi.check(b.lib.panda_ntt_execute_lde(field, cfg, d_coeffs, log_blowup, len(bufs), _ptr(g), order), "SchedulingErr")
        return b.download_vectors(d_src if flag.value == 0 else d_dst, len(bufs), big // FIELD_ELEMENT_LEN)


def panda_poly_gpu_evaluate(gm: PandaGpuManager, polys, points, field: int = 0) -> np.ndarray:
    """Additive: the values of equal-length coefficient arrays (any length from 1 up; field 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr)
    at up to ffi.POLY_MAX_POINTS points in ONE library call (panda_poly_evaluate).  `points` is a (n_points, 8) uint32 array of
    Montgomery-form elements.  The host arrays are staged into one device buffer and are not changed.  Returns a (batch, n_points, 8)
    uint32 array, value (p, k) = polys[p] at points[k]; an empty list returns an empty (0, n_points, 8) array without a call."""
    pts = np.ascontiguousarray(points, np.uint32).reshape(-1, 8)
    if len(polys) == 0:
        return np.empty((0, len(pts), 8), np.uint32)
    with _Buffers(gm) as b:
        d, batch, n = b.upload(polys)
        values = np.empty((batch, len(pts), 8), np.uint32)
        ffi.check(b.lib.panda_poly_evaluate(field, d, n, batch, _ptr(pts), len(pts), _ptr(values), gm.exec_stream.raw), "SchedulingErr")
    return values


def panda_poly_gpu_divide(gm: PandaGpuManager, polys, point, field: int = 0):
    """Additive: the quotients (f - f(z)) / (X - z) of equal-length coefficient arrays by ONE library call (panda_poly_divide_linear),
    in place on the staged device copy; the host arrays are not changed.  Returns (quotients, remainders): a list of (n, 8) uint32 arrays
    (the last element of each is zero) and a (batch, 8) uint32 array of the values f(z); an empty list returns ([], an empty (0, 8)
    array) without a call."""
    if len(polys) == 0:
        return [], np.empty((0, 8), np.uint32)
    z = np.ascontiguousarray(point, np.uint32).reshape(8)
    with _Buffers(gm) as b:
        d, batch, n = b.upload(polys)
        remainders = np.empty((batch, 8), np.uint32)
        ffi.check(b.lib.panda_poly_divide_linear(field, d, d, n, batch, _ptr(z), _ptr(remainders), gm.exec_stream.raw), "SchedulingErr")
        return b.download_vectors(d, batch, n), remainders


def _lagrange_domain(polys_n, omega, shift):
    """(log_n, omega words, shift pointer or None) of a call on evaluation-form vectors of polys_n elements"""
    if polys_n & (polys_n - 1):
        raise PandaGpuError("SchedulingErr")
    o = np.ascontiguousarray(omega, np.uint32).reshape(8)
    s = None if shift is None else np.ascontiguousarray(shift, np.uint32).reshape(8)
    return polys_n.bit_length() - 1, o, s


def panda_poly_gpu_evaluate_lagrange(gm: PandaGpuManager, evals, omega, points, field: int = 0, shift=None, order: int = 0) -> np.ndarray:
    """Additive: the values at up to ffi.POLY_MAX_POINTS points of the polynomials that equal-length vectors of n = 2^k evaluations on
    the domain shift * omega^i stand for (natural order, or ffi.DOMAIN_BITREV), by ONE library call (panda_poly_evaluate_lagrange)
    and without a transform; points on the domain return the stored element.  `omega`, `shift` and the rows of `points` are (8,) uint32
    Montgomery-form elements.  The host arrays are staged into one device buffer and are not changed.  Returns a (batch, n_points, 8)
    uint32 array; an empty list returns an empty (0, n_points, 8) array without a call."""
    pts = np.ascontiguousarray(points, np.uint32).reshape(-1, 8)
    if len(evals) == 0:
        return np.empty((0, len(pts), 8), np.uint32)
    with _Buffers(gm) as b:
        d, batch, n = b.upload(evals)
        log_n, o, s = _lagrange_domain(n, omega, shift)
        values = np.empty((batch, len(pts), 8), np.uint32)
        ffi.check(b.lib.panda_poly_evaluate_lagrange(field, d, log_n, batch, _ptr(o), None if s is None else _ptr(s), order, _ptr(pts), len(pts), _ptr(values),
                                                     gm.exec_stream.raw), "SchedulingErr")
    return values


def panda_poly_gpu_divide_lagrange(gm: PandaGpuManager, evals, omega, point, field: int = 0, shift=None, order: int = 0):
    """Additive: the quotients (f - f(z)) / (X - z) of evaluation-form vectors, as evaluations on the same domain in the same order, by
    ONE library call (panda_poly_divide_linear_lagrange) in place on the staged device copy; the host arrays are not changed.  Returns
    (quotients, remainders): a list of (n, 8) uint32 arrays and a (batch, 8) uint32 array of the values f(z); an empty list returns
    ([], an empty (0, 8) array) without a call."""
    if len(evals) == 0:
        return [], np.empty((0, 8), np.uint32)
    z = np.ascontiguousarray(point, np.uint32).reshape(8)
    with _Buffers(gm) as b:
        d, batch, n = b.upload(evals)
        log_n, o, s = _lagrange_domain(n, omega, shift)
        remainders = np.empty((batch, 8), np.uint32)
        ffi.check(b.lib.panda_poly_divide_linear_lagrange(field, d, d, log_n, batch, _ptr(o), None if s is None else _ptr(s), order, _ptr(z), _ptr(remainders),
                                                          gm.exec_stream.raw), "SchedulingErr")
        return b.download_vectors(d, batch, n), remainders


def panda_field_gpu_batch_inverse(gm: PandaGpuManager, values, field: int = 0):
    """Additive: the inverses of equal-length arrays of Montgomery-form elements (any length from 1 up; field 0 BN254 Fr, 1 BLS12-377 Fr,
    2 BLS12-381 Fr), zero for zero, by ONE library call (panda_field_batch_inverse over the staged arrays end to end, in place on the
    device copy); the host arrays are not changed.  Returns a list of (n, 8) uint32 arrays; an empty list returns [] without a call."""
    if len(values) == 0:
        return []
    with _Buffers(gm) as b:
        d, batch, n = b.upload(values)
        ffi.check(b.lib.panda_field_batch_inverse(field, d, d, batch * n, gm.exec_stream.raw), "SchedulingErr")
        return b.download_vectors(d, batch, n)


def panda_poly_gpu_grand_product(gm: PandaGpuManager, nums, dens, field: int = 0):
    """Additive: the exclusive running products Z_0 = 1, Z_i = prod_{j < i} nums[p][j] / dens[p][j] of equal-length arrays by ONE library
    call (panda_poly_grand_product, in place on the staged numerators); dens=None is the plain running product of nums.  The host arrays
    are not changed.  Returns (products, totals): a list of (n, 8) uint32 arrays and a (batch, 8) uint32 array of the full products; a
    vector with a zero denominator comes back all zero.  An empty list returns ([], an empty (0, 8) array) without a call."""
    if len(nums) == 0:
        return [], np.empty((0, 8), np.uint32)
    if dens is not None and len(dens) != len(nums):
        raise PandaGpuError("SchedulingErr")
    with _Buffers(gm) as b:
        d_num, batch, n = b.upload(nums)
        d_den = None
        if dens is not None:
            d_den, batch_den, n_den = b.upload(dens)
            if (batch_den, n_den) != (batch, n):
                raise PandaGpuError("SchedulingErr")
        totals = np.empty((batch, 8), np.uint32)
        ffi.check(b.lib.panda_poly_grand_product(field, d_num, d_den, d_num, n, batch, _ptr(totals), gm.exec_stream.raw), "SchedulingErr")
        return b.download_vectors(d_num, batch, n), totals


def panda_lookup_gpu_multiplicities(gm: PandaGpuManager, table, columns, field: int = 0):
    """Additive: the logUp multiplicities of a lookup by ONE library call (panda_lookup_multiplicities): `table` is an (n_table, 8) uint32
    array of Montgomery-form elements, `columns` a list of 1..ffi.LOOKUP_MAX_COLUMNS equal-length (n, 8) arrays.  Returns (mult, missing,
    first_missing): mult (n_table, 8) holds at the first row of every table value the wire form of the number of column elements equal
    to it and zero at its later duplicates; missing counts the column elements found nowhere in the table and first_missing is
    (column << 32) | index of the smallest such pair, 2^64 - 1 when there is none.  The host arrays are not changed."""
    if len(columns) == 0 or len(columns) > ffi.LOOKUP_MAX_COLUMNS:
        raise PandaGpuError("SchedulingErr")
    with _Buffers(gm) as b:
        d_table, _, n_table = b.upload([table])
        d_cols, n_columns, n = b.upload(columns)
        d_mult = b.device(n_table * FIELD_ELEMENT_LEN)
        ptrs = (C.c_void_p * n_columns)(*[d_cols.value + k * n * FIELD_ELEMENT_LEN for k in range(n_columns)])
        missing, first = C.c_uint64(0), C.c_uint64(0)
        ffi.check(b.lib.panda_lookup_multiplicities(field, d_table, n_table, ptrs, n_columns, n, d_mult, C.byref(missing), C.byref(first), gm.exec_stream.raw),
                  "SchedulingErr")
        return b.download_vectors(d_mult, 1, n_table)[0], missing.value, first.value


def panda_poly_gpu_running_sum(gm: PandaGpuManager, vectors, field: int = 0):
    """Additive: the exclusive running sums Z_0 = 0, Z_i = sum_{j < i} vectors[p][j] of equal-length arrays by ONE library call
    (panda_poly_running_sum, in place on the staged vectors).  The host arrays are not changed.  Returns (sums, totals): a list of (n, 8)
    uint32 arrays and a (batch, 8) uint32 array of the full sums.  An empty list returns ([], an empty (0, 8) array) without a call."""
    if len(vectors) == 0:
        return [], np.empty((0, 8), np.uint32)
    with _Buffers(gm) as b:
        d, batch, n = b.upload(vectors)
        totals = np.empty((batch, 8), np.uint32)
        ffi.check(b.lib.panda_poly_running_sum(field, d, d, n, batch, _ptr(totals), gm.exec_stream.raw), "SchedulingErr")
        return b.download_vectors(d, batch, n), totals


def panda_poly_gpu_sum_of_products(gm: PandaGpuManager, columns, terms, field: int = 0, scales=None, scale_mode: int = 0) -> np.ndarray:
    """Additive: out[p][i] = s(p, i) * sum_t coeff_t * prod_f columns[c_tf][p][(i + r_tf) mod n] by ONE library call
    (panda_poly_sum_of_products): gates, permutation checks, a b - c, folds with powers of a challenge -- any sum of monomials over
    columns of Montgomery-form elements (field 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr).  `columns` is a list of equally shaped uint32
    arrays, (n, 8) or (batch, n, 8); `terms` a list of (coeff, [(column, rotation), ...]) with coeff an 8-word element and an empty
    factor list for a constant term; `scales` an (n_scales, 8) array with scale_mode ffi.SOP_SCALE_PER_VECTOR (s = scales[p mod n_scales])
    or ffi.SOP_SCALE_CYCLIC (s = scales[i mod n_scales]).  The host arrays are staged into one device buffer and are not changed.
    Returns an array of the columns' shape."""
    cols = [np.ascontiguousarray(c, np.uint32) for c in columns]
    if not cols or not terms or cols[0].ndim not in (2, 3) or cols[0].shape[-1] != 8 or any(c.shape != cols[0].shape for c in cols):
        raise PandaGpuError("SchedulingErr")
    shape = cols[0].shape
    batch, n = (1, shape[0]) if len(shape) == 2 else shape[:2]
    coeffs = np.ascontiguousarray([np.asarray(k, np.uint32).reshape(8) for k, _ in terms], np.uint32)
    degrees = (C.c_uint * len(terms))(*[len(fs) for _, fs in terms])
    flat = [(c, r) for _, fs in terms for c, r in fs]
    factors = (ffi.SopFactor * max(len(flat), 1))(*[ffi.SopFactor(c, r) for c, r in flat])
    sc = None if scales is None else np.ascontiguousarray(scales, np.uint32).reshape(-1, 8)
    with _Buffers(gm) as b:
        d, _, _ = b.upload(cols)
        size = batch * n * FIELD_ELEMENT_LEN
        d_out = b.device(size)
        ptrs = (C.c_void_p * len(cols))(*[d.value + k * size for k in range(len(cols))])
        expr = ffi.SopExpression(ptrs, _ptr(coeffs), degrees, factors, None if sc is None else _ptr(sc), len(cols), len(terms),
                                 0 if sc is None else len(sc), scale_mode)
        ffi.check(b.lib.panda_poly_sum_of_products(field, C.byref(expr), d_out, n, batch, gm.exec_stream.raw), "SchedulingErr")
        return b.read(np.empty(shape, np.uint32), d_out)


def panda_mle_gpu_eq_table(gm: PandaGpuManager, point, field: int = 0) -> np.ndarray:
    """Additive: the table eq(r, x) = prod_j (x_j r_j + (1 - x_j)(1 - r_j)) over x < 2^k for the point r = `point`, a (k, 8) uint32 array of
    Montgomery-form elements (k may be 0), by ONE library call (panda_mle_eq_table).  Returns a (2^k, 8) uint32 array."""
    pt = np.ascontiguousarray(point, np.uint32).reshape(-1, 8)
    log_n = len(pt)
    if log_n > 28:
        raise PandaGpuError("SchedulingErr")
    host = pt if log_n else np.zeros((1, 8), np.uint32)
    with _Buffers(gm) as b:
        d = b.device(FIELD_ELEMENT_LEN << log_n)
        ffi.check(b.lib.panda_mle_eq_table(field, _ptr(host), log_n, d, gm.exec_stream.raw), "SchedulingErr")
        return b.read(np.empty((1 << log_n, 8), np.uint32), d)


def panda_sumcheck_gpu_run(gm: PandaGpuManager, columns, terms, n_evals: int, challenges, field: int = 0, order: int = 0, fused: bool = False):
    """Additive: the prover's side of a whole sumcheck over multilinear tables.  `columns` is a list of (2^k, 8) uint32 arrays of
    Montgomery-form elements, k >= 1; `terms` a list of (coeff, [column, ...]) with coeff an 8-word element and an empty list for a
    constant term; `challenges` a (k, 8) array, one per round, supplied by the caller (the transcript is the host's business); `order`
    ffi.MLE_BIND_LOW or ffi.MLE_BIND_HIGH.  The tables are staged once and the rounds ping-pong between two buffer sets: with `fused` one
    plain panda_sumcheck_round and k - 1 fused ones, otherwise a plain round and a panda_mle_fold per round; a last panda_mle_fold gives
    the final values.  fused=False is the default: at 2^24 the fused rounds were faster on eq (a b - c) but not on the gate times eq
    (DESIGN.md 5.7).  The host arrays are not
    changed.  Returns (round_evals, final_values): a (k, n_evals, 8) array of g_j(0 .. n_evals - 1) and a (len(columns), 8) array of the
    tables' values at the point of the challenges."""
    cols = [np.ascontiguousarray(c, np.uint32) for c in columns]
    ch = np.ascontiguousarray(challenges, np.uint32).reshape(-1, 8)
    if not cols or not terms or cols[0].ndim != 2 or cols[0].shape[1] != 8 or any(c.shape != cols[0].shape for c in cols):
        raise PandaGpuError("SchedulingErr")
    n = cols[0].shape[0]
    k = log_2(n)
    if n < 2 or n != 1 << k or len(ch) != k or not 1 <= n_evals <= ffi.SUMCHECK_MAX_EVALS:
        raise PandaGpuError("SchedulingErr")
    coeffs = np.ascontiguousarray([np.asarray(c, np.uint32).reshape(8) for c, _ in terms], np.uint32)
    degrees = (C.c_uint * len(terms))(*[len(fs) for _, fs in terms])
    flat = [c for _, fs in terms for c in fs]
    factors = (ffi.SopFactor * max(len(flat), 1))(*[ffi.SopFactor(c, 0) for c in flat])
    m = len(cols)
    size = n * FIELD_ELEMENT_LEN
    with _Buffers(gm) as b:
        lib = b.lib
        d, _, _ = b.upload(cols)
        d_other = b.device(m * (size // 2))
        stream = gm.exec_stream.raw
        evals = np.zeros((k, n_evals, 8), np.uint32)
        # the tables of round j are 2^(k - j) elements each; set 0 is the staged buffer, set 1 holds at most half-size tables
        sets = ([d.value + c * size for c in range(m)], [d_other.value + c * (size // 2) for c in range(m)])

        def pointers(which):
            return (C.c_void_p * m)(*sets[which])

        def round_call(j, src, challenge=None, dst=None):
            expr = ffi.SopExpression(pointers(src), _ptr(coeffs), degrees, factors, None, m, len(terms), 0, ffi.SOP_SCALE_NONE)
            log_n = k - j + (1 if dst is not None else 0)
            ffi.check(lib.panda_sumcheck_round(field, C.byref(expr), log_n, order, n_evals, None if challenge is None else _ptr(challenge),
                                               None if dst is None else pointers(dst), _ptr(evals[j]), stream), "SchedulingErr")

        cur = 0
        round_call(0, cur)
        for j in range(1, k):
            if fused:
                round_call(j, cur, ch[j - 1], 1 - cur)
                cur = 1 - cur
            else:
                ffi.check(lib.panda_mle_fold(field, pointers(cur), pointers(1 - cur), m, k - j + 1, order, _ptr(ch[j - 1]), stream), "SchedulingErr")
                cur = 1 - cur
                round_call(j, cur)
        ffi.check(lib.panda_mle_fold(field, pointers(cur), pointers(1 - cur), m, 1, order, _ptr(ch[k - 1]), stream), "SchedulingErr")
        final = np.empty((m, 8), np.uint32)
        for c in range(m):
            b.read(final[c], sets[1 - cur][c])
        return evals, final


class PandaSparseMatrix:
    """Additive: a CSR matrix over a scalar field kept resident on the device across products -- the A, B or C of an R1CS, staged once
    per circuit.  `row_ptr` holds n_rows + 1 and `col` nnz uint32 entries, `values` is an (nnz, 8) uint32 array of Montgomery-form elements
    (field 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr).  The structure is checked once on the device (panda_sparse_check); a defect raises
    PandaGpuError naming its class and index.  free() releases the device copy."""

    DEFECTS = {1: "row_ptr[0] != 0", 2: "row_ptr decreases", 3: "row_ptr[n_rows] != nnz", 4: "column index >= n_cols", 5: "value >= modulus"}

    def __init__(self, gm: PandaGpuManager, row_ptr, col, values, n_cols: int, field: int = 0):
        rp = np.ascontiguousarray(row_ptr, np.uint32).reshape(-1)
        cl = np.ascontiguousarray(col, np.uint32).reshape(-1)
        vals = np.ascontiguousarray(values, np.uint32).reshape(-1, 8)
        if len(rp) < 2 or len(vals) != len(cl) or n_cols < 1:
            raise PandaGpuError("SchedulingErr")
        self.gm, self.field = gm, field
        self.n_rows, self.n_cols, self.nnz = len(rp) - 1, int(n_cols), len(cl)
        with _Buffers(gm) as b:
            ptrs = [b.send(b.device(a.nbytes), a) if a.size else None for a in (rp, cl, vals)]
            b.wait_h2d()
            self.matrix = ffi.CsrMatrix(ptrs[0], ptrs[1], ptrs[2], self.n_rows, self.n_cols, self.nnz)
            defect, where = C.c_uint(0), C.c_uint64(0)
            ffi.check(b.lib.panda_sparse_check(field, C.byref(self.matrix), C.byref(defect), C.byref(where), gm.exec_stream.raw), "SchedulingErr")
            if defect.value:
                at = "" if where.value == 0xFFFFFFFFFFFFFFFF else f" at {where.value}"
                raise PandaGpuError(f"SparseDefect{defect.value}: {self.DEFECTS.get(defect.value, '?')}{at}")
            self._bufs = [b.keep(d) for d in ptrs if d is not None]

    def matvec(self, z) -> np.ndarray:
        """M z for z an (n_cols, 8) or (batch, n_cols, 8) uint32 array by ONE library call (panda_sparse_matvec); returns (n_rows, 8) or
        (batch, n_rows, 8).  The host array is not changed."""
        zs = np.ascontiguousarray(z, np.uint32)
        if zs.ndim not in (2, 3) or zs.shape[-2:] != (self.n_cols, 8):
            raise PandaGpuError("SchedulingErr")
        batch = 1 if zs.ndim == 2 else zs.shape[0]
        if batch == 0:
            return np.empty((0, self.n_rows, 8), np.uint32)
        with _Buffers(self.gm) as b:
            d_z, _, _ = b.upload([zs.reshape(-1, 8)])
            d_out = b.device(batch * self.n_rows * FIELD_ELEMENT_LEN)
            ffi.check(b.lib.panda_sparse_matvec(self.field, C.byref(self.matrix), d_z, d_out, batch, self.gm.exec_stream.raw), "SchedulingErr")
            return b.read(np.empty((self.n_rows, 8) if zs.ndim == 2 else (batch, self.n_rows, 8), np.uint32), d_out)

    def free(self):
        lib = ffi.load()
        for d in self._bufs:
            lib.panda_free(d)
        self._bufs = []


def panda_sparse_gpu_matvec(gm: PandaGpuManager, row_ptr, col, values, z, n_cols: int, field: int = 0) -> np.ndarray:
    """Additive: the sparse product out[r] = sum_{k in row r} values[k] z[col[k]] of a CSR matrix and a vector (or a batch of vectors) over
    a scalar field: stages the matrix, checks its structure on the device (a defect raises PandaGpuError), runs panda_sparse_matvec and
    returns the product.  A caller with one circuit and many witnesses keeps a PandaSparseMatrix instead."""
    m = PandaSparseMatrix(gm, row_ptr, col, values, n_cols, field)
    try:
        return m.matvec(z)
    finally:
        m.free()


def panda_ec_ntt_gpu(gm: PandaGpuManager, points, omega, curve: int = BN254, inverse: bool = False) -> np.ndarray:
    """Additive: the discrete Fourier transform of n = 2^k affine G1 points (the MSM's base wire form, x || y, identity <=> x == 0) over
    the group, out[k] = sum_j omega^(jk) P_j, natural order; `omega` is the FORWARD root of order n (one Montgomery-form scalar, 32 B)
    for both directions, and inverse=True uses omega^-1 and multiplies by 1 / n -- the inverse transform of a monomial SRS is the
    Lagrange-basis SRS.  One library call (panda_ec_ntt, in place on the device copy); the host array is not changed.  Returns
    (n, point bytes) uint8: canonical affine points, the identity as all-zero bytes, ready for add_cached_bases.  curve is a G1 id."""
    pb = _POINT_BYTES[curve]
    h = _as_bytes(points)
    n = h.size // pb
    if n == 0 or n & (n - 1) or n * pb != h.size:
        raise PandaGpuError("InvalidLengthErr")
    om = _as_bytes(omega)
    if om.size != FIELD_ELEMENT_LEN:
        raise PandaGpuError("InvalidLengthErr")
    with _Buffers(gm) as b:
        d = b.upload_sync(h)
        ffi.check(b.lib.panda_ec_ntt(curve, d, d, log_2(n), ffi.EC_NTT_INVERSE if inverse else ffi.EC_NTT_FORWARD, _ptr(om), gm.exec_stream.raw), "SchedulingErr")
        return b.download(d, h.size).reshape(n, pb)


def panda_points_gpu_to_affine(gm: PandaGpuManager, points, curve: int = BN254, projective: bool = False) -> np.ndarray:
    """Additive: n result triples X || Y || Z (what the MSM calls return: Jacobian, or homogeneous with projective=True; identity <=>
    Z == 0) -> n affine wire points (canonical, the identity as all-zero bytes) by ONE library call (panda_points_to_affine: one field
    inversion per chunk of points).  Returns (n, point bytes) uint8.  curve is a G1 id."""
    rb, pb = _RESULT_BYTES[curve], _POINT_BYTES[curve]
    h = _as_bytes(points)
    n = h.size // rb
    if n == 0 or n * rb != h.size:
        raise PandaGpuError("InvalidLengthErr")
    with _Buffers(gm) as b:
        d_in = b.upload_sync(h)
        d_out = b.device(n * pb, "CreateContextError")
        ffi.check(b.lib.panda_points_to_affine(curve, d_in, PROJECTIVE if projective else JACOBIAN, d_out, n, gm.exec_stream.raw), "SchedulingErr")
        return b.download(d_out, n * pb).reshape(n, pb)


def panda_points_gpu_scalar_mul(gm: PandaGpuManager, points, scalars, curve: int = BN254, mode: int = ffi.POINTS_MUL_EACH, addend=None) -> np.ndarray:
    """Additive: out[i] = addend[i] + k_i points[i] over n affine G1 points (the MSM's base wire form, identity <=> x == 0) by ONE library
    call (panda_points_scalar_mul).  `scalars` are Montgomery-form Fr elements of 32 B: n of them with mode POINTS_MUL_EACH (k_i =
    scalars[i]), one with POINTS_MUL_ONE (the same k for every point), two with POINTS_MUL_POWERS ((c, s): k_i = c s^i).  The host arrays
    are not changed.  Returns (n, point bytes) uint8: canonical affine points, the identity as all-zero bytes.  curve is a G1 id."""
    pb = _POINT_BYTES[curve]
    h = _as_bytes(points)
    n = h.size // pb
    sc = _as_bytes(scalars)
    want = {ffi.POINTS_MUL_EACH: n, ffi.POINTS_MUL_ONE: 1, ffi.POINTS_MUL_POWERS: 2}.get(mode)
    if n == 0 or n * pb != h.size or want is None or sc.size != want * FIELD_ELEMENT_LEN:
        raise PandaGpuError("InvalidLengthErr")
    add = None if addend is None else _as_bytes(addend)
    if add is not None and add.size != h.size:
        raise PandaGpuError("InvalidLengthErr")
    each = mode == ffi.POINTS_MUL_EACH
    with _Buffers(gm) as b:
        d = b.upload_sync(h)
        d_sc = b.upload_sync(sc) if each else None
        d_add = b.upload_sync(add) if add is not None else None
        ffi.check(b.lib.panda_points_scalar_mul(curve, mode, d, d_sc, None if each else _ptr(sc), d_add, d, n, gm.exec_stream.raw), "SchedulingErr")
        return b.download(d, h.size).reshape(n, pb)


class PandaKzgOpenAll:
    """Additive: KZG proofs of a polynomial at ALL n points of its domain (Feist-Khovratovich) against one SRS.  `srs` holds the n = 2^k
    affine G1 points [tau^i]G (the MSM's base wire form), `omega2` a primitive 2n-th root of unity (one Montgomery-form scalar, 32 B); the
    proofs are for the domain omega^j with omega = omega2^2.  The constructor runs panda_kzg_open_all_setup once and keeps the table of
    2n points and the workspace resident; open(coeffs) is one panda_kzg_open_all call; close() frees the device memory."""

    def __init__(self, gm: PandaGpuManager, srs, omega2, curve: int = BN254):
        self.gm, self.curve, self.pb = gm, curve, _POINT_BYTES[curve]
        h = _as_bytes(srs)
        n = h.size // self.pb
        self.omega2 = _as_bytes(omega2).copy()
        if n < 2 or n & (n - 1) or n * self.pb != h.size or self.omega2.size != FIELD_ELEMENT_LEN:
            raise PandaGpuError("InvalidLengthErr")
        self.n, self.log_n = n, log_2(n)
        work = C.c_size_t(0)
        ffi.check(ffi.load().panda_kzg_open_all_plan(curve, self.log_n, C.byref(work), None), "InvalidLengthErr")
        self.work_bytes = work.value
        with _Buffers(gm) as b:
            resident = [b.device(nbytes, "CreateContextError") for nbytes in (2 * n * self.pb, self.work_bytes, n * self.pb)]
            d_srs = b.upload_sync(h)
            ffi.check(b.lib.panda_kzg_open_all_setup(curve, d_srs, self.log_n, _ptr(self.omega2), resident[0], gm.exec_stream.raw), "SchedulingErr")
            self.d_table, self.d_work, self.d_proofs = [b.keep(d) for d in resident]

    def open(self, coeffs) -> np.ndarray:
        """n Montgomery-form coefficients (32 B each) -> (n, point bytes) uint8: proof j opens the polynomial at omega^j"""
        c = _as_bytes(coeffs)
        if c.size != self.n * FIELD_ELEMENT_LEN or not self.d_table:
            raise PandaGpuError("InvalidLengthErr")
        with _Buffers(self.gm) as b:
            d_c = b.upload_sync(c)
            ffi.check(b.lib.panda_kzg_open_all(self.curve, d_c, self.d_table, self.log_n, _ptr(self.omega2), self.d_work, self.work_bytes, self.d_proofs,
                                               self.gm.exec_stream.raw), "SchedulingErr")
            return b.download(self.d_proofs, self.n * self.pb).reshape(self.n, self.pb)

    def close(self):
        lib = ffi.load()
        for name in ("d_table", "d_work", "d_proofs"):
            d = getattr(self, name)
            if d:
                lib.panda_free(d)
            setattr(self, name, C.c_void_p())


class PandaPoseidon:
    """Additive: Poseidon over a scalar field (0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr) with one parameter set kept resident on the
    device: the permutation, the sponge hash and the Merkle tree of panda_poseidon_*.  `mds` is a (t, t, 8) and `round_constants` a
    (full_rounds + partial_rounds, t, 8) uint32 array of Montgomery-form elements; the width t is the matrix's.  A `tag` is 0 or one
    Montgomery-form element (8 uint32).  Every method is ONE library call on device copies of its arguments; host arrays are not changed.
    close() gives the table back."""

    def __init__(self, gm: PandaGpuManager, round_constants, mds, alpha: int, full_rounds: int, partial_rounds: int, field: int = 0):
        m = np.ascontiguousarray(mds, np.uint32)
        if m.ndim != 3 or m.shape[0] != m.shape[1] or m.shape[2] != 8:
            raise PandaGpuError("InvalidLengthErr")
        self.gm, self.field, self.width = gm, field, m.shape[0]
        rc = np.ascontiguousarray(round_constants, np.uint32).reshape(-1, 8)
        if len(rc) != (full_rounds + partial_rounds) * self.width:
            raise PandaGpuError("InvalidLengthErr")
        params = ffi.PoseidonParams(self.width, alpha, full_rounds, partial_rounds, rc.ctypes.data, m.ctypes.data)
        self.handle = ffi.PandaPoseidon()
        with _Buffers(gm) as b:
            ffi.check(b.lib.panda_poseidon_create(field, C.byref(params), C.byref(self.handle)), "CreateContextError")
            b._own(b.lib.panda_poseidon_destroy, self.handle)
            per = C.c_uint(0)
            ffi.check(b.lib.panda_poseidon_plan(3, 1, C.byref(per), None, None, None, None), "SchedulingErr")
            self.per_workgroup = per.value
            b.keep(self.handle)

    @staticmethod
    def _tag(tag) -> np.ndarray:
        if isinstance(tag, int) and tag == 0:
            return np.zeros(8, np.uint32)
        t = np.ascontiguousarray(tag, np.uint32).reshape(-1)
        if t.size != 8:
            raise PandaGpuError("InvalidLengthErr")
        return t

    def _live(self):
        if not self.handle.handle:
            raise PandaGpuError("SchedulingErr")

    def permute(self, states) -> np.ndarray:
        """(n, t, 8) states -> (n, t, 8) permuted states"""
        s = np.ascontiguousarray(states, np.uint32)
        self._live()
        if s.ndim != 3 or s.shape[0] == 0 or s.shape[1:] != (self.width, 8):
            raise PandaGpuError("InvalidLengthErr")
        with _Buffers(self.gm) as b:
            d, _, _ = b.upload([s.reshape(-1, 8)])
            ffi.check(b.lib.panda_poseidon_permute(self.handle, d, d, s.shape[0], self.gm.exec_stream.raw), "SchedulingErr")
            return b.read(np.empty(s.shape, np.uint32), d)

    def _hash(self, data: np.ndarray, n: int, length: int, msg_stride: int, elem_stride: int, tag) -> np.ndarray:
        t = self._tag(tag)
        with _Buffers(self.gm) as b:
            d_in, _, _ = b.upload([data.reshape(-1, 8)])
            d_out = b.device(n * FIELD_ELEMENT_LEN)
            ffi.check(b.lib.panda_poseidon_hash(self.handle, d_in, length, msg_stride, elem_stride, _ptr(t), d_out, n, self.gm.exec_stream.raw), "SchedulingErr")
            return b.read(np.empty((n, 8), np.uint32), d_out)

    def hash(self, messages, tag=0) -> np.ndarray:
        """(n, len, 8): n messages as rows -> (n, 8), the sponge's state[0] after the last chunk"""
        m = np.ascontiguousarray(messages, np.uint32)
        self._live()
        if m.ndim != 3 or m.shape[0] == 0 or m.shape[1] == 0 or m.shape[2] != 8:
            raise PandaGpuError("InvalidLengthErr")
        return self._hash(m, m.shape[0], m.shape[1], m.shape[1], 1, tag)

    def hash_columns(self, columns, tag=0) -> np.ndarray:
        """(len, n, 8): message i is row i across the len column vectors, the layout the batched transforms leave -> (n, 8)"""
        c = np.ascontiguousarray(columns, np.uint32)
        self._live()
        if c.ndim != 3 or c.shape[0] == 0 or c.shape[1] == 0 or c.shape[2] != 8:
            raise PandaGpuError("InvalidLengthErr")
        return self._hash(c, c.shape[1], c.shape[0], 1, c.shape[1], tag)

    def merkle_tree(self, leaves, tag=0):
        """(a^height, 8) leaves, a = t - 1 -> (nodes, root): the (n - 1) / (a - 1) inner nodes level by level from the bottom as an (m, 8)
        array, and the root (8,), which is also the last node"""
        lv = np.ascontiguousarray(leaves, np.uint32)
        self._live()
        a, n, height = self.width - 1, len(lv), 0
        if lv.ndim != 2 or lv.shape[1] != 8 or a < 2 or n < a:
            raise PandaGpuError("InvalidLengthErr")
        while a ** height < n:
            height += 1
        nodes = C.c_uint64(0)
        if a ** height != n or ffi.load().panda_poseidon_plan(self.width, height, None, C.byref(nodes), None, None, None):
            raise PandaGpuError("InvalidLengthErr")
        t, root = self._tag(tag), np.empty(8, np.uint32)
        with _Buffers(self.gm) as b:
            d_leaves, _, _ = b.upload([lv])
            d_nodes = b.device(nodes.value * FIELD_ELEMENT_LEN)
            ffi.check(b.lib.panda_poseidon_merkle_tree(self.handle, d_leaves, height, _ptr(t), d_nodes, _ptr(root), self.gm.exec_stream.raw), "SchedulingErr")
            return b.read(np.empty((nodes.value, 8), np.uint32), d_nodes), root

    def close(self):
        if self.handle.handle:
            ffi.load().panda_poseidon_destroy(self.handle)
        self.handle = ffi.PandaPoseidon()
