"""Device memory for the GPU tests without torch.cuda: ctypes on the libamdhip64.so the library links.

    a = hip_mem.to_device(np_array[, stream])    DeviceArray with __cuda_array_interface__ (what torch-ROCm tensors and CuPy arrays expose)
    a = hip_mem.empty(shape, dtype)
    a.get([stream]) -> np.ndarray                hipMemcpyAsync on `stream` + hipStreamSynchronize of that stream only (stream None: one blocking hipMemcpy)
    a.set(np_array[, stream])
    s = hip_mem.Stream(); s.ptr; s.synchronize()
Test infrastructure only: nothing here computes anything."""
import ctypes as C

import numpy as np

H2D, D2H = 1, 2
_lib = None


class HipError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
        P = C.c_void_p
        for name, args in (("hipMalloc", [C.POINTER(P), C.c_size_t]), ("hipFree", [P]), ("hipMemcpy", [P, P, C.c_size_t, C.c_int]),
                           ("hipMemcpyAsync", [P, P, C.c_size_t, C.c_int, P]), ("hipStreamCreateWithFlags", [C.POINTER(P), C.c_uint]), ("hipStreamDestroy", [P]),
                           ("hipStreamSynchronize", [P]), ("hipMemset", [P, C.c_int, C.c_size_t]), ("hipHostMalloc", [C.POINTER(P), C.c_size_t, C.c_uint]), ("hipHostFree", [P])):
            fn = getattr(_lib, name); fn.argtypes = args; fn.restype = C.c_int
        _lib.hipGetErrorString.restype = C.c_char_p; _lib.hipGetErrorString.argtypes = [C.c_int]
    return _lib


def chk(rc, what):
    if rc != 0:
        raise HipError(f"{what}: {lib().hipGetErrorString(rc).decode()} ({rc})")


class Stream:
    """a non-blocking stream of the test's own (hipStreamNonBlocking: no implicit ordering with the null stream)"""

    def __init__(self):
        self._s = C.c_void_p()
        chk(lib().hipStreamCreateWithFlags(C.byref(self._s), 1), "hipStreamCreateWithFlags")

    @property
    def ptr(self) -> int:
        return int(self._s.value)

    def synchronize(self):
        chk(lib().hipStreamSynchronize(self._s), "hipStreamSynchronize")

    def close(self):
        if self._s:
            lib().hipStreamDestroy(self._s); self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _sp(stream):
    return None if stream is None else C.c_void_p(stream.ptr if isinstance(stream, Stream) else int(stream))


class _Pinned:
    """a page-locked host staging array: hipMemcpyAsync from / to pageable memory would not be asynchronous"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self._p = C.c_void_p()
        chk(lib().hipHostMalloc(C.byref(self._p), max(self.nbytes, 1), 0), "hipHostMalloc")
        self.array = np.frombuffer((C.c_char * max(self.nbytes, 1)).from_address(self._p.value), self.dtype, count=int(np.prod(self.shape, dtype=np.int64))).reshape(self.shape)

    def __del__(self):
        try:
            if self._p:
                self.array = None; lib().hipHostFree(self._p); self._p = C.c_void_p()
        except Exception:
            pass


class DeviceArray:
    """a C-contiguous device array that exposes __cuda_array_interface__ (version 3, strides None)"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(int(x) for x in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self._p = C.c_void_p()
        chk(lib().hipMalloc(C.byref(self._p), max(self.nbytes, 1)), "hipMalloc")
        self._stage = None

    @property
    def ptr(self) -> int:
        return int(self._p.value)

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 3, "strides": None}

    def set(self, host, stream=None):
        host = np.ascontiguousarray(host, self.dtype)
        assert host.shape == self.shape, (host.shape, self.shape)
        if stream is None:
            chk(lib().hipMemcpy(self._p, host.ctypes.data_as(C.c_void_p), self.nbytes, H2D), "hipMemcpy")
        else:
            self._stage = _Pinned(self.shape, self.dtype); self._stage.array[...] = host
            chk(lib().hipMemcpyAsync(self._p, self._stage._p, self.nbytes, H2D, _sp(stream)), "hipMemcpyAsync")
        return self

    def get(self, stream=None) -> np.ndarray:
        if stream is None:
            out = np.empty(self.shape, self.dtype)
            chk(lib().hipMemcpy(out.ctypes.data_as(C.c_void_p), self._p, self.nbytes, D2H), "hipMemcpy")
            return out
        st = _Pinned(self.shape, self.dtype)
        chk(lib().hipMemcpyAsync(st._p, self._p, self.nbytes, D2H, _sp(stream)), "hipMemcpyAsync")
        chk(lib().hipStreamSynchronize(_sp(stream)), "hipStreamSynchronize")
        return st.array.copy()

    def fill_bytes(self, byte: int):
        chk(lib().hipMemset(self._p, byte, self.nbytes), "hipMemset")
        return self

    def free(self):
        if self._p:
            lib().hipFree(self._p); self._p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def empty(shape, dtype) -> DeviceArray:
    return DeviceArray(shape, dtype)


def to_device(host, stream=None) -> DeviceArray:
    host = np.ascontiguousarray(host)
    return DeviceArray(host.shape, host.dtype).set(host, stream)
