"""The few HIP runtime calls the denoiser's tests and tools need around the C-ABI — device buffers for hiprz_denoise_image, events on
the context's stream — through ctypes on the very libamdhip64 that libhiprz.so is linked against (no second HIP user in the process)."""
import ctypes as C

import numpy as np

from . import _lib

_rt = None


def runtime():
    global _rt
    if _rt is None:
        # looked up through libhiprz.so's own handle: dlsym searches a library's dependencies, so these are the functions of the
        # runtime the library itself calls, whichever other copies of libamdhip64 the process has mapped (torch ships one)
        _lib.load()
        _rt = C.CDLL(_lib.LIB_PATH)
        _rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _rt.hipFree.argtypes = [C.c_void_p]
        _rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        _rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        _rt.hipEventSynchronize.argtypes = [C.c_void_p]
        _rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        _rt.hipEventDestroy.argtypes = [C.c_void_p]
    return _rt


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with hipError {rc}")


class DeviceBuffer:
    """nbytes of device memory on the current device; upload / download are synchronous copies of numpy arrays"""

    def __init__(self, nbytes):
        self.nbytes, self.ptr = int(nbytes), C.c_void_p()
        _check(runtime().hipMalloc(C.byref(self.ptr), max(self.nbytes, 1)), "hipMalloc")

    @classmethod
    def of(cls, array):
        array = np.ascontiguousarray(array)
        buf = cls(array.nbytes)
        _check(runtime().hipMemcpy(buf.ptr, array.ctypes.data, array.nbytes, 1), "hipMemcpy (host to device)")
        return buf

    def download(self, shape, dtype):
        out = np.zeros(shape, dtype)
        assert out.nbytes <= self.nbytes
        _check(runtime().hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2), "hipMemcpy (device to host)")
        return out

    def free(self):
        if self.ptr:
            runtime().hipFree(self.ptr)
            self.ptr = C.c_void_p()


class Event:
    def __init__(self):
        self.handle = C.c_void_p()
        _check(runtime().hipEventCreate(C.byref(self.handle)), "hipEventCreate")

    def record(self, stream):
        _check(runtime().hipEventRecord(self.handle, stream), "hipEventRecord")

    def ms_since(self, earlier):
        _check(runtime().hipEventSynchronize(self.handle), "hipEventSynchronize")
        ms = C.c_float()
        _check(runtime().hipEventElapsedTime(C.byref(ms), earlier.handle, self.handle), "hipEventElapsedTime")
        return ms.value

    def destroy(self):
        runtime().hipEventDestroy(self.handle)
