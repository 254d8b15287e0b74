"""Device memory for the tests of the device-side node access (tests/test_device_io_gpu.py): hipMalloc, copies and streams through
ctypes on the HIP runtime libpies_hip.so itself is linked to (looked up through the library's own handle), so that pointers and
streams mean the same thing to the library and to the test.  Every buffer carries four sentinel floats before and after its data (and in front of
a data area that is deliberately one float off a 16-byte boundary); get() checks that they are untouched."""
import ctypes as C

import numpy as np

H2D, D2H = 1, 2
SENTINEL = 0xDEADBEEF


class Hip:
    def __init__(self):
        from pies_amd import capi
        # dlsym on the library's own handle searches its dependencies: these are the runtime's functions the library calls,
        # whatever other HIP runtime the process may have mapped besides
        L = self.L = capi.load()
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        for name, args in {"hipMalloc": [C.POINTER(vp), sz], "hipFree": [vp], "hipMemcpy": [vp, vp, sz, i32],
                           "hipMemcpyAsync": [vp, vp, sz, i32, vp], "hipMemsetAsync": [vp, i32, sz, vp],
                           "hipStreamCreate": [C.POINTER(vp)], "hipStreamSynchronize": [vp], "hipStreamDestroy": [vp],
                           "hipHostMalloc": [C.POINTER(vp), sz, C.c_uint], "hipHostFree": [vp], "hipSetDevice": [i32]}.items():
            getattr(L, name).argtypes = args
            getattr(L, name).restype = i32
        self.ok(L.hipSetDevice(0))

    @staticmethod
    def ok(rc):
        assert rc == 0, "HIP error %d" % rc

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.L.hipMalloc(C.byref(p), nbytes))
        return p.value

    def free(self, p):
        self.ok(self.L.hipFree(p))

    def upload(self, dst, a):
        a = np.ascontiguousarray(a)
        self.ok(self.L.hipMemcpy(dst, a.ctypes.data, a.nbytes, H2D))

    def download(self, src, count, dtype=np.uint32):
        out = np.empty(count, dtype)
        self.ok(self.L.hipMemcpy(out.ctypes.data, src, out.nbytes, D2H))  # on the default stream: behind what the library ordered there
        return out


class DevBuf:
    """`count` 4-byte words of device memory at .ptr = a 16-byte aligned address + 4 * offset bytes, sentinels all around"""

    def __init__(self, hip, count, offset=0, fill=None):
        self.hip, self.count, self.lead = hip, count, 4 + offset
        self.total = self.lead + count + 4
        self.base = hip.malloc(4 * self.total)
        assert self.base % 16 == 0
        self.ptr = self.base + 4 * self.lead
        words = np.full(self.total, SENTINEL, np.uint32)
        if fill is not None:
            words[self.lead:self.lead + count] = np.ascontiguousarray(fill).reshape(-1).view(np.uint32)
        hip.upload(self.base, words)

    def get(self, dtype=np.float32):
        words = self.hip.download(self.base, self.total)
        assert (words[:self.lead] == SENTINEL).all() and (words[self.lead + self.count:] == SENTINEL).all(), "sentinel overwritten"
        return words[self.lead:self.lead + self.count].view(dtype)

    def free(self):
        if self.base:
            self.hip.free(self.base)
            self.base = 0
