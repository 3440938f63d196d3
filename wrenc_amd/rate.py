"""ctypes binding of the rate controller (include/wrenc_rate.h, built into libwrenc_host.so): host only, no device."""
import ctypes as C

import numpy as np

from . import bitstream

CHROMA_WEIGHT = 1.0   # WRENC_RATE_CHROMA_WEIGHT
WINDOW = 64           # WRENC_RATE_WINDOW


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("qp_min", C.c_int32), ("qp_max", C.c_int32),
                ("num_pictures", C.c_int64), ("target_bytes", C.c_double), ("header_bytes", C.c_double)]


def _lib():
    lib = bitstream.load_library()
    lib.wrenc_rate_prior.restype = None
    lib.wrenc_rate_prior.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wrenc_rate_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    lib.wrenc_rate_destroy.restype = None
    lib.wrenc_rate_destroy.argtypes = [C.c_void_p]
    lib.wrenc_rate_choose.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.wrenc_rate_report.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def prior():
    """(a, b, s) of bytes ~ a N (C / N)^b 2^(-QP / s)."""
    a, b, s = C.c_double(), C.c_double(), C.c_double()
    _lib().wrenc_rate_prior(C.byref(a), C.byref(b), C.byref(s))
    return a.value, b.value, s.value


class RateError(RuntimeError):
    pass


class Controller:
    def __init__(self, width, height, target_bytes, num_pictures, qp_min=0, qp_max=63, header_bytes=0.0):
        self.lib = _lib()
        self.cfg = Config(width, height, qp_min, qp_max, num_pictures, target_bytes, header_bytes)
        self.rc = C.c_void_p()
        if self.lib.wrenc_rate_create(C.byref(self.cfg), C.byref(self.rc)):
            raise RateError("wrenc_rate_create: bad configuration")

    def choose(self, satd):
        """satd: (n, 3) plane sums of the next n pictures; returns their QPs."""
        satd = np.ascontiguousarray(satd, np.uint64).reshape(-1, 3)
        qp = np.zeros(len(satd), np.int32)
        if self.lib.wrenc_rate_choose(self.rc, len(satd), satd.ctypes.data, qp.ctypes.data):
            raise RateError("wrenc_rate_choose")
        return [int(q) for q in qp]

    def report(self, nbytes):
        nbytes = np.ascontiguousarray(nbytes, np.uint64).reshape(-1)
        if self.lib.wrenc_rate_report(self.rc, len(nbytes), nbytes.ctypes.data):
            raise RateError("wrenc_rate_report: more pictures than are outstanding")

    def close(self):
        if self.rc:
            self.lib.wrenc_rate_destroy(self.rc)
            self.rc = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
