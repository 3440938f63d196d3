"""ctypes binding of the rate controller (include/wrenc_rate.h, built into libwrenc_host.so): host only, no device."""
import ctypes as C

import numpy as np

from . import bitstream

CHROMA_WEIGHT = 1.0   # WRENC_RATE_CHROMA_WEIGHT
WINDOW = 64           # WRENC_RATE_WINDOW
# the buffer model's curve: WRENC_RATE_CURVE_DEAD, _TAIL, _BITS0, _BITS1, _CHROMA_WEIGHT; WRENC_RATE_VBV_SAFETY, _DECAY
CURVE_DEAD, CURVE_TAIL, CURVE_BITS0, CURVE_BITS1, CURVE_CHROMA_WEIGHT = 0.7, 0.125, 2.3, 0.87, 0.5
VBV_SAFETY, VBV_DECAY = 0.85, 0.9


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
    lib.wrenc_rate_curve.argtypes = [C.c_void_p, C.c_void_p]
    lib.wrenc_rate_curve_prior.restype = None
    lib.wrenc_rate_curve_prior.argtypes = [C.c_void_p, C.c_void_p]
    lib.wrenc_rate_enable_vbv.argtypes = [C.c_void_p, C.c_double]
    lib.wrenc_rate_choose_vbv.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wrenc_rate_vbv_allowance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wrenc_rate_recode.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p]
    return lib


def prior():
    """(a, b, s) of bytes ~ a N (C / N)^b 2^(-QP / s)."""
    a, b, s = C.c_double(), C.c_double(), C.c_double()
    _lib().wrenc_rate_prior(C.byref(a), C.byref(b), C.byref(s))
    return a.value, b.value, s.value


class RateError(RuntimeError):
    pass


def _hists(hist):
    hist = np.ascontiguousarray(hist, np.uint64)
    if hist.ndim < 2 or hist.shape[-2:] != (3, 64):
        raise RateError("a rate histogram is (3, 64) counts")
    return hist.reshape(-1, 3, 64)


def curve(hist):
    """wrenc_rate_curve: P(q), q = 0 .. 63, of one (3, 64) rate histogram (wrenc_amd.gpu download_rate_hist)."""
    hist = _hists(hist)
    if len(hist) != 1:
        raise RateError("curve: one histogram")
    p = np.zeros(64, np.float64)
    if _lib().wrenc_rate_curve(hist.ctypes.data, p.ctypes.data):
        raise RateError("wrenc_rate_curve")
    return p


def curve_prior():
    """(a, c) of bytes ~ a P(q) + c CTUs."""
    a, c = C.c_double(), C.c_double()
    _lib().wrenc_rate_curve_prior(C.byref(a), C.byref(c))
    return a.value, c.value


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

    # the buffer model
    def enable_vbv(self, bufsize_bits):
        if self.lib.wrenc_rate_enable_vbv(self.rc, float(bufsize_bits)):
            raise RateError("wrenc_rate_enable_vbv: a buffer below one picture's bits or the parameter sets', or pictures already chosen")

    def choose_vbv(self, hist, allowances=False):
        """hist: (n, 3, 64) rate histograms of the next n pictures; returns their QPs (and, asked for, the bits the walk
        expects the bucket to allow each)."""
        hist = _hists(hist)
        qp = np.zeros(len(hist), np.int32)
        allow = np.zeros(len(hist), np.float64)
        if self.lib.wrenc_rate_choose_vbv(self.rc, len(hist), hist.ctypes.data, qp.ctypes.data, allow.ctypes.data):
            raise RateError("wrenc_rate_choose_vbv: no buffer model enabled")
        return ([int(q) for q in qp], allow.tolist()) if allowances else [int(q) for q in qp]

    def vbv_allowance(self):
        """{"allowance", "bufsize", "fullness"} in bits, for the oldest outstanding picture."""
        a, b, f = C.c_double(), C.c_double(), C.c_double()
        if self.lib.wrenc_rate_vbv_allowance(self.rc, C.byref(a), C.byref(b), C.byref(f)):
            raise RateError("wrenc_rate_vbv_allowance: no buffer model enabled")
        return {"allowance": a.value, "bufsize": b.value, "fullness": f.value}

    def recode(self, actual_bytes, allowance_bits):
        """The QP to code the oldest outstanding picture again at."""
        q = C.c_int32()
        if self.lib.wrenc_rate_recode(self.rc, int(actual_bytes), float(allowance_bits), C.byref(q)):
            raise RateError("wrenc_rate_recode")
        return q.value

    def close(self):
        if self.rc:
            self.lib.wrenc_rate_destroy(self.rc)
            self.rc = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the quality controller (include/wrenc_rate_quality.h)
QUALITY_PRIOR, QUALITY_LEARN, QUALITY_MAX_RECODES = -0.9, 0.25, 8


def _quality_lib():
    lib = bitstream.load_library()
    lib.wrenc_quality_create.restype = C.c_void_p
    lib.wrenc_quality_create.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int]
    lib.wrenc_quality_destroy.restype = None
    lib.wrenc_quality_destroy.argtypes = [C.c_void_p]
    lib.wrenc_quality_predict.restype = C.c_double
    lib.wrenc_quality_predict.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.wrenc_quality_choose.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.wrenc_quality_report.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.wrenc_quality_correction.restype = C.c_double
    lib.wrenc_quality_correction.argtypes = [C.c_void_p]
    lib.wrenc_quality_totals.restype = None
    lib.wrenc_quality_totals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wrenc_quality_tries.argtypes = [C.c_void_p, C.c_int]
    return lib


def _curves(curves):
    curves = np.ascontiguousarray(curves, np.uint64)
    if curves.ndim < 2 or curves.shape[-2:] != (3, 64):
        raise RateError("a distortion curve is (3, 64) sums")
    return curves.reshape(-1, 3, 64)


def quality_predict(curve, width, height):
    """wrenc_quality_predict: the luma PSNR one (3, 64) distortion curve (wrenc_amd.gpu download_dist_curve) predicts at
    every QP, uncorrected."""
    curve = _curves(curve)
    if len(curve) != 1:
        raise RateError("quality_predict: one curve")
    lib = _quality_lib()
    return np.array([lib.wrenc_quality_predict(curve.ctypes.data, width, height, q) for q in range(64)])


class QualityController:
    def __init__(self, target_psnr, qp_min=0, qp_max=63, max_recodes=3):
        self.lib = _quality_lib()
        self.q = C.c_void_p(self.lib.wrenc_quality_create(float(target_psnr), qp_min, qp_max, max_recodes))
        if not self.q:
            raise RateError("wrenc_quality_create: bad configuration")

    def choose(self, curves, width, height):
        """curves: (n, 3, 64) distortion curves of the next n pictures, the current batch from now on; returns their QPs."""
        curves = np.zeros((0, 3, 64), np.uint64) if len(curves) == 0 else _curves(curves)
        qp = np.zeros(max(len(curves), 1), np.int32)
        if self.lib.wrenc_quality_choose(self.q, len(curves), curves.ctypes.data, width, height, qp.ctypes.data):
            raise RateError("wrenc_quality_choose")
        return [int(v) for v in qp[:len(curves)]]

    def report(self, picture, qp, sse_y, samples_y):
        """(accepted, qp): the QP of the coding to keep, or the one to code picture `picture` of the batch again at."""
        nxt, acc = C.c_int32(), C.c_int()
        if self.lib.wrenc_quality_report(self.q, picture, qp, int(sse_y), int(samples_y), C.byref(nxt), C.byref(acc)):
            raise RateError("wrenc_quality_report: not a picture of the batch, accepted already, or a QP tried before")
        return bool(acc.value), nxt.value

    @property
    def correction(self):
        return self.lib.wrenc_quality_correction(self.q)

    def totals(self):
        """(reencoded, misses) since the controller was made."""
        r, m = C.c_uint64(), C.c_uint64()
        self.lib.wrenc_quality_totals(self.q, C.byref(r), C.byref(m))
        return r.value, m.value

    def tries(self, picture):
        return self.lib.wrenc_quality_tries(self.q, picture)

    def close(self):
        if self.q:
            self.lib.wrenc_quality_destroy(self.q)
            self.q = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
