"""ctypes binding of the host bitstream writer (include/wrenc_bitstream.h, wrenc_amd/csrc/host).

Turns the record the device search returns (gpu.Encoder.download) into the reference's byte
stream: parameter sets once (main.rs:223-260), then per picture a picture-header NAL and one
IDR slice NAL (main.rs:294-385).  CPU code, as in the reference: CABAC is serial per picture.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "host", "libwrenc_host.so")
EXPORTED_SYMBOLS = ("wrenc_bs_picture_bound", "wrenc_bs_write_parameter_sets", "wrenc_bs_write_picture",
                    "wrenc_bs_write_picture_tokens", "wrenc_bs_last_slice_data_bits")
# per-picture QP (include/wrenc_bitstream_qp.h)
EXPORTED_QP_SYMBOLS = ("wrenc_bs_write_picture_qp", "wrenc_bs_write_picture_tokens_qp")
# pictures of any even size (include/wrenc_bitstream_window.h)
EXPORTED_WINDOW_SYMBOLS = ("wrenc_bs_write_parameter_sets_window",)
# rate control (include/wrenc_rate.h; the Python mirror is wrenc_amd/rate.py)
EXPORTED_RATE_SYMBOLS = ("wrenc_rate_prior", "wrenc_rate_create", "wrenc_rate_destroy", "wrenc_rate_choose", "wrenc_rate_report")
# its buffer model (include/wrenc_rate_vbv.h)
EXPORTED_RATE_VBV_SYMBOLS = ("wrenc_rate_curve", "wrenc_rate_curve_prior", "wrenc_rate_enable_vbv", "wrenc_rate_choose_vbv",
                             "wrenc_rate_vbv_allowance", "wrenc_rate_recode")
# quality controller (include/wrenc_rate_quality.h)
EXPORTED_QUALITY_SYMBOLS = ("wrenc_quality_create", "wrenc_quality_destroy", "wrenc_quality_predict", "wrenc_quality_choose",
                            "wrenc_quality_report", "wrenc_quality_correction", "wrenc_quality_totals", "wrenc_quality_tries")
# decoded picture hash SEI (include/wrenc_bitstream_hash.h)
EXPORTED_HASH_SYMBOLS = ("wrenc_bs_picture_hash", "wrenc_bs_write_hash_sei")

OK, EINVAL, ENOSPC, EDATA = 0, -1, -2, -3
HASH_MD5, HASH_CRC, HASH_CHECKSUM = 0, 1, 2   # include/wrenc_hash.h
HASH_TYPES = {"md5": HASH_MD5, "crc": HASH_CRC, "checksum": HASH_CHECKSUM}
HASH_VALUE_BYTES = {HASH_MD5: 16, HASH_CRC: 2, HASH_CHECKSUM: 4}


class BitstreamError(RuntimeError):
    def __init__(self, code, what):
        RuntimeError.__init__(self, "%s failed with %d (%s)" % (
            what, code, {EINVAL: "bad argument", ENOSPC: "buffer too small", EDATA: "inconsistent record"}.get(code, "?")))
        self.code = code


class _Record(C.Structure):
    _fields_ = [("cu_log2_size", C.c_void_p), ("luma_mode", C.c_void_p), ("chroma_mode", C.c_void_p),
                ("lev_y", C.c_void_p), ("lev_cb", C.c_void_p), ("lev_cr", C.c_void_p)]


class _Tokens(C.Structure):
    _fields_ = [("cu_log2_size", C.c_void_p), ("luma_mode", C.c_void_p), ("chroma_mode", C.c_void_p),
                ("pool", C.c_void_p), ("pool_words", C.c_size_t), ("first_page", C.c_void_p)]


_lib = None


def load_library():
    """The writer has no Python or CPU-oracle fallback: a missing library is an error."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.wrenc_bs_picture_bound.restype = C.c_size_t
        lib.wrenc_bs_picture_bound.argtypes = [C.c_int, C.c_int]
        lib.wrenc_bs_write_parameter_sets.restype = C.c_int
        lib.wrenc_bs_write_parameter_sets.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                      C.POINTER(C.c_size_t)]
        lib.wrenc_bs_write_picture.restype = C.c_int
        lib.wrenc_bs_write_picture.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_Record), C.c_void_p,
                                               C.c_size_t, C.POINTER(C.c_size_t)]
        lib.wrenc_bs_last_slice_data_bits.restype = C.c_longlong
        _lib = lib
    return _lib


def write_parameter_sets(width, height, qp):
    """VPS + SPS + PPS NAL units (bytes)."""
    lib = load_library()
    buf = np.zeros(4096, np.uint8)
    n = C.c_size_t()
    rc = lib.wrenc_bs_write_parameter_sets(width, height, qp, buf.ctypes.data, buf.size, C.byref(n))
    if rc != OK:
        raise BitstreamError(rc, "wrenc_bs_write_parameter_sets")
    return buf[:n.value].tobytes()


def write_parameter_sets_window(coded_w, coded_h, vis_w, vis_h, qp):
    """VPS + SPS + PPS of a vis_w x vis_h picture coded at coded_w x coded_h: the SPS carries the conformance window
    (wrenc_bs_write_parameter_sets_window)."""
    lib = load_library()
    buf = np.zeros(4096, np.uint8)
    n = C.c_size_t()
    lib.wrenc_bs_write_parameter_sets_window.restype = C.c_int
    lib.wrenc_bs_write_parameter_sets_window.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    rc = lib.wrenc_bs_write_parameter_sets_window(coded_w, coded_h, vis_w, vis_h, qp, buf.ctypes.data, buf.size, C.byref(n))
    if rc != OK:
        raise BitstreamError(rc, "wrenc_bs_write_parameter_sets_window")
    return buf[:n.value].tobytes()


def _plane(rec, key, shape, dtype):
    a = np.ascontiguousarray(rec[key], dtype=dtype)
    if a.shape != shape:
        raise ValueError("%s has shape %r, expected %r" % (key, a.shape, shape))
    return a


def _write(name, qps, w, h, poc, arg, struct):
    """Call writer `name` with (w, h, *qps, poc, record) into a buffer that grows to what it reports it needs."""
    lib = load_library()
    fn = getattr(lib, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * (3 + len(qps)) + [C.POINTER(struct), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    args = [w, h] + [int(q) for q in qps] + [int(poc), C.byref(arg)]
    # wrenc_bs_picture_bound is the proven worst case (12 bytes per luma sample); real pictures need a small
    # fraction, and the writer reports the size it needs when the buffer is too small
    cap = min(lib.wrenc_bs_picture_bound(w, h), w * h // 2 + 65536)
    buf = np.empty(cap, np.uint8)
    n = C.c_size_t()
    rc = fn(*args, buf.ctypes.data, cap, C.byref(n))
    if rc == ENOSPC:
        cap = n.value
        buf = np.empty(cap, np.uint8)
        rc = fn(*args, buf.ctypes.data, cap, C.byref(n))
    if rc != OK:
        raise BitstreamError(rc, name)
    return buf[:n.value].tobytes()


def _record(w, h, rec):
    arrs = [_plane(rec, "cu_log2_size", (h // 4, w // 4), np.uint8), _plane(rec, "luma_mode", (h // 4, w // 4), np.uint8),
            _plane(rec, "chroma_mode", (h // 8, w // 8), np.uint8), _plane(rec, "lev_y", (h, w), np.int16),
            _plane(rec, "lev_cb", (h // 2, w // 2), np.int16), _plane(rec, "lev_cr", (h // 2, w // 2), np.int16)]
    return _Record(*[a.ctypes.data for a in arrs]), arrs


def _tokens(w, h, pool, pic):
    pool = np.ascontiguousarray(pool, np.uint32)
    arrs = [_plane(pic, "cu_log2_size", (h // 4, w // 4), np.uint8), _plane(pic, "luma_mode", (h // 4, w // 4), np.uint8),
            _plane(pic, "chroma_mode", (h // 8, w // 8), np.uint8), pool, np.ascontiguousarray(pic["first_page"], np.uint32)]
    return _Tokens(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, pool.ctypes.data, pool.size,
                   arrs[4].ctypes.data), arrs


def write_picture(width, height, qp, poc, rec):
    """Picture header NAL + IDR slice NAL (bytes) of one picture from its search record: a dict with
    cu_log2_size, luma_mode, chroma_mode, lev_y, lev_cb, lev_cr as gpu.Encoder.download returns them."""
    w, h = int(width), int(height)
    r, _keep = _record(w, h, rec)
    return _write("wrenc_bs_write_picture", (qp,), w, h, poc, r, _Record)


def write_picture_qp(width, height, pps_qp, slice_qp, poc, rec):
    """write_picture for a picture searched at slice_qp in a sequence whose parameter sets carry pps_qp
    (include/wrenc_bitstream_qp.h)."""
    w, h = int(width), int(height)
    r, _keep = _record(w, h, rec)
    return _write("wrenc_bs_write_picture_qp", (pps_qp, slice_qp), w, h, poc, r, _Record)


def write_picture_tokens(width, height, qp, poc, pool, pic):
    """The same NAL units from the device's token record (gpu.Encoder.download_tokens: `pool` and one of its per-picture
    dicts): the host runs the CU-level syntax and the arithmetic coder only."""
    w, h = int(width), int(height)
    t, _keep = _tokens(w, h, pool, pic)
    return _write("wrenc_bs_write_picture_tokens", (qp,), w, h, poc, t, _Tokens)


def write_picture_tokens_qp(width, height, pps_qp, slice_qp, poc, pool, pic):
    """write_picture_tokens for a picture searched at slice_qp in a sequence whose parameter sets carry pps_qp."""
    w, h = int(width), int(height)
    t, _keep = _tokens(w, h, pool, pic)
    return _write("wrenc_bs_write_picture_tokens_qp", (pps_qp, slice_qp), w, h, poc, t, _Tokens)


def _hash_id(hash_type):
    return HASH_TYPES[hash_type] if isinstance(hash_type, str) else int(hash_type)


def picture_hash(width, height, hash_type, y, cb, cr):
    """wrenc_bs_picture_hash: the decoded picture hash of planes in host memory (the coded size), as the three components'
    values [Y, Cb, Cr], each the bytes the SEI carries (MD5 16, CRC 2, checksum 4, big-endian).  hash_type: an id of
    include/wrenc_hash.h or "md5" / "crc" / "checksum"."""
    lib = load_library()
    w, h, t = int(width), int(height), _hash_id(hash_type)
    planes = [np.ascontiguousarray(a, np.uint8) for a in (y, cb, cr)]
    if w > 0 and h > 0 and [a.shape for a in planes] != [(h, w), (h // 2, w // 2), (h // 2, w // 2)]:
        raise ValueError("planes of %r do not make a %dx%d picture" % ([a.shape for a in planes], w, h))
    out = (C.c_uint8 * 48)()
    lib.wrenc_bs_picture_hash.restype = C.c_int
    lib.wrenc_bs_picture_hash.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = lib.wrenc_bs_picture_hash(w, h, t, planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, out)
    if rc != OK:
        raise BitstreamError(rc, "wrenc_bs_picture_hash")
    raw = bytes(out)
    assert not any(raw[16 * p + HASH_VALUE_BYTES[t]:16 * p + 16].strip(b"\x00") for p in range(3))
    return [raw[16 * p:16 * p + HASH_VALUE_BYTES[t]] for p in range(3)]


def write_hash_sei(hash_type, values):
    """wrenc_bs_write_hash_sei: the SUFFIX_SEI NAL unit (bytes) that carries the three components' values [Y, Cb, Cr] (as
    picture_hash returns them, or a 48-byte wrenc_picture_hash such as gpu.PictureHash); it goes directly behind the
    picture's slice NAL unit."""
    lib = load_library()
    t = _hash_id(hash_type)
    rec = (C.c_uint8 * 48)()
    if isinstance(values, (list, tuple)):
        for p, v in enumerate(values):
            if len(v) > 16:
                raise ValueError("a component's value has at most 16 bytes")
            rec[16 * p:16 * p + len(v)] = list(v)
    else:
        rec[:] = list(bytes(values))
    lib.wrenc_bs_write_hash_sei.restype = C.c_int
    lib.wrenc_bs_write_hash_sei.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    buf = np.zeros(128, np.uint8)
    n = C.c_size_t()
    rc = lib.wrenc_bs_write_hash_sei(t, rec, buf.ctypes.data, buf.size, C.byref(n))
    if rc != OK:
        raise BitstreamError(rc, "wrenc_bs_write_hash_sei")
    return buf[:n.value].tobytes()


def last_slice_data_bits():
    """CABAC bits of the CTU data of this thread's last write_picture call."""
    return int(load_library().wrenc_bs_last_slice_data_bits())
