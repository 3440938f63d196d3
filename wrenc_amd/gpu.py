"""ctypes binding of the C ABI in include/wrenc_gpu.h (libwrenc_gpu.so).

This is the Python-side mirror used by tests and bench.py; a C++/Rust host binds
the same symbols.  There is no CPU fallback: if the HIP
library is missing or no gfx950 device is present, creation fails loudly.
"""
import ctypes as C
import os

import numpy as np

# The HIP runtime gives a process 4 hardware queues per device by default; the context uses 4 encode lanes
# plus one copy stream, and the copy stream only overlaps the search if it has a queue of its own.  Must be
# in the environment before the runtime initialises (first HIP call of the process).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WRENC_GPU_LIB", os.path.join(_HERE, "csrc", "libwrenc_gpu.so"))

# Every function of include/wrenc_gpu.h and include/wrenc_gpu_test.h: name -> (restype, argtypes).  load_library() applies
# the table once; nothing else assigns a prototype (tests/test_abi.py holds it against the headers' declarations).
# Pointers are void pointers: callers pass arrays, byref() and addresses alike.
_I, _P, _S, _Z, _LL = C.c_int, C.c_void_p, C.c_char_p, C.c_size_t, C.c_longlong
PROTOTYPES = {
    "wrenc_gpu_default_config": (_I, [_P, _I, _I, _I, _I]),
    "wrenc_gpu_config_extra_params": (_I, [_P, _S]),
    "wrenc_gpu_create": (_I, [_P, _P]),
    "wrenc_gpu_destroy": (None, [_P]),
    "wrenc_gpu_last_error": (_S, [_P]),
    "wrenc_gpu_upload": (_I, [_P, _I, _P, _P, _P, _Z, _Z]),
    "wrenc_gpu_set_visible_size": (_I, [_P, _I, _I]),
    "wrenc_gpu_visible_size": (_I, [_P, _P, _P]),
    "wrenc_gpu_set_source_size": (_I, [_P, _I, _I]),
    "wrenc_gpu_source_size": (_I, [_P, _P, _P]),
    "wrenc_gpu_scale_taps": (_I, [_I, _I, _I, _P, _P, _P]),
    "wrenc_gpu_set_source_format": (_I, [_P, _I]),
    "wrenc_gpu_source_format": (_I, [_P]),
    "wrenc_gpu_upload_planes": (_I, [_P, _I, _P, _P]),
    "wrenc_gpu_format_from_name": (_I, [_S]),
    "wrenc_gpu_format_name": (_S, [_I]),
    "wrenc_gpu_format_layout": (_I, [_I, _I, _I, _P]),
    "wrenc_gpu_set_source_rgb": (_I, [_P, _I, _I, _I]),
    "wrenc_gpu_source_rgb": (_I, [_P, _P, _P, _P]),
    "wrenc_gpu_rgb_from_name": (_I, [_S]),
    "wrenc_gpu_rgb_name": (_S, [_I]),
    "wrenc_gpu_rgb_layout": (_I, [_I, _I, _I, _P]),
    "wrenc_gpu_rgb_coefficients": (_I, [_I, _I, _P]),
    "wrenc_gpu_rgb_convert_host": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "wrenc_gpu_upload_planes_device": (_I, [_P, _I, _P, _P, _P]),
    "wrenc_gpu_encode": (_I, [_P, _I, _I]),
    "wrenc_gpu_set_slot_qp": (_I, [_P, _I, _P]),
    "wrenc_gpu_sync": (_I, [_P]),
    "wrenc_gpu_download": (_I, [_P, _I, _P]),
    "wrenc_gpu_compact_mask_words": (_Z, [_I, _I]),
    "wrenc_gpu_download_compact": (_I, [_P, _I, _I, _P]),
    "wrenc_gpu_expand_levels": (None, [_I, _I, _P, _P, _P, _P, _P]),
    "wrenc_gpu_download_tokens": (_I, [_P, _I, _I, _P, _P, _Z, _P]),
    "wrenc_gpu_download_metrics": (_I, [_P, _I, _I, _P]),
    "wrenc_gpu_download_complexity": (_I, [_P, _I, _I, _P]),
    "wrenc_gpu_download_rate_hist": (_I, [_P, _I, _I, _P]),
    "wrenc_gpu_rate_hist_bin": (_I, [_I]),
    "wrenc_gpu_rate_hist_host": (_I, [_I, _I, _P, _P, _P, _P]),
    "wrenc_gpu_download_dist_curve": (_I, [_P, _I, _I, _P]),
    "wrenc_gpu_dist_curve_host": (_I, [_I, _I, _P, _P, _P, _P]),
    "wrenc_gpu_metrics_values": (None, [_I, _I, _P, _P, _P]),
    "wrenc_gpu_download_hashes": (_I, [_P, _I, _I, _I, _P]),
    "wrenc_gpu_last_hash_ms": (_I, [_P, _P]),
    "wrenc_gpu_download_recon": (_I, [_P, _I, _P, _P, _P]),
    "wrenc_gpu_download_recon_device": (_I, [_P, _I, _P, _P, _P, _P]),
    "wrenc_gpu_recon_from_name": (_I, [_S]),
    "wrenc_gpu_recon_name": (_S, [_I]),
    "wrenc_gpu_recon_layout": (_I, [_I, _I, _I, _P]),
    "wrenc_gpu_recon_coefficients": (_I, [_I, _I, _P]),
    "wrenc_gpu_recon_convert_host": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "wrenc_gpu_alloc_host": (_P, [_P, _Z]),
    "wrenc_gpu_free_host": (None, [_P, _P]),
    "wrenc_gpu_encode_picture": (_I, [_P, _P, _P, _P, _P]),
    "wrenc_gpu_set_schedule": (_I, [_P, _I]),
    "wrenc_gpu_last_schedule": (_I, [_P]),
    "wrenc_gpu_device_info": (_I, [_P, _P, _P]),
    "wrenc_gpu_stats_enable": (_I, [_P, _I]),
    "wrenc_gpu_last_encode_stats": (_I, [_P, _P, _P, _P]),
    "wrenc_gpu_last_encode_kernel_stats": (_I, [_P, _P]),
    "wrenc_gpu_final_pass_mismatches": (_I, [_P, _P]),
    # test hooks on a context's state, and the planner
    "wrenc_gpu_test_download_originals": (_I, [_P, _I, _P, _P, _P]),
    "wrenc_gpu_test_load_record": (_I, [_P, _I, _P]),
    "wrenc_gpu_test_load_recon": (_I, [_P, _I, _P, _P, _P]),
    "wrenc_gpu_test_set_wave_slots": (_I, [_P, _LL]),
    "wrenc_gpu_test_scratch_overflows": (_I, [_P, _P]),
    "wrenc_gpu_test_plan": (_I, [_I, _I, _P, _I, _I, _LL, _I, _P, _P, _I, _P, _I, _P, _I]),
    # include/wrenc_gpu_test.h
    "wrenc_gpu_test_metrics": (_I, [_P, _P, _P, _P, _P]),
    "wrenc_gpu_test_hash": (_I, [_P, _P, _I, _P]),
    "wrenc_gpu_test_head_ranges": (_I, [_P, _P, _P]),
    "wrenc_gpu_test_avail_tab": (_I, [_P, _P]),
    "wrenc_gpu_test_fwd_dct": (_I, [_P, _P, _I, _I, _P]),
    "wrenc_gpu_test_inv_dct": (_I, [_P, _P, _I, _I, _P]),
    "wrenc_gpu_test_dequantize": (_I, [_P, _P, _I, _I, _P]),
    "wrenc_gpu_test_quantize": (_I, [_P, _P, _I, _I, _P, _P]),
    "wrenc_gpu_test_fwd_dct32": (_I, [_P, _P, _I, _P, _I, _I, _P]),
    "wrenc_gpu_test_inv_dct32": (_I, [_P, _P, _I, _P, _I, _I, _P]),
    "wrenc_gpu_test_fwd_dct_nb": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "wrenc_gpu_test_inv_dct_nb": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "wrenc_gpu_test_dequantize_nb": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "wrenc_gpu_test_quantize_nb": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "wrenc_gpu_test_fwd_dct_mfma": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
    "wrenc_gpu_test_inv_dct_mfma": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _P]),
    "wrenc_gpu_test_fwd_dct4_reg": (_I, [_P, _P, _I, _P]),
    "wrenc_gpu_test_inv_dct4_reg": (_I, [_P, _P, _I, _P]),
    "wrenc_gpu_test_quantize_p16": (_I, [_P, _P, _I, _P, _P]),
    "wrenc_gpu_test_quantize_pk": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "wrenc_gpu_test_recon_rows": (_I, [_P, _P, _P, _P, _I, _P, _P]),
    "wrenc_gpu_test_predict": (_I, [_P, _P, _P, _P, _I, _P, _P, _Z]),
    "wrenc_gpu_test_predict_layout": (_I, [_I, _I, _I, _P, _P]),
    "wrenc_gpu_test_const_field": (_I, [_P, _S, _P, _Z]),
}
EXPORTED_SYMBOLS = list(PROTOTYPES)


class Config(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("qp", C.c_int32), ("max_split_depth", C.c_int32),
        ("device", C.c_int32), ("n_slots", C.c_int32),
        ("lv_table", C.c_int64 * 1024), ("dq_table", C.c_int64 * 1024),
        ("lambda_q", C.c_int64), ("lambda_rd", C.c_float), ("lambda_rd_chroma", C.c_float),
        ("header_bits_luma", C.c_int64 * 67 * 4 * 2),
        ("header_bits_chroma", C.c_int64 * 4),
    ]


class Picture(C.Structure):
    _fields_ = [
        ("rec_y", C.c_void_p), ("rec_cb", C.c_void_p), ("rec_cr", C.c_void_p),
        ("lev_y", C.c_void_p), ("lev_cb", C.c_void_p), ("lev_cr", C.c_void_p),
        ("cu_log2_size", C.c_void_p), ("luma_mode", C.c_void_p), ("chroma_mode", C.c_void_p),
        ("ctu_cost", C.c_void_p),
    ]


class Compact(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("payload", C.c_void_p), ("payload_cap", C.c_size_t), ("n_blocks", C.c_size_t),
                ("cu_log2_size", C.c_void_p), ("luma_mode", C.c_void_p), ("chroma_mode", C.c_void_p),
                ("rec_y", C.c_void_p), ("rec_cb", C.c_void_p), ("rec_cr", C.c_void_p)]


class Tokens(C.Structure):
    _fields_ = [("first_page", C.c_void_p), ("cu_log2_size", C.c_void_p), ("luma_mode", C.c_void_p), ("chroma_mode", C.c_void_p),
                ("rec_y", C.c_void_p), ("rec_cb", C.c_void_p), ("rec_cr", C.c_void_p)]


TOKEN_PAGE = 64  # WRENC_GPU_TOKEN_PAGE


class Metrics(C.Structure):
    _fields_ = [("sse", C.c_uint64 * 3), ("ssim_sum", C.c_double * 3), ("ssim_windows", C.c_uint32 * 3)]


HASH_MD5, HASH_CRC, HASH_CHECKSUM = 0, 1, 2   # include/wrenc_hash.h
HASH_TYPES = {"md5": HASH_MD5, "crc": HASH_CRC, "checksum": HASH_CHECKSUM}


class PictureHash(C.Structure):
    """wrenc_picture_hash: Y, Cb, Cr, each the bytes the SEI carries (MD5 16, CRC 2, checksum 4), zeros behind."""
    _fields_ = [("value", (C.c_uint8 * 16) * 3)]

    def values(self, hash_type):
        """The three components' values as bytes of the type's length."""
        n = {HASH_MD5: 16, HASH_CRC: 2, HASH_CHECKSUM: 4}[_hash_id(hash_type)]
        return [bytes(self.value[p])[:n] for p in range(3)]


def _hash_id(hash_type):
    return HASH_TYPES[hash_type] if isinstance(hash_type, str) else int(hash_type)


class Complexity(C.Structure):
    _fields_ = [("satd", C.c_uint64 * 3), ("ctu_satd", C.c_void_p)]


RATE_HIST_BINS, RATE_HIST_TOP_BIN = 64, 56    # include/wrenc_ratecurve.h


class RateHist(C.Structure):
    """wrenc_rate_hist: count[plane][bin], Y, Cb, Cr."""
    _fields_ = [("count", (C.c_uint64 * RATE_HIST_BINS) * 3)]


def _hist_array(hists, n, columns=RATE_HIST_BINS):
    return np.frombuffer(hists, np.uint64).reshape(-1, 3, columns)[:n].copy()


def rate_hist_bin(magnitude):
    """wrenc_gpu_rate_hist_bin (host only): the bin of a coefficient magnitude 0 .. 16,320 (include/wrenc_ratecurve.h);
    WrencGpuError outside."""
    lib = load_library()
    rc = lib.wrenc_gpu_rate_hist_bin(int(magnitude))
    if rc < 0:
        raise WrencGpuError(rc, "rate_hist_bin(%d)" % magnitude)
    return rc


def rate_hist_host(y, cb, cr):
    """wrenc_gpu_rate_hist_host (host only): the rate histogram of a picture by include/wrenc_ratecurve.h itself, a (3, 64)
    uint64 array; WrencGpuError for planes that are not h x w, h/2 x w/2, h/2 x w/2 with w and h multiples of 16."""
    planes = [np.ascontiguousarray(p, np.uint8) for p in (y, cb, cr)]
    h, w = planes[0].shape if planes[0].ndim == 2 else (0, 0)
    if any(p.ndim != 2 for p in planes) or planes[1].shape != (h // 2, w // 2) or planes[2].shape != (h // 2, w // 2):
        raise WrencGpuError(-1, "rate_hist_host: planes of %s" % ([p.shape for p in planes],))
    lib = load_library()
    out = (RateHist * 1)()
    rc = lib.wrenc_gpu_rate_hist_host(w, h, _p(planes[0]), _p(planes[1]), _p(planes[2]), out)
    if rc:
        raise WrencGpuError(rc, "rate_hist_host(%d x %d)" % (w, h))
    return _hist_array(out, 1)[0]


DIST_CURVE_QPS = 64                           # include/wrenc_distcurve.h


class DistCurve(C.Structure):
    """wrenc_dist_curve: sse8[plane][qp], Y, Cb, Cr."""
    _fields_ = [("sse8", (C.c_uint64 * DIST_CURVE_QPS) * 3)]


def dist_curve_host(y, cb, cr):
    """wrenc_gpu_dist_curve_host (host only): the distortion curve of a picture by include/wrenc_distcurve.h itself, a (3, 64)
    uint64 array; WrencGpuError for planes that are not h x w, h/2 x w/2, h/2 x w/2 with w and h multiples of 16."""
    planes = [np.ascontiguousarray(p, np.uint8) for p in (y, cb, cr)]
    h, w = planes[0].shape if planes[0].ndim == 2 else (0, 0)
    if any(p.ndim != 2 for p in planes) or planes[1].shape != (h // 2, w // 2) or planes[2].shape != (h // 2, w // 2):
        raise WrencGpuError(-1, "dist_curve_host: planes of %s" % ([p.shape for p in planes],))
    lib = load_library()
    out = (DistCurve * 1)()
    rc = lib.wrenc_gpu_dist_curve_host(w, h, _p(planes[0]), _p(planes[1]), _p(planes[2]), out)
    if rc:
        raise WrencGpuError(rc, "dist_curve_host(%d x %d)" % (w, h))
    return _hist_array(out, 1, DIST_CURVE_QPS)[0]


class PlanLaunch(C.Structure):
    """wrenc_gpu_plan_launch"""
    _fields_ = [(k, C.c_int32) for k in ("lane", "team", "diag", "r_min", "count", "first", "n", "grid", "group", "qp", "span")]
    _fields_ += [("ctus", C.c_int64)]


class PlanInfo(C.Structure):
    """wrenc_gpu_plan_info"""
    _fields_ = [(k, C.c_int32) for k in ("n_launches", "n_entries", "n_groups", "n_lanes", "n_spans", "schedule", "wpb", "team",
                                         "encode_lanes", "team_below_pct", "team_below_pct_depth3")]


def encode_plan(ctu_cols, ctu_rows, qps, schedule, wave_slots, depth3):
    """wrenc_gpu_test_plan (host only, no device): the launch plan of an encode call as a dict of the info record's fields
    plus "launches" (a list of dicts, the fields of wrenc_gpu_plan_launch), "entries" and "groups" ((qp, n_real) pairs)."""
    lib = load_library()
    q = (C.c_int * len(qps))(*[int(x) for x in qps])
    info = PlanInfo()
    args = (int(ctu_cols), int(ctu_rows), q, len(qps), int(schedule), int(wave_slots), 1 if depth3 else 0, C.byref(info))
    lib.wrenc_gpu_test_plan(*args, None, 0, None, 0, None, 0)       # the sizes (an error where the arguments are refused, below)
    launches = (PlanLaunch * max(1, info.n_launches))()
    entries = (C.c_int * max(1, info.n_entries))()
    groups = (C.c_int * max(2, 2 * info.n_groups))()
    rc = lib.wrenc_gpu_test_plan(*args, launches, info.n_launches, entries, info.n_entries, groups, info.n_groups)
    if rc:
        raise WrencGpuError(rc, "encode_plan(%d x %d CTUs, %d pictures)" % (ctu_cols, ctu_rows, len(qps)))
    out = {k: getattr(info, k) for k, _ in PlanInfo._fields_}
    out["launches"] = [{k: getattr(launches[i], k) for k, _ in PlanLaunch._fields_} for i in range(info.n_launches)]
    out["entries"] = list(entries[:info.n_entries])
    out["groups"] = [(groups[2 * i], groups[2 * i + 1]) for i in range(info.n_groups)]
    return out


def metrics_values(width, height, m):
    """wrenc_gpu_metrics_values (host only): a Metrics record as {"PSNR": {Avg, Y, U, V}, "SSIM": {...}, "_raw": {...}}, the
    shape of metrics.frame_metrics."""
    lib = load_library()
    psnr, ssim = (C.c_double * 4)(), (C.c_double * 4)()
    lib.wrenc_gpu_metrics_values(width, height, C.byref(m), psnr, ssim)
    names = ("Avg", "Y", "U", "V")
    return {"PSNR": dict(zip(names, psnr)), "SSIM": dict(zip(names, ssim)),
            "_raw": {"sse": list(m.sse), "ssim_sum": list(m.ssim_sum), "ssim_windows": list(m.ssim_windows), "bytes": bytes(m)}}


def scale_taps(n_in, n_out, o):
    """wrenc_gpu_scale_taps (host only): (first input index, [coefficients]) of output sample o of one axis n_in -> n_out
    of the scaling filter (include/wrenc_scale.h); WrencGpuError outside the limits."""
    lib = load_library()
    first, n = C.c_int(), C.c_int()
    coef = (C.c_int16 * 17)()
    rc = lib.wrenc_gpu_scale_taps(int(n_in), int(n_out), int(o), C.byref(first), C.byref(n), coef)
    if rc:
        raise WrencGpuError(rc, "scale_taps(%d, %d, %d)" % (n_in, n_out, o))
    return first.value, list(coef[:n.value])


class FormatLayout(C.Structure):
    _fields_ = [("n_planes", C.c_int), ("bytes_per_sample", C.c_int), ("row_bytes", C.c_size_t * 3), ("rows", C.c_size_t * 3),
                ("offset", C.c_size_t * 3), ("frame_bytes", C.c_size_t)]


def format_from_name(name):
    """wrenc_gpu_format_from_name (host only): the id of a source format named as ffmpeg names it (include/wrenc_format.h);
    WrencGpuError for an unknown name."""
    lib = load_library()
    rc = lib.wrenc_gpu_format_from_name(name.encode() if name is not None else None)
    if rc < 0:
        raise WrencGpuError(rc, "format_from_name(%r)" % (name,))
    return rc


def format_name(fmt):
    """wrenc_gpu_format_name (host only): the name of a format id, None for an unknown one."""
    lib = load_library()
    name = lib.wrenc_gpu_format_name(int(fmt))
    return name.decode() if name is not None else None


def _format_id(fmt):
    return format_from_name(fmt) if isinstance(fmt, str) else int(fmt)


def format_layout(fmt, w, h):
    """wrenc_gpu_format_layout (host only): a tightly packed w x h frame of format `fmt` (an id or a name) as it lies in a raw
    file: {"n_planes", "bytes_per_sample", "row_bytes", "rows", "offset" (a list per plane), "frame_bytes"}."""
    lib = load_library()
    out = FormatLayout()
    rc = lib.wrenc_gpu_format_layout(_format_id(fmt), int(w), int(h), C.byref(out))
    if rc:
        raise WrencGpuError(rc, "format_layout(%r, %d, %d)" % (fmt, w, h))
    n = out.n_planes
    return {"n_planes": n, "bytes_per_sample": out.bytes_per_sample, "row_bytes": list(out.row_bytes[:n]), "rows": list(out.rows[:n]),
            "offset": list(out.offset[:n]), "frame_bytes": out.frame_bytes}


RGB_MATRICES = {"bt709": 0, "bt601": 1}   # include/wrenc_rgb.h
RGB_RANGES = {"tv": 0, "pc": 1}


def rgb_from_name(name):
    """wrenc_gpu_rgb_from_name (host only): the id of an RGB layout named as ffmpeg names it (include/wrenc_rgb.h; "rgba" and
    "bgra" are aliases of rgb0 and bgr0); WrencGpuError for an unknown name."""
    lib = load_library()
    rc = lib.wrenc_gpu_rgb_from_name(name.encode() if name is not None else None)
    if rc < 0:
        raise WrencGpuError(rc, "rgb_from_name(%r)" % (name,))
    return rc


def rgb_name(layout):
    """wrenc_gpu_rgb_name (host only): the name of a layout id, None for an unknown one."""
    lib = load_library()
    name = lib.wrenc_gpu_rgb_name(int(layout))
    return name.decode() if name is not None else None


def _rgb_id(layout):
    return rgb_from_name(layout) if isinstance(layout, str) else int(layout)


def _rgb_matrix_id(matrix):
    if isinstance(matrix, str):
        if matrix not in RGB_MATRICES:
            raise WrencGpuError(-1, "unknown matrix %r" % (matrix,))
        return RGB_MATRICES[matrix]
    return int(matrix)


def _rgb_range_id(rng):
    if isinstance(rng, str):
        if rng not in RGB_RANGES:
            raise WrencGpuError(-1, "unknown range %r" % (rng,))
        return RGB_RANGES[rng]
    return int(rng)


def rgb_layout(layout, w, h):
    """wrenc_gpu_rgb_layout (host only): a tightly packed w x h frame of RGB layout `layout` (an id or a name) as it lies in a
    raw file, the dict of format_layout."""
    lib = load_library()
    out = FormatLayout()
    rc = lib.wrenc_gpu_rgb_layout(_rgb_id(layout), int(w), int(h), C.byref(out))
    if rc:
        raise WrencGpuError(rc, "rgb_layout(%r, %d, %d)" % (layout, w, h))
    n = out.n_planes
    return {"n_planes": n, "bytes_per_sample": out.bytes_per_sample, "row_bytes": list(out.row_bytes[:n]), "rows": list(out.rows[:n]),
            "offset": list(out.offset[:n]), "frame_bytes": out.frame_bytes}


def rgb_coefficients(matrix, rng):
    """wrenc_gpu_rgb_coefficients (host only): [yr, yg, yb, br, bg, bb, rr, rg, rb, yoff] of a matrix and a range (ids or names)."""
    lib = load_library()
    out = (C.c_int * 10)()
    rc = lib.wrenc_gpu_rgb_coefficients(_rgb_matrix_id(matrix), _rgb_range_id(rng), out)
    if rc:
        raise WrencGpuError(rc, "rgb_coefficients(%r, %r)" % (matrix, rng))
    return list(out)


def _rgb_planes(planes):
    """One array or a sequence of arrays -> a tuple of 2-D uint8 arrays whose last axis is contiguous."""
    if isinstance(planes, np.ndarray):
        planes = (planes,)
    planes = tuple(np.asarray(a) for a in planes)
    assert len(planes) in (1, 3) and all(a.ndim == 2 and a.dtype == np.uint8 and a.strides[1] == 1 for a in planes)
    return planes


def rgb_convert_host(layout, matrix, rng, w, h, planes):
    """wrenc_gpu_rgb_convert_host (host only): the rules of include/wrenc_rgb.h over a whole w x h picture.  planes: one
    rows x 3w or rows x 4w uint8 array for a packed layout, three arrays G, B, R for gbrp, possibly views into wider arrays.
    Returns (y, cb, cr)."""
    lib = load_library()
    planes = _rgb_planes(planes)
    ptr = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
    stride = (C.c_size_t * 3)(*[a.strides[0] for a in planes])
    w, h = int(w), int(h)
    y = np.zeros((max(h, 0), max(w, 0)), np.uint8)
    cb = np.zeros((max(h, 0) // 2, max(w, 0) // 2), np.uint8)
    cr = np.zeros_like(cb)
    lay = FormatLayout()
    if lib.wrenc_gpu_rgb_layout(_rgb_id(layout), w, h, C.byref(lay)) == 0:   # what the C side will read must be there
        if len(planes) != lay.n_planes or any(a.shape != (h, lay.row_bytes[p]) for p, a in enumerate(planes)):
            raise WrencGpuError(-1, "rgb_convert_host: planes of %s" % ([a.shape for a in planes],))
    rc = lib.wrenc_gpu_rgb_convert_host(_rgb_id(layout), _rgb_matrix_id(matrix), _rgb_range_id(rng), w, h, ptr, stride, _p(y), _p(cb), _p(cr))
    if rc:
        raise WrencGpuError(rc, "rgb_convert_host(%r, %r, %r, %d, %d)" % (layout, matrix, rng, w, h))
    return y, cb, cr


class ReconFormat(C.Structure):
    _fields_ = [("format", C.c_int32), ("matrix", C.c_int32), ("range", C.c_int32)]


def recon_from_name(name):
    """wrenc_gpu_recon_from_name (host only): the id of an output format of the reconstruction (include/wrenc_recon.h: the
    RGB layouts of wrenc_rgb.h with their ids and aliases, then yuv420p and nv12); WrencGpuError for an unknown name."""
    lib = load_library()
    rc = lib.wrenc_gpu_recon_from_name(name.encode() if name is not None else None)
    if rc < 0:
        raise WrencGpuError(rc, "recon_from_name(%r)" % (name,))
    return rc


def recon_name(fmt):
    """wrenc_gpu_recon_name (host only): the name of an output format id, None for an unknown one."""
    lib = load_library()
    name = lib.wrenc_gpu_recon_name(int(fmt))
    return name.decode() if name is not None else None


def _recon_id(fmt):
    return recon_from_name(fmt) if isinstance(fmt, str) else int(fmt)


def recon_layout(fmt, w, h):
    """wrenc_gpu_recon_layout (host only): a tightly packed w x h frame of output format `fmt` (an id or a name), the dict of
    format_layout."""
    lib = load_library()
    out = FormatLayout()
    rc = lib.wrenc_gpu_recon_layout(_recon_id(fmt), int(w), int(h), C.byref(out))
    if rc:
        raise WrencGpuError(rc, "recon_layout(%r, %d, %d)" % (fmt, w, h))
    n = out.n_planes
    return {"n_planes": n, "bytes_per_sample": out.bytes_per_sample, "row_bytes": list(out.row_bytes[:n]), "rows": list(out.rows[:n]),
            "offset": list(out.offset[:n]), "frame_bytes": out.frame_bytes}


def recon_coefficients(matrix, rng):
    """wrenc_gpu_recon_coefficients (host only): [cy, rv, gu, gv, bu, yoff] of a matrix and a range (ids or names)."""
    lib = load_library()
    out = (C.c_int * 6)()
    rc = lib.wrenc_gpu_recon_coefficients(_rgb_matrix_id(matrix), _rgb_range_id(rng), out)
    if rc:
        raise WrencGpuError(rc, "recon_coefficients(%r, %r)" % (matrix, rng))
    return list(out)


def _recon_planes(fmt, w, h, out, what):
    """The planes a recon call fills: fresh arrays of the layout's shapes, or the caller's `out` (2-D uint8 arrays of those
    shapes, possibly views into wider arrays with the last axis contiguous).  Returns (planes, pointer array, stride array)."""
    lay = recon_layout(fmt, w, h)
    shapes = [(lay["rows"][p], lay["row_bytes"][p]) for p in range(lay["n_planes"])]
    if out is None:
        out = [np.zeros(s, np.uint8) for s in shapes]
    else:
        out = [out] if isinstance(out, np.ndarray) else list(out)
        if len(out) != len(shapes) or any(not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.shape != s or a.strides[1] != 1
                                          or not a.flags.writeable for a, s in zip(out, shapes)):
            raise WrencGpuError(-1, "%s: out must be writable uint8 arrays of shapes %s" % (what, shapes))
    ptr = (C.c_void_p * 3)(*[a.ctypes.data for a in out])
    stride = (C.c_size_t * 3)(*[a.strides[0] for a in out])
    return out, ptr, stride


def recon_convert_host(fmt, matrix, rng, w, h, y, cb, cr, out=None):
    """wrenc_gpu_recon_convert_host (host only): the rules of include/wrenc_recon.h over a whole picture, from the visible
    planes y (h x w), cb and cr (h/2 x w/2) to the planes of output format `fmt` as recon_layout numbers them: a list of
    2-D uint8 arrays (rows x row_bytes), fresh ones or `out` filled in place."""
    lib = load_library()
    w, h = int(w), int(h)
    y, cb, cr = (np.ascontiguousarray(a, np.uint8) for a in (y, cb, cr))
    if y.shape != (h, w) or cb.shape != (h // 2, w // 2) or cr.shape != cb.shape:
        raise WrencGpuError(-1, "recon_convert_host: planes of %s" % ([a.shape for a in (y, cb, cr)],))
    planes, ptr, stride = _recon_planes(fmt, w, h, out, "recon_convert_host")
    rc = lib.wrenc_gpu_recon_convert_host(_recon_id(fmt), _rgb_matrix_id(matrix), _rgb_range_id(rng), w, h, _p(y), _p(cb), _p(cr), ptr, stride)
    if rc:
        raise WrencGpuError(rc, "recon_convert_host(%r, %r, %r, %d, %d)" % (fmt, matrix, rng, w, h))
    return planes


class WrencGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("wrenc_gpu error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load_library():
    """Load libwrenc_gpu.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


def default_config(width, height, qp, max_split_depth, device=0, n_slots=1, extra_params=None):
    cfg = Config()
    lib = load_library()
    rc = lib.wrenc_gpu_default_config(C.byref(cfg), width, height, qp, max_split_depth)
    if rc:
        raise WrencGpuError(rc, "default_config")
    if extra_params:
        rc = lib.wrenc_gpu_config_extra_params(C.byref(cfg), extra_params.encode())
        if rc:
            raise WrencGpuError(rc, lib.wrenc_gpu_last_error(None).decode())
    cfg.device = device
    cfg.n_slots = n_slots
    return cfg


def const_field(cfg, name, dtype):
    """wrenc_gpu_test_const_field (host only): member `name` of the constant block the device is given for `cfg`, as a flat
    array of `dtype`; WrencGpuError for a name the block does not have."""
    lib = load_library()
    buf = np.zeros(1 << 16, np.uint8)   # (the largest member, dct, is 8 KiB)
    n = lib.wrenc_gpu_test_const_field(C.byref(cfg), name.encode(), _p(buf), buf.size)
    if n < 0:
        raise WrencGpuError(n, "const_field(%r)" % (name,))
    return buf[:n].view(dtype).copy()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def alloc_picture(width, height):
    return {
        "rec_y": np.zeros((height, width), np.uint8),
        "rec_cb": np.zeros((height // 2, width // 2), np.uint8),
        "rec_cr": np.zeros((height // 2, width // 2), np.uint8),
        "lev_y": np.zeros((height, width), np.int16),
        "lev_cb": np.zeros((height // 2, width // 2), np.int16),
        "lev_cr": np.zeros((height // 2, width // 2), np.int16),
        "cu_log2_size": np.zeros((height // 4, width // 4), np.uint8),
        "luma_mode": np.zeros((height // 4, width // 4), np.uint8),
        "chroma_mode": np.zeros((height // 8, width // 8), np.uint8),
        "ctu_cost": np.zeros(((height // 32) * (width // 32),), np.float32),
    }


_PIC_KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode",
             "chroma_mode", "ctu_cost")


class Encoder:
    """One context = one GPU.  Mirrors the picture-granular call surface a C++
    SliceEncoder::encode uses in place of the per-CTU split_ct loop."""

    def __init__(self, width, height, qp=26, max_split_depth=3, device=0, n_slots=1, config=None, extra_params=None,
                 schedule=None, visible=None, source=None, source_format=None,
                 source_rgb=None):
        """width x height: the coded size, whole 32x32 CTUs.  visible=(w, h): the pictures are that size (even, at least
        16x16, the coded size its round-up to multiples of 32): upload takes planes of it, the device replicates their last
        column and row into the margin, and download_metrics reports that rectangle (wrenc_gpu_set_visible_size).
        source=(w, h): the pictures are THAT size and the device resamples them to the visible size (the coded size when
        none is given) in front of everything else (wrenc_gpu_set_source_size).
        source_format: an id or a name of include/wrenc_format.h; the pictures come in that format through upload_planes and
        the device converts them to 8-bit 4:2:0 first of all (wrenc_gpu_set_source_format).
        source_rgb=(layout, matrix, range), ids or names of include/wrenc_rgb.h: the pictures are RGB, come through upload_rgb
        and are converted to Y'CbCr on the device (wrenc_gpu_set_source_rgb); exclusive with a non-zero source_format."""
        self.lib = load_library()
        self.cfg = config if config is not None else default_config(width, height, qp, max_split_depth,
                                                                     device, n_slots, extra_params)
        self.extra_params = extra_params
        self._qcfg = {}
        self.width, self.height = self.cfg.width, self.cfg.height
        self.ctx = C.c_void_p()
        rc = self.lib.wrenc_gpu_create(C.byref(self.cfg), C.byref(self.ctx))
        if rc:
            raise WrencGpuError(rc, self.lib.wrenc_gpu_last_error(None).decode())
        self._keep = {}
        self._pinned = []
        self.vis_width, self.vis_height = self.width, self.height
        self.src_width, self.src_height = self.width, self.height
        if schedule is not None:
            self.set_schedule(schedule)
        if visible is not None:
            try:
                self.set_visible_size(*visible)
            except WrencGpuError:
                self.close()
                raise
        if source is not None:
            try:
                self.set_source_size(*source)
            except WrencGpuError:
                self.close()
                raise
        if source_format is not None:
            try:
                self.set_source_format(source_format)
            except WrencGpuError:
                self.close()
                raise
        if source_rgb is not None:
            try:
                self.set_source_rgb(*((source_rgb,) if isinstance(source_rgb, (str, int)) else source_rgb))
            except WrencGpuError:
                self.close()
                raise

    def _check(self, rc):
        if rc:
            raise WrencGpuError(rc, self.lib.wrenc_gpu_last_error(self.ctx).decode())

    def close(self):
        if self.ctx:
            for ptr in self._pinned:
                self.lib.wrenc_gpu_free_host(self.ctx, ptr)
            self._pinned = []
            self.lib.wrenc_gpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, slot, y, cb, cr):
        y = np.ascontiguousarray(y, np.uint8)
        cb = np.ascontiguousarray(cb, np.uint8)
        cr = np.ascontiguousarray(cr, np.uint8)
        assert y.shape == (self.src_height, self.src_width)
        assert cb.shape == cr.shape == (self.src_height // 2, self.src_width // 2)
        self._keep[slot] = (y, cb, cr)  # host buffers must outlive the async copy
        self._check(self.lib.wrenc_gpu_upload(self.ctx, slot, _p(y), _p(cb), _p(cr), self.src_width, self.src_width // 2))

    def upload_strided(self, slot, y, cb, cr):
        """upload of planes that are views into wider arrays (last axis contiguous): their row strides go to the C ABI."""
        planes = [np.asarray(a) for a in (y, cb, cr)]
        assert all(a.dtype == np.uint8 and a.strides[1] == 1 for a in planes)
        assert planes[0].shape == (self.src_height, self.src_width) and planes[1].strides[0] == planes[2].strides[0]
        assert planes[1].shape == planes[2].shape == (self.src_height // 2, self.src_width // 2)
        self._keep[slot] = tuple(planes)
        self._check(self.lib.wrenc_gpu_upload(self.ctx, slot, _p(planes[0]), _p(planes[1]), _p(planes[2]),
                                              planes[0].strides[0], planes[1].strides[0]))

    def set_source_format(self, fmt):
        """wrenc_gpu_set_source_format (an id or a name): before the first upload; 0 / "yuv420p" restores the plain behaviour."""
        self._check(self.lib.wrenc_gpu_set_source_format(self.ctx, _format_id(fmt)))

    def source_format(self):
        return self.lib.wrenc_gpu_source_format(self.ctx)

    def upload_planes(self, slot, planes):
        """wrenc_gpu_upload_planes: the planes of the context's source format at its source size, numpy uint8 / uint16 arrays
        (rows x samples; an interleaved CbCr plane rows x 2 * pairs), possibly views into wider arrays (last axis
        contiguous): their own row strides go to the C ABI."""
        planes = tuple(np.asarray(a) for a in planes)
        assert 2 <= len(planes) <= 3 and all(a.ndim == 2 and a.dtype in (np.uint8, np.uint16) and a.strides[1] == a.itemsize for a in planes)
        self._keep[slot] = planes  # host buffers must outlive the async copy
        ptr = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
        stride = (C.c_size_t * 3)(*[a.strides[0] for a in planes])
        self._check(self.lib.wrenc_gpu_upload_planes(self.ctx, slot, ptr, stride))

    def set_source_rgb(self, layout, matrix="bt709", rng="tv"):
        """wrenc_gpu_set_source_rgb (ids or names of include/wrenc_rgb.h): before the first upload; the pictures come as RGB
        through upload_rgb (or upload_device) and the device converts them to 8-bit 4:2:0 first of all.  layout None or -1
        puts the context back."""
        if layout is None or (not isinstance(layout, str) and int(layout) == -1):
            self._check(self.lib.wrenc_gpu_set_source_rgb(self.ctx, -1, 0, 0))
        else:
            self._check(self.lib.wrenc_gpu_set_source_rgb(self.ctx, _rgb_id(layout), _rgb_matrix_id(matrix), _rgb_range_id(rng)))

    def source_rgb(self):
        """wrenc_gpu_source_rgb: (layout, matrix, range) as ids; layout -1 when no RGB source is set."""
        out = [C.c_int(), C.c_int(), C.c_int()]
        self._check(self.lib.wrenc_gpu_source_rgb(self.ctx, *[C.byref(v) for v in out]))
        return tuple(v.value for v in out)

    def upload_rgb(self, slot, planes):
        """wrenc_gpu_upload_planes on a context with an RGB source: one rows x 3w (rgb24, bgr24) or rows x 4w (rgb0, bgr0)
        uint8 array, or three arrays G, B, R (gbrp), at the source size; views into wider arrays (last axis contiguous) give
        their own row strides to the C ABI."""
        planes = _rgb_planes(planes)
        self._keep[slot] = planes  # host buffers must outlive the async copy
        ptr = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
        stride = (C.c_size_t * 3)(*[a.strides[0] for a in planes])
        self._check(self.lib.wrenc_gpu_upload_planes(self.ctx, slot, ptr, stride))

    def upload_device(self, slot, pointers, strides, stream=0):
        """wrenc_gpu_upload_planes_device: the planes of the context's source kind as DEVICE addresses (plain integers, one to
        three) with their row strides in bytes; stream: the hipStream_t (an integer; 0 the null stream) that wrote them and
        may overwrite them right behind this call.  No host wait; the planes are copied."""
        pointers = [int(p) if p else None for p in pointers]
        strides = [int(s) for s in strides]
        assert 1 <= len(pointers) <= 3 and len(strides) == len(pointers)
        ptr = (C.c_void_p * 3)(*pointers)
        stride = (C.c_size_t * 3)(*strides)
        self._check(self.lib.wrenc_gpu_upload_planes_device(self.ctx, slot, ptr, stride, C.c_void_p(int(stream) if stream else None)))

    def set_visible_size(self, vis_w, vis_h):
        """wrenc_gpu_set_visible_size: before the first upload; the coded size itself restores the plain behaviour."""
        self._check(self.lib.wrenc_gpu_set_visible_size(self.ctx, int(vis_w), int(vis_h)))
        self.vis_width, self.vis_height = int(vis_w), int(vis_h)
        self.src_width, self.src_height = self.source_size()

    def set_source_size(self, src_w, src_h):
        """wrenc_gpu_set_source_size: upload takes planes of this size and the device scales them to the visible size; before
        the first upload and after any set_visible_size; the visible size itself restores the plain behaviour."""
        self._check(self.lib.wrenc_gpu_set_source_size(self.ctx, int(src_w), int(src_h)))
        self.src_width, self.src_height = int(src_w), int(src_h)

    def source_size(self):
        w, h = C.c_int(), C.c_int()
        self._check(self.lib.wrenc_gpu_source_size(self.ctx, C.byref(w), C.byref(h)))
        return w.value, h.value

    def visible_size(self):
        w, h = C.c_int(), C.c_int()
        self._check(self.lib.wrenc_gpu_visible_size(self.ctx, C.byref(w), C.byref(h)))
        return w.value, h.value

    def download_originals(self, slot):
        """Test entry: the coded-size original planes (y, cb, cr) the slot holds, margin included."""
        y = np.zeros((self.height, self.width), np.uint8)
        cb = np.zeros((self.height // 2, self.width // 2), np.uint8)
        cr = np.zeros_like(cb)
        self._check(self.lib.wrenc_gpu_test_download_originals(self.ctx, slot, _p(y), _p(cb), _p(cr)))
        return y, cb, cr

    def encode(self, first_slot=0, n_pictures=1):
        self._check(self.lib.wrenc_gpu_encode(self.ctx, first_slot, n_pictures))

    def set_qp(self, slot, qp):
        """Search `slot` at `qp` from the next encode call on (None: the context's QP again).  The per-QP config is
        resolved like the context's, from the encoder's own extra_params (include/wrenc_gpu.h, wrenc_gpu_set_slot_qp)."""
        if qp is None:
            return self.set_slot_config(slot, None)
        qp = int(qp)
        if qp not in self._qcfg:
            self._qcfg[qp] = default_config(self.width, self.height, qp, self.cfg.max_split_depth, self.cfg.device,
                                            self.cfg.n_slots, self.extra_params)
        self.set_slot_config(slot, self._qcfg[qp])

    def set_slot_config(self, slot, qcfg):
        """wrenc_gpu_set_slot_qp with a config of the caller's (None: the context's)."""
        self._check(self.lib.wrenc_gpu_set_slot_qp(self.ctx, slot, C.addressof(qcfg) if qcfg is not None else None))

    def sync(self):
        self._check(self.lib.wrenc_gpu_sync(self.ctx))

    def download_compact(self, first_slot, n, payload_cap=None):
        """The compact read-back of n slots (include/wrenc_gpu.h): per picture (mask, payload[:n_blocks], maps dict)."""
        w, h = self.width, self.height
        words = self.lib.wrenc_gpu_compact_mask_words(w, h)
        blocks = (w // 4) * (h // 4) * 3 // 2
        cap = blocks if payload_cap is None else payload_cap
        outs = (Compact * n)()
        keep = []
        for k in range(n):
            mask = np.zeros(words, np.uint32)
            pay = np.zeros((max(cap, 1), 16), np.int16)
            maps = {"cu_log2_size": np.zeros((h // 4, w // 4), np.uint8), "luma_mode": np.zeros((h // 4, w // 4), np.uint8),
                    "chroma_mode": np.zeros((h // 8, w // 8), np.uint8)}
            outs[k].mask, outs[k].payload, outs[k].payload_cap = _p(mask).value, _p(pay).value, cap
            for name, arr in maps.items():
                setattr(outs[k], name, _p(arr).value)
            keep.append((mask, pay, maps))
        self._check(self.lib.wrenc_gpu_download_compact(self.ctx, first_slot, n, outs))
        return [(m, p[:outs[k].n_blocks], maps) for k, (m, p, maps) in enumerate(keep)]

    def download_tokens(self, first_slot, n, pool_words=None):
        """The token read-back of n slots (include/wrenc_gpu.h: residual_coding done on the device): (pool, [per picture a
        dict with first_page and the maps]); feed both to bitstream.write_picture_tokens."""
        w, h = self.width, self.height
        grow = pool_words is None
        if pool_words is None:
            pool_words = max(n * w * h * 3 // 2, 1 << 16)   # 6 bytes per luma sample: plenty at QP 27 and above
        pool = np.zeros(pool_words, np.uint32)
        outs = (Tokens * n)()
        pics = []
        for k in range(n):
            d = {"first_page": np.zeros((h // 32) * (w // 32), np.uint32), "cu_log2_size": np.zeros((h // 4, w // 4), np.uint8),
                 "luma_mode": np.zeros((h // 4, w // 4), np.uint8), "chroma_mode": np.zeros((h // 8, w // 8), np.uint8)}
            for name, arr in d.items():
                setattr(outs[k], name, _p(arr).value)
            pics.append(d)
        used = C.c_size_t()
        rc = self.lib.wrenc_gpu_download_tokens(self.ctx, first_slot, n, outs, _p(pool), pool_words, C.byref(used))
        while rc == -3 and grow and pool_words < (1 << 31):     # WRENC_GPU_ENOMEM: a bigger pool (the pass is cheap)
            pool_words *= 4
            pool = np.zeros(pool_words, np.uint32)
            rc = self.lib.wrenc_gpu_download_tokens(self.ctx, first_slot, n, outs, _p(pool), pool_words, C.byref(used))
        self._check(rc)
        self.last_token_words = int(used.value)   # words of the pages in use (they are spread over the whole pool)
        return pool, pics

    def download_metrics(self, first_slot, n):
        """PSNR / SSIM of n encoded slots from the device's sums (include/wrenc_gpu.h, wrenc_gpu_download_metrics): per
        picture {"PSNR": {...}, "SSIM": {...}} as metrics.frame_metrics gives them, the raw sums under "_raw".  With a visible
        size: of that rectangle."""
        outs = (Metrics * max(n, 1))()
        self._check(self.lib.wrenc_gpu_download_metrics(self.ctx, first_slot, n, outs))
        return [metrics_values(self.vis_width, self.vis_height, outs[k]) for k in range(n)]

    def download_complexity(self, first_slot, n, ctu_map=True):
        """Hadamard activity of n slots' originals (include/wrenc_gpu.h, wrenc_gpu_download_complexity), before or after
        their search: per picture {"satd": [Y, Cb, Cr], "ctu_satd": (h/32, w/32) uint32 array or None}."""
        outs = (Complexity * max(n, 1))()
        maps = [np.zeros((self.height // 32, self.width // 32), np.uint32) if ctu_map else None for _ in range(max(n, 0))]
        for k, m in enumerate(maps):
            outs[k].ctu_satd = _p(m).value if m is not None else None
        self._check(self.lib.wrenc_gpu_download_complexity(self.ctx, first_slot, n, outs))
        return [{"satd": [int(v) for v in outs[k].satd], "ctu_satd": maps[k]} for k in range(n)]

    def download_rate_hist(self, first_slot, n):
        """The rate histograms of n slots' originals (include/wrenc_gpu.h, wrenc_gpu_download_rate_hist), before or after
        their search: an (n, 3, 64) uint64 array, count[picture][plane][bin]."""
        outs = (RateHist * max(n, 1))()
        self._check(self.lib.wrenc_gpu_download_rate_hist(self.ctx, first_slot, n, outs))
        return _hist_array(outs, n)

    def download_dist_curve(self, first_slot, n):
        """The distortion curves of n slots' originals (include/wrenc_gpu.h, wrenc_gpu_download_dist_curve), before or after
        their search: an (n, 3, 64) uint64 array, sse8[picture][plane][qp]."""
        outs = (DistCurve * max(n, 1))()
        self._check(self.lib.wrenc_gpu_download_dist_curve(self.ctx, first_slot, n, outs))
        return _hist_array(outs, n, DIST_CURVE_QPS)

    def test_metrics(self, org, rec, maps=False):
        """Test entry: the metrics kernel on two arbitrary pictures (y, cb, cr) of the context's size.  Returns the entry of
        download_metrics; with maps, also the three planes' per-window f32 SSIM values as (h/4 - 1, w/4 - 1) arrays."""
        o = [np.ascontiguousarray(a, np.uint8) for a in org]
        r = [np.ascontiguousarray(a, np.uint8) for a in rec]
        shapes = [(self.height, self.width)] + [(self.height // 2, self.width // 2)] * 2
        assert [a.shape for a in o] == shapes and [a.shape for a in r] == shapes
        out = Metrics()
        wins = [np.zeros((hh // 4 - 1, ww // 4 - 1), np.float32) for hh, ww in shapes] if maps else None
        self._check(self.lib.wrenc_gpu_test_metrics(self.ctx, (C.c_void_p * 3)(*[_p(a).value for a in o]),
                                                    (C.c_void_p * 3)(*[_p(a).value for a in r]), C.byref(out),
                                                    (C.c_void_p * 3)(*[_p(a).value for a in wins]) if maps else None))
        m = metrics_values(self.width, self.height, out)
        return (m, wins) if maps else m

    def download_hashes(self, first_slot, n, hash_type):
        """The decoded picture hash of n encoded slots' reconstruction (include/wrenc_gpu.h, wrenc_gpu_download_hashes):
        per picture a PictureHash; hash_type an id of include/wrenc_hash.h or "md5" / "crc" / "checksum"."""
        outs = (PictureHash * max(n, 1))()
        self._check(self.lib.wrenc_gpu_download_hashes(self.ctx, first_slot, n, _hash_id(hash_type), outs))
        return [outs[k] for k in range(n)]

    def last_hash_ms(self):
        """Device time of the last download_hashes call's kernels (HIP events; after stats_enable())."""
        ms = C.c_float()
        self._check(self.lib.wrenc_gpu_last_hash_ms(self.ctx, C.byref(ms)))
        return ms.value

    def test_hash(self, rec, hash_type):
        """Test entry: the hash kernels on an arbitrary picture (y, cb, cr) of the context's size; a PictureHash."""
        r = [np.ascontiguousarray(a, np.uint8) for a in rec]
        assert [a.shape for a in r] == [(self.height, self.width)] + [(self.height // 2, self.width // 2)] * 2
        out = PictureHash()
        self._check(self.lib.wrenc_gpu_test_hash(self.ctx, (C.c_void_p * 3)(*[_p(a).value for a in r]), _hash_id(hash_type),
                                                 C.byref(out)))
        return out

    def device_info(self):
        """(wavefronts of the search kernel the device holds at once, HIP streams an encode call uses)."""
        slots, lanes = C.c_longlong(), C.c_int()
        self._check(self.lib.wrenc_gpu_device_info(self.ctx, C.byref(slots), C.byref(lanes)))
        return int(slots.value), int(lanes.value)

    def test_load_record(self, slot, rec):
        """Test entry: put a record (maps + level planes) into a slot as if a search had produced it."""
        keep = {k: np.ascontiguousarray(rec[k]) for k in ("lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode")}
        pic = Picture(*[_p(keep[k]) if k in keep else None for k in _PIC_KEYS])
        self._check(self.lib.wrenc_gpu_test_load_record(self.ctx, slot, C.byref(pic)))

    def test_load_recon(self, slot, y, cb, cr):
        """Test entry: put coded-size planes into a slot's reconstruction and mark the slot encoded."""
        y, cb, cr = (np.ascontiguousarray(a, np.uint8) for a in (y, cb, cr))
        assert y.shape == (self.height, self.width) and cb.shape == cr.shape == (self.height // 2, self.width // 2)
        self._check(self.lib.wrenc_gpu_test_load_recon(self.ctx, slot, _p(y), _p(cb), _p(cr)))

    def download_recon(self, slot, fmt="yuv420p", matrix="bt709", rng="tv", out=None):
        """wrenc_gpu_download_recon: the slot's reconstruction at the visible size in output format `fmt` (an id or a name of
        include/wrenc_recon.h), made on the device; matrix and rng (ids or names) are read for the RGB formats only.
        Returns a list of 2-D uint8 arrays (rows x row_bytes) as recon_layout numbers the planes: fresh ones, or `out`
        (views into wider arrays keep their row strides; only the rows' bytes are written)."""
        w, h = self.visible_size()
        planes, ptr, stride = _recon_planes(fmt, w, h, out, "download_recon")
        f = ReconFormat(_recon_id(fmt), _rgb_matrix_id(matrix), _rgb_range_id(rng))
        self._check(self.lib.wrenc_gpu_download_recon(self.ctx, slot, C.byref(f), ptr, stride))
        return planes

    def download_recon_device(self, slot, fmt, pointers, strides, stream=0, matrix="bt709", rng="tv"):
        """wrenc_gpu_download_recon_device: as download_recon, into DEVICE memory: the planes' addresses (plain integers, one
        to three) and row strides in bytes; stream: the hipStream_t (an integer; 0 the null stream) that consumes the
        picture: the copies run behind what it has queued so far, and what it queues next runs behind them.  No host
        wait."""
        pointers = [int(p) if p else None for p in pointers]
        strides = [int(s) for s in strides]
        assert 1 <= len(pointers) <= 3 and len(strides) == len(pointers)
        ptr = (C.c_void_p * 3)(*pointers)
        stride = (C.c_size_t * 3)(*strides)
        f = ReconFormat(_recon_id(fmt), _rgb_matrix_id(matrix), _rgb_range_id(rng))
        self._check(self.lib.wrenc_gpu_download_recon_device(self.ctx, slot, C.byref(f), ptr, stride, C.c_void_p(int(stream) if stream else None)))

    def expand_levels(self, mask, payload):
        """Dense level planes from a compact record (host only)."""
        w, h = self.width, self.height
        ly = np.empty((h, w), np.int16)
        lcb = np.empty((h // 2, w // 2), np.int16)
        lcr = np.empty((h // 2, w // 2), np.int16)
        pay = np.ascontiguousarray(payload, np.int16)
        self.lib.wrenc_gpu_expand_levels(w, h, _p(mask), _p(pay), _p(ly), _p(lcb), _p(lcr))
        return ly, lcb, lcr

    def alloc_host(self, nbytes):
        """A page-locked uint8 array (wrenc_gpu_alloc_host): transfers from / to it run at PCIe rate.  Freed
        by close(); do not use it afterwards."""
        ptr = self.lib.wrenc_gpu_alloc_host(self.ctx, nbytes)
        if not ptr:
            raise WrencGpuError(-3, self.lib.wrenc_gpu_last_error(self.ctx).decode())
        self._pinned.append(ptr)
        return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(ptr))

    def download(self, slot, keys=None, out=None):
        """All planes of the record, or only `keys` (the C ABI skips NULL pointers); `out` = arrays to fill
        instead of fresh ones."""
        if out is None:
            out = alloc_picture(self.width, self.height)
        if keys is not None:
            out = {k: v for k, v in out.items() if k in keys}
        pic = Picture(*[_p(out[k]) if k in out else None for k in _PIC_KEYS])
        self._check(self.lib.wrenc_gpu_download(self.ctx, slot, C.byref(pic)))
        return out

    def encode_picture(self, y, cb, cr):
        self.upload(0, y, cb, cr)
        self.encode(0, 1)
        return self.download(0)

    SCHEDULE_AUTO, SCHEDULE_WAVE, SCHEDULE_TEAM = 0, 1, 2

    def set_schedule(self, schedule):
        """How CTUs map to wavefronts (include/wrenc_gpu.h: wrenc_gpu_schedule); results are the same either way."""
        self._check(self.lib.wrenc_gpu_set_schedule(self.ctx, int(schedule)))

    def last_schedule(self):
        return self.lib.wrenc_gpu_last_schedule(self.ctx)

    def test_set_wave_slots(self, slots):
        """Test entry: the wave-slot count AUTO compares a diagonal with (<= 0: the device's)."""
        self._check(self.lib.wrenc_gpu_test_set_wave_slots(self.ctx, int(slots)))

    def test_scratch_overflows(self):
        """Test entry: workgroups that took a scratch region outside their XCD's partition (0 on MI355X)."""
        n = C.c_longlong(0)
        self._check(self.lib.wrenc_gpu_test_scratch_overflows(self.ctx, C.byref(n)))
        return int(n.value)

    def test_head_ranges(self):
        """Test entry: (counts[4], ranges[4][6]) of wrenc_gpu_test_head_ranges (include/wrenc_gpu.h)."""
        counts = (C.c_int * 4)()
        ranges = (C.c_int * 24)()
        self._check(self.lib.wrenc_gpu_test_head_ranges(self.ctx, counts, ranges))
        return list(counts), np.array(list(ranges), dtype=np.int64).reshape(4, 6)

    def test_avail_tab(self):
        """Test entry: blocks whose table-derived segment availability differs from the reference's rules (must be 0)."""
        n = C.c_int(0)
        self._check(self.lib.wrenc_gpu_test_avail_tab(self.ctx, C.byref(n)))
        return int(n.value)

    def stats_enable(self, on=True):
        """Per-launch timing events (measurement mode, see include/wrenc_gpu.h)."""
        self._check(self.lib.wrenc_gpu_stats_enable(self.ctx, 1 if on else 0))

    def last_encode_stats(self):
        t, k, n = C.c_float(), C.c_float(), C.c_int()
        self._check(self.lib.wrenc_gpu_last_encode_stats(self.ctx, C.byref(t), C.byref(k), C.byref(n)))
        return {"total_ms": t.value, "kernel_ms_sum": k.value, "n_launches": n.value}

    def last_encode_kernel_stats(self):
        """Per kernel of the last encode call: {"wave": {...}, "team": {...}} with ms_sum, launches, ctu_pictures."""
        class KS(C.Structure):
            _fields_ = [("ms_sum", C.c_float), ("launches", C.c_int32), ("ctu_pictures", C.c_int64)]
        out = (KS * 2)()
        self._check(self.lib.wrenc_gpu_last_encode_kernel_stats(self.ctx, out))
        return {n: {"ms_sum": out[i].ms_sum, "launches": out[i].launches, "ctu_pictures": out[i].ctu_pictures}
                for i, n in enumerate(("wave", "team"))}

    def final_pass_mismatches(self):
        v = C.c_longlong()
        self._check(self.lib.wrenc_gpu_final_pass_mismatches(self.ctx, C.byref(v)))
        return v.value

    # ---- building blocks ----
    def _blocks(self, fn, arr):
        arr = np.ascontiguousarray(arr, np.int16)
        count, n, _ = arr.shape
        out = np.zeros_like(arr)
        self._check(fn(self.ctx, _p(arr), int(n).bit_length() - 1, count, _p(out)))
        return out

    def fwd_dct(self, blocks):
        return self._blocks(self.lib.wrenc_gpu_test_fwd_dct, blocks)

    def fwd_dct32(self, blocks, use_mfma, reps=1):
        """(coefficients, kernel ms) of the 32x32 forward transform: v_dot2 code or the i8-MFMA experiment."""
        arr = np.ascontiguousarray(blocks, np.int16)
        assert arr.shape[1:] == (32, 32)
        out = np.zeros_like(arr)
        ms = C.c_float()
        self._check(self.lib.wrenc_gpu_test_fwd_dct32(self.ctx, _p(arr), arr.shape[0], _p(out), int(use_mfma), int(reps),
                                                      C.byref(ms)))
        return out, ms.value

    def inv_dct32(self, blocks, use_mfma, reps=1):
        """(residuals, kernel ms) of the 32x32 inverse transform: v_dot2 code or the i8-MFMA version."""
        arr = np.ascontiguousarray(blocks, np.int16)
        assert arr.shape[1:] == (32, 32)
        out = np.zeros_like(arr)
        ms = C.c_float()
        self._check(self.lib.wrenc_gpu_test_inv_dct32(self.ctx, _p(arr), arr.shape[0], _p(out), int(use_mfma), int(reps),
                                                      C.byref(ms)))
        return out, ms.value

    def inv_dct(self, blocks):
        return self._blocks(self.lib.wrenc_gpu_test_inv_dct, blocks)

    def dequantize(self, blocks):
        return self._blocks(self.lib.wrenc_gpu_test_dequantize, blocks)

    # ---- the same device functions on groups of blocks, as the search calls them ----
    def _groups(self, fn, groups, o1):
        arr = np.ascontiguousarray(groups, np.int16)
        count, nb, n, _ = arr.shape
        out = np.zeros_like(arr)
        self._check(fn(self.ctx, _p(arr), int(n).bit_length() - 1, nb, int(o1), count, _p(out)))
        return out

    def fwd_dct_groups(self, groups, o1=0):
        """groups: (count, nb, n, n) residuals, a group's blocks at r1[o1 ..] of its wavefront; coefficients, same shape."""
        return self._groups(self.lib.wrenc_gpu_test_fwd_dct_nb, groups, o1)

    def inv_dct_groups(self, groups, o1=0):
        return self._groups(self.lib.wrenc_gpu_test_inv_dct_nb, groups, o1)

    def _groups_arm(self, fn, groups, o1, use_mfma, reps):
        arr = np.ascontiguousarray(groups, np.int16)
        count, nb, n, _ = arr.shape
        out = np.zeros_like(arr)
        ms = C.c_float()
        self._check(fn(self.ctx, _p(arr), int(n).bit_length() - 1, nb, int(o1), count, _p(out), int(use_mfma), int(reps),
                       C.byref(ms)))
        return out, ms.value

    def fwd_dct_groups_arm(self, groups, use_mfma, o1=0, reps=1):
        """(coefficients, kernel ms) of groups of 8x8 or 16x16 residual blocks (as fwd_dct_groups): the i8-MFMA version
        the search runs (use_mfma, residuals within +-255) or the v_dot2 templates."""
        return self._groups_arm(self.lib.wrenc_gpu_test_fwd_dct_mfma, groups, o1, use_mfma, reps)

    def inv_dct_groups_arm(self, groups, use_mfma, o1=0, reps=1):
        """(residuals, kernel ms) of groups of 8x8 or 16x16 dequantised blocks, the same two arms."""
        return self._groups_arm(self.lib.wrenc_gpu_test_inv_dct_mfma, groups, o1, use_mfma, reps)

    def dequantize_groups(self, groups, o1=0):
        return self._groups(self.lib.wrenc_gpu_test_dequantize_nb, groups, o1)

    def quantize_groups(self, groups):
        """groups: (count, nb, n, n) coefficients, nb = 1 or 2 (the Cb + Cr pair through quantize_solo's two-block path).
        Returns (levels, summed level cost per group, whether the device function reported a level per group)."""
        arr = np.ascontiguousarray(groups, np.int16)
        count, nb, n, _ = arr.shape
        out = np.zeros_like(arr)
        cost = np.zeros(count, np.int64)
        any_level = np.full(count, -1, np.int32)
        self._check(self.lib.wrenc_gpu_test_quantize_nb(self.ctx, _p(arr), int(n).bit_length() - 1, nb, count, _p(out),
                                                        _p(cost), _p(any_level)))
        assert np.isin(any_level, (0, 1)).all(), "a group's any_level was not written"
        return out, cost, any_level == 1

    def _blocks4_reg(self, fn, blocks):
        arr = np.ascontiguousarray(blocks, np.int16)
        assert arr.shape[1:] == (4, 4)
        out = np.zeros_like(arr)
        self._check(fn(self.ctx, _p(arr), arr.shape[0], _p(out)))
        return out

    def fwd_dct4_reg(self, blocks):
        """4x4 residual blocks through the register transform of the search's 4x4 passes (four blocks per wavefront)."""
        return self._blocks4_reg(self.lib.wrenc_gpu_test_fwd_dct4_reg, blocks)

    def inv_dct4_reg(self, levels):
        """4x4 blocks of levels -> residuals: in-lane dequantisation at the context's QP + the register inverse transform."""
        return self._blocks4_reg(self.lib.wrenc_gpu_test_inv_dct4_reg, levels)

    def recon_rows(self, pred, res, org):
        """Rows of four samples through the search's row reconstruction: pred, org (n, 4) uint8, res (n, 4) int16 (any
        value) -> (reconstruction (n, 4) uint8, squared error per row (n,) uint32)."""
        pred, org = (np.ascontiguousarray(a, np.uint8) for a in (pred, org))
        res = np.ascontiguousarray(res, np.int16)
        assert pred.ndim == 2 and pred.shape[1] == 4 and res.shape == pred.shape == org.shape
        rec = np.zeros_like(pred)
        ssd = np.zeros(pred.shape[0], np.uint32)
        self._check(self.lib.wrenc_gpu_test_recon_rows(self.ctx, _p(pred), _p(res), _p(org), pred.shape[0], _p(rec), _p(ssd)))
        return rec, ssd

    def _predict(self, rec_y, rec_cb, rec_cr, items):
        """wrenc_gpu_test_predict on (n, 5) int32 items: (the output bytes, where each item's start: n + 1 offsets, by
        wrenc_gpu_test_predict_layout -- a bad item is left to the entry itself to refuse)."""
        planes = [np.ascontiguousarray(a, np.uint8) for a in (rec_y, rec_cb, rec_cr)]
        assert planes[0].shape == (self.height, self.width)
        at = np.zeros(len(items) + 1, np.uintp)
        laid = self.lib.wrenc_gpu_test_predict_layout(self.width, self.height, len(items), _p(items), _p(at)) == 0
        out = np.zeros(int(at[-1]) if laid else 1, np.uint8)
        self._check(self.lib.wrenc_gpu_test_predict(self.ctx, _p(planes[0]), _p(planes[1]), _p(planes[2]), len(items),
                                                    _p(items), _p(out), out.size))
        return out, [int(v) for v in at]

    def predict_blocks(self, rec_y, rec_cb, rec_cr, items):
        """items: (n, 5) int32 {x, y, log2 luma size, comp (0 luma, 1 Cb+Cr pair, 2 luma 4x4 through the packed predictor
        of the 4x4 leaf search), mode}; returns the list of predicted blocks (luma: (n, n); pair: (2, n/2, n/2))."""
        items = np.ascontiguousarray(items, np.int32).reshape(-1, 5)
        out, at = self._predict(rec_y, rec_cb, rec_cr, items)
        res = []
        for k, q in enumerate(items):
            n = 1 << int(q[2])
            blk = out[at[k]:at[k + 1]]
            res.append(blk.reshape(2, n // 2, n // 2) if q[3] == 1 else blk.reshape(n, n))
        return res

    NO_MODE = 255   # a pack candidate that is not evaluated (dev_predict.h, kNoMode): rides along as zeros

    @staticmethod
    def pack_modes(modes):
        """The mode word of a pack item of predict_full_blocks: up to three candidate modes (0..66 or NO_MODE)."""
        word = len(modes) << 24
        for j, m in enumerate(modes):
            word |= int(m) << (8 * j)
        return word

    def predict_full_blocks(self, rec_y, rec_cb, rec_cr, items):
        """The search's full-candidate predictor (predict_full: four samples per lane) into each of its destinations, with
        the block's own samples in the planes as originals.  items: (n, 5) int32 {x, y, log2 luma size, kind, mode}:
        kind 8: a luma block into the recon tile; 9: the Cb+Cr pair into the tile (mode 0..66 or a CCLM mode);
        kind 10: the luma blocks of an 8x8 pack of 1..3 candidates into its LDS park, mode = pack_modes([...]);
        kind 11: a 16x16 pack of 1..2 candidates, luma and chroma pair, into its park.
        Returns per item (prediction, residual) as read back from the destination and from the residual buffer: uint8 /
        int16 arrays of shape (n, n) (kind 8), (2, n/2, n/2) (9), (candidates, 8, 8) (10); kind 11: each a pair
        (luma (candidates, 16, 16), chroma (candidates, 2, 8, 8))."""
        items = np.ascontiguousarray(items, np.int32).reshape(-1, 5)
        assert all(int(q[3]) in (8, 9, 10, 11) for q in items)
        out, at = self._predict(rec_y, rec_cb, rec_cr, items)
        res = []
        for k, q in enumerate(items):
            n, kind, nc = 1 << int(q[2]), int(q[3]), int(q[4]) >> 24
            sz = (at[k + 1] - at[k]) // 3                 # prediction bytes, then as many int16 residuals
            pair = []
            for arr in (out[at[k]:at[k] + sz], out[at[k] + sz:at[k + 1]].view(np.int16)):
                if kind == 8:
                    pair.append(arr.reshape(n, n))
                elif kind == 9:
                    pair.append(arr.reshape(2, n // 2, n // 2))
                elif kind == 10:
                    pair.append(arr.reshape(nc, 8, 8))
                else:
                    pair.append((arr[:256 * nc].reshape(nc, 16, 16), arr[256 * nc:].reshape(nc, 2, 8, 8)))
            res.append(tuple(pair))
        return res

    def sad_lists(self, rec_y, rec_cb, rec_cr, items):
        """SAD lists (the search's sad_list_angular) of blocks against their own samples in the planes as originals.
        items: (n, 7) {x, y, log2 luma size, comps (1 luma, 2 chroma pair, 3 both), first mode, entries (<= 16), stride};
        entry j = first mode + j * stride (not evaluated beyond 66: its SAD stays 0).  Returns (n, 16) uint32."""
        it = np.ascontiguousarray(items, np.int32).reshape(-1, 7)
        dev = np.zeros((len(it), 5), np.int32)
        dev[:, :3] = it[:, :3]
        dev[:, 3] = np.where(it[:, 3] == 4, 7, 3 + it[:, 3])   # comps 4: the CCLM list of the chroma pair (lanes 0..2: LT, T, L)
        dev[:, 4] = np.where(it[:, 3] == 4, 0, it[:, 4] | (it[:, 5] << 8) | (it[:, 6] << 16))
        out, _ = self._predict(rec_y, rec_cb, rec_cr, dev)
        return out.view(np.uint32).reshape(len(it), 16)

    def quantize_p16(self, blocks):
        """4x4 blocks through the packed quantiser of the 4x4 leaf search (four blocks per wavefront)."""
        arr = np.ascontiguousarray(blocks, np.int16)
        count, n, _ = arr.shape
        assert n == 4
        out = np.zeros_like(arr)
        cost = np.zeros(count, np.int64)
        self._check(self.lib.wrenc_gpu_test_quantize_p16(self.ctx, _p(arr), count, _p(out), _p(cost)))
        return out, cost

    def quantize_pk(self, packs, log2n, nc):
        """Packs of nc candidates (each: luma block, then Cb and Cr of half the side) through the packed quantiser of
        the 8x8 / 16x16 leaf searches.  packs: (n_packs, nc * 1.5 * 4^log2n) int16; returns (levels, cost[n_packs, nc, 2])."""
        arr = np.ascontiguousarray(packs, np.int16)
        n_packs = arr.shape[0]
        assert arr.shape[1] == nc * 3 * (1 << (2 * log2n)) // 2
        out = np.zeros_like(arr)
        cost = np.zeros((n_packs, nc, 2), np.int64)
        self._check(self.lib.wrenc_gpu_test_quantize_pk(self.ctx, _p(arr), int(log2n), int(nc), n_packs, _p(out), _p(cost)))
        return out, cost

    def quantize(self, blocks):
        arr = np.ascontiguousarray(blocks, np.int16)
        count, n, _ = arr.shape
        out = np.zeros_like(arr)
        cost = np.zeros(count, np.int64)
        self._check(self.lib.wrenc_gpu_test_quantize(self.ctx, _p(arr), int(n).bit_length() - 1, count,
                                                     _p(out), _p(cost)))
        return out, cost
