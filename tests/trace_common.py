"""What the candidate-level tests share (tests/test_gpu_trace.py, tests/test_gpu_mode_census.py): the diagnostic build
libwrenc_gpu_trace.so in place of the product library, one traced encode, and the comparison of a device trace with the
oracle's."""
import ctypes as C
import os

import numpy as np
import pytest

TRACE_MAX = 1 << 19     # kTraceMax: the records the device's buffer holds


@pytest.fixture()
def trace_gpu(built):
    from wrenc_amd import gpu
    path = os.path.join(os.path.dirname(gpu.LIB_PATH), "libwrenc_gpu_trace.so")
    assert os.path.exists(path), "run __graft_entry__.build() first"
    saved = (gpu._lib, gpu.LIB_PATH)
    gpu._lib, gpu.LIB_PATH = None, path
    try:
        yield gpu
    finally:
        gpu._lib, gpu.LIB_PATH = saved


def gpu_trace(gpu, y, cb, cr, qp, depth, schedule, extra_params=None):
    """One picture through the traced library: (record, {key: set of f32 bit patterns}, records made)."""
    h, w = y.shape
    enc = gpu.Encoder(w, h, qp=qp, max_split_depth=depth, schedule=schedule, extra_params=extra_params)
    fn = enc.lib.wrenc_gpu_trace_read
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    fn(enc.ctx, None, 0)                      # reset
    out = enc.encode_picture(y, cb, cr)
    buf = np.zeros((TRACE_MAX, 8), np.int32)
    n = fn(enc.ctx, buf.ctypes.data_as(C.c_void_p), buf.shape[0])
    enc.close()
    assert 0 < n <= buf.shape[0]
    trace = {}
    for rec in buf[:n].tolist():
        trace.setdefault(tuple(rec[:7]), set()).add(rec[7] & 0xFFFFFFFF)
    return out, trace, n


def assert_trace_matches(gtrace, otrace):
    """Every evaluation of the device exists in the oracle's trace with the same f32 bits, none has two values, all four
    kinds are there, and the device saw most of the oracle's distinct candidates (it skips only re-evaluations)."""
    kinds = set()
    for key, vals in gtrace.items():
        assert len(vals) == 1, ("GPU evaluated %s twice with different results" % (key,))
        assert key in otrace, ("GPU evaluated a candidate the reference never evaluates: %s" % (key,))
        assert vals == otrace[key], ("candidate %s: GPU %s oracle %s" % (key, vals, otrace[key]))
        kinds.add(key[4])
    assert kinds == {0, 1, 2, 3}
    assert len(gtrace) >= 0.9 * len(otrace), (len(gtrace), len(otrace))
