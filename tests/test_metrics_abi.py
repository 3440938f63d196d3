"""The host side of the device metrics (include/wrenc_gpu.h: wrenc_gpu_metrics, wrenc_gpu_metrics_values) and the
--metrics option's argument handling: nothing here needs a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import metrics_ref
from content import content

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
NEW_SYMBOLS = ("wrenc_gpu_download_metrics", "wrenc_gpu_metrics_values", "wrenc_gpu_test_metrics")


def _record(gpu, org, rec):
    m = gpu.Metrics()
    for p in range(3):
        sse, win = metrics_ref.plane_sums(org[p], rec[p])
        m.sse[p], m.ssim_sum[p], m.ssim_windows[p] = sse, float(np.sum(win.astype(np.float64))), win.size
    return m


def test_reference_windows_are_ssim_planes(built):
    """The per-window helper of these tests restates metrics.ssim_plane: its mean is that function's value, bit for bit."""
    from wrenc_amd import metrics
    a, b = content("cclm", 96, 64, 1), content("noise", 96, 64, 2)
    for p in range(3):
        win = metrics_ref.ssim_windows(a[p], b[p])
        assert win.dtype == np.float32
        assert float(np.sum(win.astype(np.float64)) / win.size) == metrics.ssim_plane(a[p], b[p])


@pytest.mark.parametrize("w,h", [(32, 32), (96, 64), (352, 288)])
def test_metrics_values_are_frame_metrics(built, w, h):
    from wrenc_amd import gpu, metrics
    rng = np.random.default_rng(w * 7 + h)
    org = content("cclm", w, h, 3)
    noisy = tuple(np.clip(p.astype(np.int64) + rng.integers(-9, 10, p.shape), 0, 255).astype(np.uint8) for p in org)
    same_chroma = (noisy[0], org[1].copy(), org[2].copy())     # sse == 0 on two planes
    for rec in (noisy, same_chroma, tuple(p.copy() for p in org)):
        m = _record(gpu, org, rec)
        got = gpu.metrics_values(w, h, m)
        want = metrics.frame_metrics(org, rec)
        for k in ("Avg", "Y", "U", "V"):
            g, x = got["PSNR"][k], want["PSNR"][k]
            assert (g == x) if np.isinf(x) else abs(g - x) <= 1e-12 * abs(x), (k, g, x)
        planes = [m.ssim_sum[p] / m.ssim_windows[p] for p in range(3)]
        for p, k in enumerate(("Y", "U", "V")):
            assert got["SSIM"][k] == planes[p]
        assert abs(got["SSIM"]["Avg"] - (4.0 * planes[0] + planes[1] + planes[2]) / 6.0) <= 1e-15
        metrics_ref.check_entry(got, org, rec)
        assert got["_raw"]["sse"] == list(m.sse) and got["_raw"]["ssim_windows"] == list(m.ssim_windows)
    ident = gpu.metrics_values(w, h, _record(gpu, org, org))
    assert all(v == float("inf") for v in ident["PSNR"].values()) and all(v == 1.0 for v in ident["SSIM"].values())


def test_record_layout(built):
    from wrenc_amd import gpu
    assert C.sizeof(gpu.Metrics) == 64                        # 60 bytes of fields, 8-byte alignment
    assert [gpu.Metrics.sse.offset, gpu.Metrics.ssim_sum.offset, gpu.Metrics.ssim_windows.offset] == [0, 24, 48]


def test_new_symbols_are_exported(built):
    from wrenc_amd import gpu
    lib = C.CDLL(gpu.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in gpu.EXPORTED_SYMBOLS
        assert getattr(lib, name)
    header = open(os.path.join(ROOT, "include", "wrenc_gpu.h")).read()
    test_header = open(os.path.join(ROOT, "include", "wrenc_gpu_test.h")).read()     # the test entries' declarations
    assert all(name + "(" in (test_header if "_test_" in name else header) for name in NEW_SYMBOLS)


@pytest.mark.parametrize("front", ["native", "python"])
def test_metrics_option_needs_a_value(built, tmp_path, front):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    out = tmp_path / "o.vvc"
    r = subprocess.run(cmd + ["-i", str(tmp_path / "missing.yuv"), "-o", str(out), "--input-size", "64x64", "--output-size", "64x64",
                              "--num-pictures", "1", "--qp", "32", "--metrics"], cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0 and b"error: option --metrics needs a value" in r.stderr, r.stderr
    assert not out.exists() or out.stat().st_size == 0
