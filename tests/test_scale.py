"""The scaling filter on the host (include/wrenc_scale.h, exported as wrenc_gpu_scale_taps) against its restatement in
Python (tests/scale_ref.py), and the --scale argument errors of both command lines, which need no device: the options are
parsed before any context is made."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scale_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
EINVAL = -1


@pytest.mark.parametrize("n_in,n_out", scale_ref.AXIS_PAIRS, ids=["%d-%d" % p for p in scale_ref.AXIS_PAIRS])
def test_taps_equal_the_python_taps(built, n_in, n_out):
    """First index, count and coefficients of every output index; every set sums to 4096 and holds at most 16."""
    from wrenc_amd import gpu
    for o in range(n_out):
        first, coef = gpu.scale_taps(n_in, n_out, o)
        want_first, want = scale_ref.taps(n_in, n_out, o)
        assert (first, coef) == (want_first, want), o
        assert sum(coef) == scale_ref.UNITY and 1 <= len(coef) <= 16, o


def test_equal_sizes_give_the_single_tap(built):
    from wrenc_amd import gpu
    for n in (1, 16, 17, 100, 3840, 16384):
        for o in sorted({0, n // 2, n - 1}):
            assert gpu.scale_taps(n, n, o) == (o, [scale_ref.UNITY]), (n, o)
    x = np.random.default_rng(3).integers(0, 256, (18, 22)).astype(np.uint8)
    assert np.array_equal(scale_ref.scale_plane(x, 22, 18), x)


def test_refusals(built):
    from wrenc_amd import gpu
    gpu.scale_taps(64, 16, 15)         # the limits themselves are served
    gpu.scale_taps(16, 64, 63)
    for n_in, n_out, o in ((4 * 16 + 2, 16, 0), (16, 4 * 16 + 2, 0), (0, 16, 0), (16, 0, 0), (0, 0, 0), (16, 16, 16), (16, 16, -1),
                           (16386, 16386, 0)):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.scale_taps(n_in, n_out, o)
        assert e.value.code == EINVAL, (n_in, n_out, o)


def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + args, cwd=ROOT, capture_output=True, timeout=120)


@pytest.mark.parametrize("front", ["native", "python"])
def test_scale_argument_errors(built, front, tmp_path):
    """Status 0 and the error: prefix, as the other option errors; nothing is opened or created before them."""
    base = ["-i", str(tmp_path / "missing.yuv"), "-o", str(tmp_path / "out.vvc"), "--num-pictures", "1", "--qp", "32", "--scale"]
    for size in ("71x50", "70x51", "14x50", "70x14"):
        r = _run(front, base + ["--input-size", size, "--output-size", "64x32"])
        assert r.returncode == 0 and b"error: with --scale, input-size must be even and at least 16x16" in r.stderr, (size, r.stderr)
    for src, dst, pad in (("258x64", "64x64", []), ("64x258", "64x64", []), ("16x64", "96x64", []), ("64x16", "64x96", []),
                          ("140x50", "34x30", ["--pad"])):
        r = _run(front, base + pad + ["--input-size", src, "--output-size", dst])
        assert r.returncode == 0 and b"error: with --scale, input-size and output-size must be within a factor of 4" in r.stderr, (src, dst, r.stderr)
    assert not (tmp_path / "out.vvc").exists()
