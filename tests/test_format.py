"""The source formats on the host (include/wrenc_format.h, exported as wrenc_gpu_format_from_name, _format_name and
_format_layout) against their restatement in Python (tests/format_ref.py), and the --input-format argument error of both
command lines, which needs no device: the options are parsed before any context is made."""
import os
import subprocess
import sys

import numpy as np
import pytest

import format_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
EINVAL = -1
SIZES = [(64, 64), (70, 50), (34, 30), (3840, 2160)]


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_layout_equals_the_python_layout(built, w, h):
    from wrenc_amd import gpu
    for fmt in range(6):
        got = gpu.format_layout(fmt, w, h)
        assert got == format_ref.layout(fmt, w, h), fmt
        assert gpu.format_layout(format_ref.NAMES[fmt], w, h) == got
        # ... which is how pack()'s planes lie in a file
        raw = format_ref.picture("zeros", fmt, w, h)
        assert [p.shape[0] for p in raw] == got["rows"] and [p.shape[1] * p.itemsize for p in raw] == got["row_bytes"], fmt
        assert sum(p.nbytes for p in raw) == got["frame_bytes"], fmt


def test_a_2160p_frame_in_bytes(built):
    from wrenc_amd import gpu
    n = 3840 * 2160
    want = {"yuv420p": n * 3 // 2, "nv12": n * 3 // 2, "yuv420p10le": n * 3, "p010le": n * 3, "yuv422p": n * 2, "yuv422p10le": n * 4}
    for name, size in want.items():
        assert gpu.format_layout(name, 3840, 2160)["frame_bytes"] == size, name


def test_names_round_trip(built):
    from wrenc_amd import gpu
    for fmt, name in enumerate(format_ref.NAMES):
        assert gpu.format_from_name(name) == fmt and gpu.format_name(fmt) == name
    for fmt in (-1, 6, 100):
        assert gpu.format_name(fmt) is None
    for name in ("", "bogus", "YUV420P", "yuv420p ", "yuv420p10", "p010", None):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.format_from_name(name)
        assert e.value.code == EINVAL, name


def test_layout_refusals(built):
    from wrenc_amd import gpu
    gpu.format_layout(5, 16, 16)                       # the smallest frame is served
    for fmt, w, h in ((-1, 64, 64), (6, 64, 64), (0, 65, 64), (2, 64, 63), (1, 14, 64), (4, 64, 14), (3, 0, 0), (5, -64, 64)):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.format_layout(fmt, w, h)
        assert e.value.code == EINVAL, (fmt, w, h)
    lib = gpu.load_library()
    assert lib.wrenc_gpu_format_layout(0, 64, 64, None) == EINVAL      # a null pointer


def test_the_reference_pictures_cover_what_they_claim():
    """all10 at 64x64 holds every value in every plane; its 4:2:2 pairs hold both parities of a + b and both extremes; pack()
    puts junk where the definition does not read, and convert() does not see it."""
    for fmt in format_ref.FORMATS:
        t = format_ref.top(fmt)
        y, cb, cr = format_ref.samples("all10", fmt, 64, 64)
        for p in (y, cb, cr):
            assert np.array_equal(np.unique(p), np.arange(t + 1)), fmt
        if format_ref.is422(fmt):
            for c in (cb, cr):
                pair = set(zip(c[0::2].ravel().tolist(), c[1::2].ravel().tolist()))
                assert (0, 0) in pair and (t, t) in pair and {(a + b) & 1 for a, b in pair} == {0, 1}, fmt
        raw = format_ref.pack(fmt, y, cb, cr, np.random.default_rng(5))
        if fmt == format_ref.P010LE:
            assert all(len(np.unique(p & 63)) == 64 for p in raw)
        elif format_ref.is16(fmt):
            assert all(int(p.max()) > 1023 for p in raw)
        else:                                          # 8-bit 4:2:0 and luma: the byte itself
            clean = format_ref.pack(fmt, y, cb, cr, np.random.default_rng(6))
            assert all(np.array_equal(a, b) for a, b in zip(raw, clean))
    # the definition by hand, a word at a time
    word = np.array([[0, 1, 2, 5, 6, 1021, 1022, 1023, 1024, 65535]], np.uint16)
    assert format_ref._sample(format_ref.YUV420P10LE, word).tolist() == [[0, 0, 1, 1, 2, 255, 255, 255, 255, 255]]
    assert format_ref._sample(format_ref.P010LE, word << 6 | 63).tolist()[0][:8] == [0, 0, 1, 1, 2, 255, 255, 255]
    two = np.array([[0, 1, 1023, 1023, 3], [0, 2, 1023, 1020, 65535]], np.uint16)
    assert format_ref._halve(format_ref.YUV422P10LE, two).tolist() == [[0, 0, 255, 255, 128]]
    assert format_ref._halve(format_ref.YUV422P, np.array([[0, 1, 255, 254], [0, 2, 255, 255]], np.uint8)).tolist() == [[0, 2, 255, 255]]


def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + args, cwd=ROOT, capture_output=True, timeout=120)


@pytest.mark.parametrize("front", ["native", "python"])
def test_input_format_argument_error(built, front, tmp_path):
    """Status 0 and the error: prefix, as the other option errors; nothing is opened or created before it."""
    base = ["-i", str(tmp_path / "missing.yuv"), "-o", str(tmp_path / "out.vvc"), "--num-pictures", "1", "--qp", "32",
            "--input-size", "64x64", "--output-size", "64x64"]
    for name in ("bogus", "yuv444p", ""):
        r = _run(front, base + ["--input-format", name])
        assert r.returncode == 0 and b"error: Invalid input-format: " + name.encode() in r.stderr, (name, r.stderr)
    r = _run(front, base + ["--input-format"])
    assert r.returncode == 0 and b"error: option --input-format needs a value" in r.stderr, r.stderr
    r = _run(front, base + ["--input-format", "p010le"])       # a known name gets as far as the input file
    assert r.returncode == 0 and b"error: failed to open input file" in r.stderr, r.stderr
    assert not (tmp_path / "out.vvc").exists()
