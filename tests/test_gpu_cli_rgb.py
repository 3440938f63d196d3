"""RGB --input-format of the command line (wrenc_amd/csrc/host/wrenc_main.cpp): a sequence of RGB frames, converted on the
device by --colorspace and --range (run A), against the same sequence converted by tests/rgb_ref.py to yuv420p -- and, for
the --scale run, scaled by tests/scale_ref.py -- and coded with the same options but those (run B): the two runs write the
same stream and the same --reconst file."""
import os
import subprocess

import pytest

import format_ref
import rgb_ref
import scale_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
SW, SH, VW, VH, N, QP = 70, 50, 34, 30, 3, 32


def _run(args):
    r = subprocess.run([NATIVE] + args, cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r


def _pair(d, tag, frames_a, option_a, size_a, frames_b, size_b, w, h):
    outs = []
    for name, frames, option, size in (("a", frames_a, option_a, size_a), ("b", frames_b, [], size_b)):
        src, out, rec = (d / ("%s_%s%s" % (tag, name, e)) for e in (".raw", ".vvc", ".yuv"))
        src.write_bytes(b"".join(frames))
        _run(["-i", str(src), "-o", str(out), "-r", str(rec), "--pad", "--num-pictures", str(N), "--qp", str(QP), "--max-split-depth", "2"]
             + size + option)
        outs.append((out.read_bytes(), rec.read_bytes()))
    (sa, ra), (sb, rb) = outs
    assert sa == sb and len(sa) > 200
    assert ra == rb and len(ra) == N * w * h * 3 // 2          # --reconst stays 8-bit 4:2:0 of --output-size


def test_rgb24_input_against_the_converted_sequence(built, tmp_path):
    lay, matrix, rng = rgb_ref.RGB24, rgb_ref.BT601, rgb_ref.PC
    raw = [rgb_ref.picture("textured", lay, SW, SH, seed=40 + i) for i in range(N)]
    size = ["--input-size", "%dx%d" % (SW, SH), "--output-size", "%dx%d" % (SW, SH)]
    assert len(rgb_ref.raw_bytes(raw[0])) == SW * SH * 3
    _pair(tmp_path, "rgb24", [rgb_ref.raw_bytes(f) for f in raw], ["--input-format", "rgb24", "--colorspace", "bt601", "--range", "pc"], size,
          [format_ref.raw_bytes(rgb_ref.convert(lay, matrix, rng, f)) for f in raw], size, SW, SH)


def test_gbrp_input_scaled_against_the_converted_then_scaled_sequence(built, tmp_path):
    """Conversion comes before scaling: run B reads frames converted (bt709 tv, the defaults) and then scaled by the references."""
    lay = rgb_ref.GBRP
    raw = [rgb_ref.picture("textured", lay, SW, SH, seed=50 + i) for i in range(N)]
    scaled = [scale_ref.scale_planes(rgb_ref.convert(lay, rgb_ref.BT709, rgb_ref.TV, f), VW, VH) for f in raw]
    _pair(tmp_path, "gbrp", [rgb_ref.raw_bytes(f) for f in raw], ["--input-format", "gbrp"],
          ["--scale", "--input-size", "%dx%d" % (SW, SH), "--output-size", "%dx%d" % (VW, VH)],
          [format_ref.raw_bytes(f) for f in scaled], ["--input-size", "%dx%d" % (VW, VH), "--output-size", "%dx%d" % (VW, VH)], VW, VH)
