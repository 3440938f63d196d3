"""--input-format of the command line (wrenc_amd/csrc/host/wrenc_main.cpp): a sequence in a 10-bit or interleaved format,
converted on the device (run A), against the same sequence converted by tests/format_ref.py to yuv420p and coded with the
same options but --input-format (run B): the two runs write the same stream, --reconst and --metrics documents."""
import os
import subprocess

import pytest

import format_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
SW, SH, VW, VH, N, QP = 70, 50, 34, 30, 3, 32


def _run(args):
    return subprocess.run([NATIVE] + args, cwd=ROOT, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Per format: the file in that format and the file of its numpy conversion, N frames of SW x SH."""
    d = tmp_path_factory.mktemp("format")
    files = {}
    for fmt in (format_ref.YUV420P10LE, format_ref.NV12):
        frames = [format_ref.picture("textured", fmt, SW, SH, seed=40 + i) for i in range(N)]
        a, b = d / ("%s.yuv" % format_ref.NAMES[fmt]), d / ("%s_as_yuv420p.yuv" % format_ref.NAMES[fmt])
        a.write_bytes(b"".join(format_ref.raw_bytes(f) for f in frames))
        b.write_bytes(b"".join(format_ref.raw_bytes(format_ref.convert(fmt, f)) for f in frames))
        assert a.stat().st_size == N * format_ref.layout(fmt, SW, SH)["frame_bytes"] and b.stat().st_size == N * SW * SH * 3 // 2
        files[fmt] = (a, b)
    return d, files


def _pair(inputs, fmt, tag, size_args, extra):
    """Runs A and B with the same options; returns their (stream, --reconst, --metrics document)."""
    d, files = inputs
    outs = []
    for name, src, option in (("a", files[fmt][0], ["--input-format", format_ref.NAMES[fmt]]), ("b", files[fmt][1], [])):
        out, rec, rep = (d / ("%s_%s%s" % (tag, name, e)) for e in (".vvc", ".yuv", ".json"))
        args = ["-i", str(src), "-o", str(out), "-r", str(rec), "--pad", "--num-pictures", str(N), "--qp", str(QP),
                "--max-split-depth", "2", "--metrics", str(rep)]
        r = _run(args + size_args + option + extra)
        assert r.returncode == 0 and b"error" not in r.stderr and b"PSNR" in r.stderr, r.stderr     # the metrics summary line
        outs.append((out.read_bytes(), rec.read_bytes(), rep.read_bytes()))
    return outs


def _check_pair(outs, w, h):
    (sa, ra, ma), (sb, rb, mb) = outs
    assert sa == sb and len(sa) > 200
    assert ra == rb and len(ra) == N * w * h * 3 // 2          # --reconst stays 8-bit 4:2:0 of --output-size
    assert ma == mb and b'"width": %d, "height": %d, "frames": %d' % (w, h, N) in ma


@pytest.mark.parametrize("tag,extra", [("plain", []), ("batches", ["--batch", "2", "--threads", "3", "--devices", "0,0"])])
def test_ten_bit_input_against_the_converted_sequence(built, inputs, tag, extra):
    size = ["--input-size", "%dx%d" % (SW, SH), "--output-size", "%dx%d" % (SW, SH)]
    _check_pair(_pair(inputs, format_ref.YUV420P10LE, "p10_" + tag, size, extra), SW, SH)


def test_nv12_input_scaled_against_the_converted_sequence(built, inputs):
    size = ["--scale", "--input-size", "%dx%d" % (SW, SH), "--output-size", "%dx%d" % (VW, VH)]
    _check_pair(_pair(inputs, format_ref.NV12, "nv12_scale", size, []), VW, VH)


def test_yuv420p_is_a_run_without_the_option(built, inputs):
    d, files = inputs
    outs = []
    for tag, extra in (("with", ["--input-format", "yuv420p"]), ("without", [])):
        out, rec = d / ("plain_%s.vvc" % tag), d / ("plain_%s.yuv" % tag)
        r = _run(["-i", str(files[format_ref.NV12][1]), "-o", str(out), "-r", str(rec), "--input-size", "%dx%d" % (SW, SH), "--pad",
                  "--output-size", "%dx%d" % (SW, SH), "--num-pictures", str(N), "--qp", str(QP), "--max-split-depth", "2"] + extra)
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        outs.append((out.read_bytes(), rec.read_bytes()))
    assert outs[0] == outs[1] and len(outs[0][0]) > 500 and len(outs[0][1]) == N * SW * SH * 3 // 2


def test_a_ten_bit_input_is_read_by_its_own_frame_size(built, inputs, tmp_path):
    """A file of as many bytes as two 8-bit frames is one 10-bit frame: the second picture is missing."""
    d, files = inputs
    data = files[format_ref.YUV420P10LE][0].read_bytes()[:2 * SW * SH * 3 // 2]
    src = tmp_path / "short.yuv"
    src.write_bytes(data)
    r = _run(["-i", str(src), "-o", str(tmp_path / "out.vvc"), "--input-size", "%dx%d" % (SW, SH), "--pad", "--output-size",
              "%dx%d" % (SW, SH), "--num-pictures", "2", "--qp", str(QP), "--max-split-depth", "2", "--input-format", "yuv420p10le"])
    assert r.returncode == 0 and b"error: input ended after 1 of 2 pictures" in r.stderr, r.stderr
