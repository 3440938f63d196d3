"""--scale of the command lines (wrenc_amd/csrc/host/wrenc_main.cpp; wrenc_amd/cli.py forwards it): a 70x50 sequence scaled
to 34x30 on the device and padded (run A) against the sequence scaled by tests/scale_ref.py and coded with the same options
but --scale (run B): the two runs write the same stream, --reconst and --metrics documents."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scale_ref
from window_stream import textured

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
SW, SH, VW, VH, N, QP = 70, 50, 34, 30, 3, 32


def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + args, cwd=ROOT, capture_output=True, timeout=600)


def _raw(frames):
    return b"".join(p.tobytes() for f in frames for p in f)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("scale")
    frames = [textured(SW, SH, 40 + i) for i in range(N)]
    a, b = d / "a.yuv", d / "b.yuv"
    a.write_bytes(_raw(frames))
    b.write_bytes(_raw([scale_ref.scale_planes(f, VW, VH) for f in frames]))
    return d, a, b


def _pair(front, inputs, tag, extra):
    """Runs A and B with the same options; returns their (stream, --reconst, --metrics document)."""
    d, a_in, b_in = inputs
    outs = []
    for name, src, scale in (("a", a_in, ["--scale"]), ("b", b_in, [])):
        out, rec, rep = (d / ("%s_%s_%s%s" % (front, tag, name, e)) for e in (".vvc", ".yuv", ".json"))
        args = ["-i", str(src), "-o", str(out), "-r", str(rec), "--input-size", "%dx%d" % (SW, SH), "--pad", "--output-size",
                "%dx%d" % (VW, VH), "--num-pictures", str(N), "--qp", str(QP), "--max-split-depth", "2", "--metrics", str(rep)]
        r = _run(front, args + scale + extra)
        assert r.returncode == 0 and b"error" not in r.stderr and b"PSNR" in r.stderr, r.stderr     # the metrics summary line
        outs.append((out.read_bytes(), rec.read_bytes(), rep.read_bytes()))
    return outs


def _check_pair(outs):
    (sa, ra, ma), (sb, rb, mb) = outs
    assert sa == sb and len(sa) > 200
    assert ra == rb and len(ra) == N * VW * VH * 3 // 2
    assert ma == mb and b'"width": %d, "height": %d, "frames": %d' % (VW, VH, N) in ma


@pytest.mark.parametrize("front", ["native", "python"])
def test_scale_against_the_scaled_sequence(built, inputs, front):
    _check_pair(_pair(front, inputs, "plain", []))


@pytest.mark.parametrize("tag,extra", [("compact", ["--tokens", "off"]), ("bitrate", ["--bitrate", "300", "--fps", "30"]),
                                       ("batches", ["--batch", "2", "--threads", "3", "--devices", "0,0"])])
def test_scale_with_other_options(built, inputs, tag, extra):
    _check_pair(_pair("native", inputs, tag, extra))


def test_scale_with_equal_sizes_changes_nothing(built, inputs):
    d, a_in, _ = inputs
    outs = []
    for tag, extra in (("with", ["--scale"]), ("without", [])):
        out, rec = d / ("equal_%s.vvc" % tag), d / ("equal_%s.yuv" % tag)
        r = _run("native", ["-i", str(a_in), "-o", str(out), "-r", str(rec), "--input-size", "%dx%d" % (SW, SH), "--pad",
                            "--output-size", "%dx%d" % (SW, SH), "--num-pictures", str(N), "--qp", str(QP), "--max-split-depth", "2"] + extra)
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        outs.append((out.read_bytes(), rec.read_bytes()))
    assert outs[0] == outs[1] and len(outs[0][0]) > 500 and len(outs[0][1]) == N * SW * SH * 3 // 2


def test_a_scaled_stream_decodes_to_its_reconstruction(built, tmp_path):
    """128x96 -> 64x64 (whole CTUs: the stream carries no window, which is what the parser accepts): the stream parses, its
    pictures are those of a direct encode of the numpy-scaled frames, and the specification decoder rebuilds --reconst."""
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    sw, sh, w, h, depth = 128, 96, 64, 64, 2
    frames = [textured(sw, sh, 50 + i) for i in range(2)]
    src, out, rec = tmp_path / "in.yuv", tmp_path / "out.vvc", tmp_path / "rec.yuv"
    src.write_bytes(_raw(frames))
    r = _run("native", ["-i", str(src), "-o", str(out), "-r", str(rec), "--scale", "--input-size", "%dx%d" % (sw, sh), "--output-size",
                        "%dx%d" % (w, h), "--num-pictures", "2", "--qp", str(QP), "--max-split-depth", str(depth)])
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    stream = out.read_bytes()
    assert po.parse_stream_info(stream) == {"width": w, "height": h, "init_qp": QP, "n_pictures": 2}
    recon = np.frombuffer(rec.read_bytes(), np.uint8)
    per = w * h * 3 // 2
    assert recon.size == 2 * per
    enc = gpu.Encoder(w, h, qp=QP, max_split_depth=depth)
    for i, f in enumerate(frames):
        want = enc.encode_picture(*scale_ref.scale_planes(f, w, h))
        back = po.parse_picture(stream, i)
        for k in ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr"):
            assert np.array_equal(back[k], want[k]), (i, k)
        planes = po.spec_decode_record(back, QP)
        got = recon[i * per:(i + 1) * per]
        assert np.array_equal(got, np.concatenate([p.ravel() for p in planes])), i
    enc.close()
