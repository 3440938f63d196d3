"""--pad of the command lines (wrenc_amd/csrc/host/wrenc_main.cpp; wrenc_amd/cli.py forwards it): a 70x50 sequence coded at
96x64 with a conformance window (run A) against the numpy-padded sequence coded plainly at 96x64 (run B).  B's stream is
what the repository's parser and specification decoder cover (tests/test_gpu_bitstream.py, tests/test_cli.py); A's is
shown to be B's with the window fields in the SPS and nothing else, and never goes to the parser, which accepts only
sps_conformance_window_flag == 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import metrics_ref
from window_stream import NAL_SPS, check_window_sps, crop_planes, pad_planes, split_nals, split_raw, textured

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
VW, VH, CW, CH, N, QP = 70, 50, 96, 64, 3, 32


def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + args, cwd=ROOT, capture_output=True, timeout=600)


def _planes(buf, i, w, h):
    per = w * h * 3 // 2
    a = np.frombuffer(buf, np.uint8)[i * per:(i + 1) * per]
    return (a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pad")
    frames = [textured(VW, VH, 20 + i) for i in range(N)]
    a, b = d / "a.yuv", d / "b.yuv"
    a.write_bytes(b"".join(p.tobytes() for f in frames for p in f))
    b.write_bytes(b"".join(p.tobytes() for f in frames for p in pad_planes(f, CW, CH)))
    return d, frames, a, b


def _pair(front, inputs, tag, extra, metrics=False):
    """Runs A and B with the same options; returns (A's stream, B's stream, A's --reconst, B's --reconst, A's report)."""
    d, _, a_in, b_in = inputs
    outs = []
    for name, src, size in (("a", a_in, ["--pad", "--output-size", "%dx%d" % (VW, VH)]), ("b", b_in, ["--output-size", "%dx%d" % (CW, CH)])):
        out, rec, rep = (d / ("%s_%s_%s%s" % (front, tag, name, e)) for e in (".vvc", ".yuv", ".json"))
        args = ["-i", str(src), "-o", str(out), "-r", str(rec), "--input-size", "%dx%d" % (VW, VH), "--num-pictures", str(N),
                "--qp", str(QP), "--max-split-depth", "2"] + size + extra + (["--metrics", str(rep)] if metrics else [])
        r = _run(front, args)
        assert r.returncode == 0 and (metrics or r.stderr == b""), r.stderr
        outs.append((out.read_bytes(), rec.read_bytes(), json.loads(rep.read_text()) if metrics else None))
    return outs[0][0], outs[1][0], outs[0][1], outs[1][1], outs[0][2]


def _check_relation(sa, sb, ra, rb):
    """Every NAL unit of A other than the SPS is B's, byte for byte; A's SPS is B's with the window; A's reconstruction is
    the crop of B's."""
    na, nb = split_raw(sa), split_raw(sb)
    assert len(na) == len(nb) == 3 + 2 * N
    types = [t for t, _ in split_nals(sa)]
    assert types == [t for t, _ in split_nals(sb)] and types.count(NAL_SPS) == 1
    for i, t in enumerate(types):
        if t != NAL_SPS:
            assert na[i] == nb[i], i
    i = types.index(NAL_SPS)
    check_window_sps(split_nals(sb)[i][1], split_nals(sa)[i][1], (CW, CH), (VW, VH))
    assert len(ra) == N * VW * VH * 3 // 2 and len(rb) == N * CW * CH * 3 // 2
    for k in range(N):
        want = crop_planes(_planes(rb, k, CW, CH), VW, VH)
        got = _planes(ra, k, VW, VH)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), k


@pytest.mark.parametrize("front", ["native", "python"])
def test_pad_against_the_padded_sequence(built, inputs, front):
    sa, sb, ra, rb, doc = _pair(front, inputs, "plain", [], metrics=True)
    _check_relation(sa, sb, ra, rb)
    # the report is that of the visible pictures: the input against A's own reconstruction file
    assert (doc["width"], doc["height"], doc["frames"]) == (VW, VH, N)
    frames = inputs[1]
    for k in range(N):
        entry = {m: doc[m]["per_frame"][k] for m in ("PSNR", "SSIM")}
        metrics_ref.check_entry(entry, frames[k], _planes(ra, k, VW, VH))


@pytest.mark.parametrize("tag,extra", [("compact", ["--tokens", "off"]), ("bitrate", ["--bitrate", "300", "--fps", "30"]),
                                       ("batches", ["--batch", "2", "--threads", "3", "--devices", "0,0"])])
def test_pad_with_other_options(built, inputs, tag, extra):
    sa, sb, ra, rb, _ = _pair("native", inputs, tag, extra)
    _check_relation(sa, sb, ra, rb)


def test_pad_on_whole_ctus_changes_nothing(built, inputs):
    d, _, _, b_in = inputs
    outs = []
    for tag, extra in (("with", ["--pad"]), ("without", [])):
        out, rec = d / ("whole_%s.vvc" % tag), d / ("whole_%s.yuv" % tag)
        r = _run("native", ["-i", str(b_in), "-o", str(out), "-r", str(rec), "--input-size", "96x64", "--output-size", "96x64",
                            "--num-pictures", str(N), "--qp", str(QP), "--max-split-depth", "2"] + extra)
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        outs.append((out.read_bytes(), rec.read_bytes()))
    assert outs[0] == outs[1] and len(outs[0][0]) > 500


@pytest.mark.parametrize("front", ["native", "python"])
def test_refused_sizes(built, inputs, front):
    d, _, a_in, _ = inputs
    base = ["-i", str(a_in), "-o", str(d / "refused.vvc"), "--input-size", "70x50", "--num-pictures", "1", "--qp", "32"]
    for size in ("71x50", "70x51", "14x50", "70x14"):
        r = _run(front, base + ["--pad", "--output-size", size])
        assert r.returncode == 0 and b"error: with --pad, output-size must be even and at least 16x16" in r.stderr, (size, r.stderr)
    r = _run(front, base + ["--output-size", "70x50"])
    assert r.returncode == 0 and b"multiple of the 32x32 CTU" in r.stderr
