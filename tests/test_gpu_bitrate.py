"""--bitrate of the native program (wrenc_amd/csrc/host/wrenc_main.cpp: wrenc_gpu_download_complexity per batch,
include/wrenc_rate.h's controller, wrenc_gpu_set_slot_qp per slot) on a sequence with a scene change on a batch
boundary: 80 smooth, then 80 textured pictures of 352x288 in batches of 16.  The yardstick is the existing fixed-QP
path: the target lies half way (in the logarithm) between the totals of --qp 32 and --qp 33, where no constant QP gets
closer than half their distance.

Measured on an MI355X: B32 973,479, B33 897,349, total 933,672, |ln(total / target)| 0.0010 against the bound 0.0407; QPs per
batch 26-27, 26-27, 22-23, 23-24, 31-32 (smooth), 37-38, 33, 38-39, 44-45, 50-51 (textured)."""
import json
import math
import os
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
W, H, N, BATCH, FPS = 352, 288, 160, 16, 30


def _native(args, **kw):
    return subprocess.run([NATIVE] + [str(a) for a in args], capture_output=True, timeout=600, **kw)


@pytest.fixture(scope="module")
def runs(built, tmp_path_factory):
    """The sequence, the two fixed-QP baselines and the --bitrate run (with its repeats), made once."""
    from wrenc_amd import synth
    d = tmp_path_factory.mktemp("bitrate")
    src = d / "in.yuv"
    with open(src, "wb") as f:
        for i in range(N):
            make = synth.synth_frame if i < N // 2 else synth.synth_textured_frame
            f.write(b"".join(p.tobytes() for p in make(W, H, i % 8)))
    common = ["-i", src, "--input-size", "%dx%d" % (W, H), "--output-size", "%dx%d" % (W, H), "--num-pictures", N,
              "--max-split-depth", 2, "--batch", BATCH]

    def run(name, extra):
        out, met, rec = d / (name + ".vvc"), d / (name + ".json"), d / (name + ".yuv")
        r = _native(common + ["-o", out, "--metrics", met, "-r", rec] + extra)
        assert r.returncode == 0 and b"error" not in r.stderr, r.stderr
        return {"stream": out.read_bytes(), "metrics": json.load(open(met)), "rec": rec, "stderr": r.stderr.decode()}

    res = {"common": common, "dir": d, "q32": run("q32", ["--qp", 32]), "q33": run("q33", ["--qp", 33])}
    b32, b33 = len(res["q32"]["stream"]), len(res["q33"]["stream"])
    assert b32 > b33
    res["target"] = math.sqrt(b32 * b33)                       # bytes of the whole stream
    res["kbps"] = res["target"] / N * 8.0 * FPS / 1000.0
    rate = ["--qp", 26, "--bitrate", "%.6f" % res["kbps"], "--fps", FPS]
    res["rate_args"] = rate
    res["rc"] = run("rc", rate + ["--verbose"])
    return res


def _batch_qps(m):
    qp = m["frame_qp"]
    assert len(qp) == N
    return [qp[i:i + BATCH] for i in range(0, N, BATCH)]


def test_total_is_closer_than_any_constant_qp(runs):
    b32, b33 = len(runs["q32"]["stream"]), len(runs["q33"]["stream"])
    total = len(runs["rc"]["stream"])
    m = runs["rc"]["metrics"]
    assert 0 < total - sum(m["frame_bytes"]) < 512            # the total counts the parameter sets
    err, bound = abs(math.log(total / runs["target"])), 0.5 * math.log(b32 / b33)
    print("B32 %d  B33 %d  target %.0f  total %d  |ln(total/target)| %.4f  bound %.4f  QPs per batch %s" % (
        b32, b33, runs["target"], total, err, bound, [sorted(set(q)) for q in _batch_qps(m)]))
    print("\n".join(l for l in runs["rc"]["stderr"].splitlines() if l.startswith("rate control:")))
    assert err < bound, (err, bound)


def test_two_adjacent_qps_per_batch_and_feed_forward(runs):
    batches = _batch_qps(runs["rc"]["metrics"])
    for q in batches:
        assert max(q) - min(q) <= 1 and all(0 <= v <= 63 for v in q), q
    # The batch at picture 80 is the first textured one, and chosen when only smooth pictures have been reported (those up
    # to picture 47): what raises its QP is its complexity.  It is already above the batch before it and nearer the run's
    # last batch than that one is.
    mean = [sum(q) / len(q) for q in batches]
    before, at, last = mean[N // 2 // BATCH - 1], mean[N // 2 // BATCH], mean[-1]
    assert at > before, (before, at)
    assert abs(at - last) < abs(before - last), (before, at, last)


def test_stream_parses_and_decodes(runs):
    from oracle import pyoracle as po
    stream, m = runs["rc"]["stream"], runs["rc"]["metrics"]
    assert po.parse_stream_info(stream) == {"width": W, "height": H, "init_qp": 26, "n_pictures": N}
    recon = np.fromfile(runs["rc"]["rec"], np.uint8).reshape(N, -1)
    t0 = time.perf_counter()
    for i in range(N):
        back = po.parse_picture(stream, i)
        assert back["slice_qp"] == m["frame_qp"][i], i
        sy, scb, scr = po.spec_decode_record(back, m["frame_qp"][i])
        assert np.array_equal(np.concatenate([sy.ravel(), scb.ravel(), scr.ravel()]), recon[i]), i
    print("parsed and decoded %d pictures in %.2f s" % (N, time.perf_counter() - t0))


def test_bytes_do_not_depend_on_the_run_or_the_threads(runs):
    d = runs["dir"]
    for name, extra in (("again", []), ("t1", ["--threads", 1]), ("compact", ["--tokens", "off", "--ramp-down", "auto"])):
        out = d / (name + ".vvc")
        r = _native(runs["common"] + ["-o", out] + runs["rate_args"] + extra)
        assert r.returncode == 0 and b"error" not in r.stderr, r.stderr
        assert out.read_bytes() == runs["rc"]["stream"], name


def test_fixed_qp_bytes_are_those_of_a_one_qp_file(runs):
    """Nothing of the new path runs without --bitrate: --qp 32 writes what a --qp-file of 32s writes."""
    d = runs["dir"]
    (d / "q.txt").write_text("32 " * N)
    out = d / "file.vvc"
    r = _native(runs["common"] + ["-o", out, "--qp", 32, "--qp-file", d / "q.txt"])
    assert r.returncode == 0 and out.read_bytes() == runs["q32"]["stream"]


@pytest.mark.parametrize("args,message", [
    (["--bitrate", "500", "--qp-file", "q.txt"], b"--bitrate and --qp-file exclude each other"),
    (["--bitrate", "0"], b"Invalid bitrate: 0"),
    (["--bitrate", "-3"], b"Invalid bitrate: -3"),
    (["--bitrate", "fast"], b"Invalid bitrate: fast"),
    (["--bitrate", "500k"], b"Invalid bitrate: 500k"),
    (["--bitrate", "nan"], b"Invalid bitrate: nan"),
    (["--bitrate", "500", "--fps", "0"], b"Invalid fps: 0"),
    (["--bitrate"], b"option --bitrate needs a value"),
])
def test_option_errors(built, tmp_path, args, message):
    (tmp_path / "q.txt").write_text("32 32\n")
    out = tmp_path / "o.vvc"
    r = _native(["-i", tmp_path / "missing.yuv", "-o", out, "--input-size", "64x64", "--output-size", "64x64", "--num-pictures", 2,
                 "--qp", 32] + args, cwd=tmp_path)
    assert r.returncode == 0 and b"error: " + message in r.stderr, r.stderr
    assert not out.exists() or out.stat().st_size == 0
