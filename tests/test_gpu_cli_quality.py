"""--target-psnr of the command lines (wrenc_amd/csrc/host/wrenc_main.cpp; wrenc_amd/cli.py forwards it) on mixed content:
8 smooth, then 8 textured pictures of 160x96, depth 2, batches of 4, a floor of 37.0 dB of luma PSNR.  The yardsticks take
nothing from the program under test: the table PSNR[picture][QP] comes from the library with per-slot QPs and
wrenc_amd/metrics.py, the floor is recomputed from --reconst and the input, the QPs are parsed from the stream."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
W, H, N, BATCH, DEPTH, QP = 160, 96, 16, 4, 2, 26
TARGET = 37.0
QPS = list(range(20, 32))
HASH_CRC = 1                                # include/wrenc_hash.h
# sha256 of the plain --qp 26 stream and of the --bitrate 300 --fps 30 stream of this sequence as the commit before the
# option wrote them
PARENT_QP26_SHA256 = "14f40db4d3e351ee367656356f829738f0a065e37b514e0b2c8252b5924a04eb"
PARENT_BITRATE_SHA256 = "ced70e4bf11e34275b4b7081977c0b90940147e09707d0bd9cb57d695004817e"


def _frames():
    from wrenc_amd import synth
    return [(synth.synth_frame if i < N // 2 else synth.synth_textured_frame)(W, H, i % 8) for i in range(N)]


def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + [str(a) for a in args], cwd=ROOT, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def table(built):
    """PSNR[i][q - 20] of the luma plane, q = 20 .. 31: every picture in 12 slots, a QP per slot, one encode call."""
    from wrenc_amd import gpu, metrics
    enc = gpu.Encoder(W, H, qp=QP, max_split_depth=DEPTH, n_slots=len(QPS))
    out = np.zeros((N, len(QPS)))
    for i, f in enumerate(_frames()):
        for s, q in enumerate(QPS):
            enc.upload(s, *f)
            enc.set_qp(s, q)
        enc.encode(0, len(QPS))
        for s in range(len(QPS)):
            out[i, s] = metrics.psnr_from_mse(metrics.plane_mse(f[0], enc.download(s)["rec_y"]))
    enc.close()
    return out


@pytest.fixture(scope="module")
def runs(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("quality")
    src = d / "in.yuv"
    with open(src, "wb") as f:
        for p in _frames():
            f.write(b"".join(x.tobytes() for x in p))
    common = ["-i", src, "--input-size", "%dx%d" % (W, H), "--output-size", "%dx%d" % (W, H), "--num-pictures", N,
              "--max-split-depth", DEPTH, "--batch", BATCH]

    def run(front, name, extra):
        out, met, rec = d / (name + ".vvc"), d / (name + ".json"), d / (name + ".yuv")
        r = _run(front, common + ["-o", out, "--metrics", met, "-r", rec] + extra)
        assert r.returncode == 0 and b"error" not in r.stderr, r.stderr
        return {"stream": out.read_bytes(), "metrics": json.load(open(met)), "rec": rec, "stderr": r.stderr.decode()}

    quality = ["--qp", QP, "--target-psnr", TARGET, "--hash", "crc"]
    return {"common": common, "dir": d, "quality_args": quality, "run": run,
            "native": run("native", "native", quality + ["--verbose"]), "python": run("python", "python", quality)}


def _best(table):
    """Per picture the largest QP of the table at or above the target."""
    return [max(q for k, q in enumerate(QPS) if row[k] >= TARGET) for row in table]


def test_premise_the_two_halves_want_different_qps(table):
    print("PSNR table, QP %d .. %d:\n%s" % (QPS[0], QPS[-1], np.array2string(table, precision=2, max_line_width=200)))
    for i, row in enumerate(table):
        assert (row >= TARGET).any() and (row < TARGET).any(), i
    best = _best(table)
    print("best QPs:", best)
    assert min(best[N // 2:]) - max(best[:N // 2]) >= 2


def test_floor_every_picture_is_at_or_above_the_target(runs):
    from wrenc_amd import metrics
    res = runs["native"]
    recon = np.fromfile(res["rec"], np.uint8).reshape(N, -1)
    psnr = [metrics.psnr_from_mse(metrics.plane_mse(f[0], recon[i][:W * H].reshape(H, W))) for i, f in enumerate(_frames())]
    print("luma PSNR:", ["%.2f" % p for p in psnr], "QPs:", res["metrics"]["frame_qp"])
    assert min(psnr) >= TARGET
    assert res["metrics"]["quality"]["misses"] == 0 and res["metrics"]["quality"]["target_psnr"] == TARGET
    assert re.search(r"quality: \d+ re-encoded, 0 misses", res["stderr"])


def test_worth_having_smaller_than_the_best_fixed_qp(runs, table):
    fixed = max(q for k, q in enumerate(QPS) if (table[:, k] >= TARGET).all())
    plain = runs["run"]("native", "fixed", ["--qp", fixed, "--hash", "crc"])
    print("fixed QP %d: %d bytes; --target-psnr: %d bytes, QPs %s" % (fixed, len(plain["stream"]), len(runs["native"]["stream"]),
                                                                      runs["native"]["metrics"]["frame_qp"]))
    assert len(runs["native"]["stream"]) < len(plain["stream"])


def test_cost_and_reports(runs):
    import picture_hash_ref
    from oracle import pyoracle as po
    res = runs["native"]
    q = res["metrics"]["quality"]
    print("re-encoded %d, tries %s" % (q["reencoded"], q["tries"]))
    assert q["reencoded"] <= 2 * N
    assert len(q["tries"]) == N and sum(q["tries"]) == q["reencoded"] + N and min(q["tries"]) >= 1
    found = re.findall(r"quality: batch at picture (\d+): (\d+) re-encoded, (\d+) misses", res["stderr"])
    assert [int(f[0]) for f in found] == list(range(0, N, BATCH))
    assert sum(int(f[1]) for f in found) == q["reencoded"] and all(f[2] == "0" for f in found)
    assert "quality: %d re-encoded, 0 misses" % q["reencoded"] in res["stderr"]
    bare, _ = picture_hash_ref.strip_sei(res["stream"])
    assert [po.parse_picture(bare, i)["slice_qp"] for i in range(N)] == res["metrics"]["frame_qp"]


def test_stream_parses_and_decodes_to_the_reconstruction(runs):
    import picture_hash_ref
    from oracle import pyoracle as po
    res = runs["native"]
    bare, sei = picture_hash_ref.strip_sei(res["stream"])
    assert len(sei) == N
    assert po.parse_stream_info(bare) == {"width": W, "height": H, "init_qp": QP, "n_pictures": N}
    recon = np.fromfile(res["rec"], np.uint8).reshape(N, -1)
    for i in range(N):
        back = po.parse_picture(bare, i)
        sy, scb, scr = po.spec_decode_record(back, back["slice_qp"])
        assert np.array_equal(np.concatenate([sy.ravel(), scb.ravel(), scr.ravel()]), recon[i]), i
        assert picture_hash_ref.PREFIX + sei[i][1] == picture_hash_ref.sei_nal(HASH_CRC, picture_hash_ref.picture_values(HASH_CRC, (sy, scb, scr))), i


def test_bytes_depend_on_input_and_options_alone(runs):
    assert runs["python"]["stream"] == runs["native"]["stream"]
    d = runs["dir"]
    for name, extra in (("t1", ["--threads", 1]), ("t8", ["--threads", 8]), ("compact", ["--tokens", "off"]), ("auto", ["--ramp-down", "auto"])):
        out = d / (name + ".vvc")
        r = _run("native", runs["common"] + ["-o", out] + runs["quality_args"] + extra)
        assert r.returncode == 0 and b"error" not in r.stderr, r.stderr
        assert out.read_bytes() == runs["native"]["stream"], name


def test_without_the_option_the_bytes_are_the_parent_commits(runs):
    plain = runs["run"]("native", "plain", ["--qp", QP])
    assert "quality" not in plain["metrics"] and "quality:" not in plain["stderr"]
    assert hashlib.sha256(plain["stream"]).hexdigest() == PARENT_QP26_SHA256
    rate = runs["run"]("native", "rate", ["--qp", QP, "--bitrate", 300, "--fps", 30])
    assert hashlib.sha256(rate["stream"]).hexdigest() == PARENT_BITRATE_SHA256
