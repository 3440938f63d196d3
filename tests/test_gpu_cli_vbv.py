"""--vbv-bufsize of the command lines (wrenc_amd/csrc/host/wrenc_main.cpp; wrenc_amd/cli.py forwards it) on a sequence with
a scene change: 16 smooth, then 16 textured pictures of 352x288 in batches of 4 -- four batches on each side --, a target of
5,800 bytes a picture and a bucket of three pictures' worth.  The yardstick is tests/vbv_ref.py, which walks the bucket
over the bytes in the file and reads nothing the program reports: plain --bitrate at the same target overflows that bucket
(the input is one where enforcement matters), --vbv-bufsize never does, and gets there by coding pictures again."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import vbv_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
W, H, N, BATCH, FPS = 352, 288, 32, 4, 30
KBPS = 1392.0                               # 5,800 bytes a picture
R_BITS = KBPS * 1000.0 / FPS                # 46,400 bits arrive per picture
BUF_KBIT = 139.2                            # three pictures' worth
HASH_CRC = 1                                # include/wrenc_hash.h
# sha256 of the plain --bitrate stream of this sequence as the commit before the buffer model wrote it
PARENT_BITRATE_SHA256 = "5e1d7ab2cd10a11728f4cb5c308ab816b6e3b3330123a110e4fff79b63354a90"


def _run(front, args, **kw):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + [str(a) for a in args], cwd=ROOT, capture_output=True, timeout=600, **kw)


@pytest.fixture(scope="module")
def runs(built, tmp_path_factory):
    """The sequence, the plain --bitrate run and the --vbv-bufsize runs of both front ends, made once."""
    from wrenc_amd import synth
    d = tmp_path_factory.mktemp("vbv")
    src = d / "in.yuv"
    with open(src, "wb") as f:
        for i in range(N):
            make = synth.synth_frame if i < N // 2 else synth.synth_textured_frame
            f.write(b"".join(p.tobytes() for p in make(W, H, i % 8)))
    common = ["-i", src, "--input-size", "%dx%d" % (W, H), "--output-size", "%dx%d" % (W, H), "--num-pictures", N,
              "--max-split-depth", 2, "--batch", BATCH, "--qp", 26, "--bitrate", KBPS, "--fps", FPS]

    def run(front, name, extra):
        out, met, rec = d / (name + ".vvc"), d / (name + ".json"), d / (name + ".yuv")
        r = _run(front, common + ["-o", out, "--metrics", met, "-r", rec] + extra)
        assert r.returncode == 0 and b"error" not in r.stderr, r.stderr
        return {"stream": out.read_bytes(), "metrics": json.load(open(met)), "rec": rec, "stderr": r.stderr.decode()}

    vbv = ["--vbv-bufsize", BUF_KBIT, "--hash", "crc"]
    return {"common": common, "dir": d, "vbv_args": vbv, "plain": run("native", "plain", ["--hash", "crc"]),
            "plain_bare": run("native", "bare", []),
            "native": run("native", "native", vbv + ["--verbose"]), "python": run("python", "python", vbv)}


def test_plain_bitrate_overflows_the_bucket(runs):
    w = vbv_ref.walk(runs["plain"]["stream"], BUF_KBIT * 1000.0, R_BITS)
    print("plain --bitrate: violations at pictures %s, worst %.0f bits over" % (w["violations"], -min(w["left"])))
    assert len(w["violations"]) >= 1
    assert "vbv" not in runs["plain"]["metrics"] and "vbv:" not in runs["plain"]["stderr"]


@pytest.mark.parametrize("front", ["native", "python"])
def test_the_bucket_never_overflows_and_pictures_were_coded_again(runs, front):
    res = runs[front]
    m = res["metrics"]["vbv"]
    w = vbv_ref.walk(res["stream"], BUF_KBIT * 1000.0, R_BITS)
    print("%s: re-encoded %d, violations %d; least bits left %.0f; QPs %s" % (front, m["reencoded"], m["violations"], min(w["left"]),
                                                                              res["metrics"]["frame_qp"]))
    assert w["violations"] == []
    assert m["violations"] == 0 and m["reencoded"] >= 1 and m["bufsize_bits"] == BUF_KBIT * 1000.0
    # what the program reports is what the file says
    assert len(m["fullness"]) == N and np.allclose(m["fullness"], w["left"], rtol=0, atol=1e-6)
    header, pictures = vbv_ref.picture_bytes(res["stream"])
    assert pictures == res["metrics"]["frame_bytes"] and 0 < header < 512
    assert "vbv: %d re-encoded, 0 violations" % m["reencoded"] in res["stderr"]
    assert res["stream"] == runs["native"]["stream"]


def test_verbose_reports_every_batch(runs):
    found = re.findall(r"vbv: batch at picture (\d+): (\d+) re-encoded, (\d+) violations", runs["native"]["stderr"])
    assert [int(f[0]) for f in found] == list(range(0, N, BATCH))
    assert sum(int(f[1]) for f in found) == runs["native"]["metrics"]["vbv"]["reencoded"] and all(f[2] == "0" for f in found)


def test_stream_parses_and_decodes_to_the_reconstruction(runs):
    """Every picture, the ones coded again included: the slice header carries the final QP, --metrics reports it, and the
    stream (its SEI units removed: the parser knows none) decodes to the frames of --reconst."""
    import picture_hash_ref
    from oracle import pyoracle as po
    res = runs["native"]
    bare, sei = picture_hash_ref.strip_sei(res["stream"])
    assert len(sei) == N
    m = res["metrics"]
    assert po.parse_stream_info(bare) == {"width": W, "height": H, "init_qp": 26, "n_pictures": N}
    recon = np.fromfile(res["rec"], np.uint8).reshape(N, -1)
    for i in range(N):
        back = po.parse_picture(bare, i)
        assert back["slice_qp"] == m["frame_qp"][i], i
        sy, scb, scr = po.spec_decode_record(back, m["frame_qp"][i])
        planes = np.concatenate([sy.ravel(), scb.ravel(), scr.ravel()])
        assert np.array_equal(planes, recon[i]), i
        # ... and the SEI behind it is the hash of that final coding
        assert picture_hash_ref.PREFIX + sei[i][1] == picture_hash_ref.sei_nal(HASH_CRC, picture_hash_ref.picture_values(HASH_CRC, (sy, scb, scr))), i
    assert len(set(m["frame_qp"])) > 2                      # a QP per picture, not two per batch


def test_bytes_do_not_depend_on_the_threads(runs):
    d = runs["dir"]
    for name, extra in (("t1", ["--threads", 1]), ("t8", ["--threads", 8]), ("compact", ["--tokens", "off"])):
        out = d / (name + ".vvc")
        r = _run("native", runs["common"] + ["-o", out] + runs["vbv_args"] + extra)
        assert r.returncode == 0 and b"error" not in r.stderr, r.stderr
        assert out.read_bytes() == runs["native"]["stream"], name


def test_without_the_option_the_bytes_are_the_parent_commits(runs):
    assert hashlib.sha256(runs["plain_bare"]["stream"]).hexdigest() == PARENT_BITRATE_SHA256


@pytest.mark.parametrize("front", ["native", "python"])
@pytest.mark.parametrize("args,message", [
    (["--vbv-bufsize", "100"], b"--vbv-bufsize needs --bitrate"),
    (["--vbv-bufsize", "100", "--bitrate", "500", "--qp-file", "q.txt"], b"--bitrate and --qp-file exclude each other"),
    (["--vbv-bufsize", "100", "--qp-file", "q.txt"], b"--vbv-bufsize and --qp-file exclude each other"),
    (["--vbv-bufsize", "16", "--bitrate", "500", "--fps", "30"], b"vbv-bufsize 16 kbit is smaller than one picture's share of the bitrate, 16.667 kbit"),
    (["--vbv-bufsize", "0", "--bitrate", "500"], b"Invalid vbv-bufsize: 0"),
    (["--vbv-bufsize", "-8", "--bitrate", "500"], b"Invalid vbv-bufsize: -8"),
    (["--vbv-bufsize", "big", "--bitrate", "500"], b"Invalid vbv-bufsize: big"),
    (["--vbv-bufsize", "100k", "--bitrate", "500"], b"Invalid vbv-bufsize: 100k"),
    (["--bitrate", "500", "--vbv-bufsize"], b"option --vbv-bufsize needs a value"),
])
def test_option_errors(built, tmp_path, front, args, message):
    (tmp_path / "q.txt").write_text("32 32\n")
    out = tmp_path / "o.vvc"
    r = _run(front, ["-i", tmp_path / "missing.yuv", "-o", out, "--input-size", "64x64", "--output-size", "64x64", "--num-pictures", 2,
                     "--qp", 32] + args)
    assert r.returncode == 0 and b"error: " + message in r.stderr, r.stderr
    assert not out.exists() or out.stat().st_size == 0
