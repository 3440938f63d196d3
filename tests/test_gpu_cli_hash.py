"""--hash of the command lines (wrenc_amd/csrc/host/wrenc_main.cpp; wrenc_amd/cli.py forwards it): a decoded picture hash SEI
behind every slice.  With the SEI units removed the stream is the plain run's, byte for byte; that stream goes through the
repository's parser and specification decoder (which know no SEI), and the hash of what THEY decode is what the SEI carries:
device hash == hash of what an independent decoder makes of the stream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import picture_hash_ref as ref
from content import content
from window_stream import pad_planes, split_nals, split_raw, textured

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
W, H, N, QP = 96, 64, 3, 32
NAL_IDR = 7


def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    r = subprocess.run(cmd + args, cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def _planes(buf, i, w, h):
    per = w * h * 3 // 2
    a = np.frombuffer(buf, np.uint8)[i * per:(i + 1) * per]
    return (a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2))


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    d = tmp_path_factory.mktemp("hash")
    frames = [content(k, W, H, 40 + i) for i, k in enumerate(("cclm", "noise", "ramp"))]
    src = d / "in.yuv"
    src.write_bytes(b"".join(p.tobytes() for f in frames for p in f))
    return d, src


def _args(src, out, size=(W, H)):
    return ["-i", str(src), "-o", str(out), "--input-size", "%dx%d" % size, "--output-size", "%dx%d" % size, "--num-pictures", str(N),
            "--qp", str(QP), "--max-split-depth", "2"]


def _sei_units(stream, n=N):
    """The stream without its SEI units and those units, after checking that exactly one follows every slice."""
    types = [t for t, _ in split_nals(stream)]
    assert types.count(ref.NAL_SUFFIX_SEI) == types.count(NAL_IDR) == n
    for i, t in enumerate(types):
        if t == NAL_IDR:
            assert types[i + 1] == ref.NAL_SUFFIX_SEI
        if t == ref.NAL_SUFFIX_SEI:
            assert types[i - 1] == NAL_IDR
    bare, sei = ref.strip_sei(stream)
    return bare, [ref.PREFIX + u for _, u in sei]


@pytest.fixture(scope="module")
def plain(source):
    d, src = source
    out, rec = d / "plain.vvc", d / "plain.yuv"
    r = _run("native", _args(src, out) + ["-r", str(rec)])
    assert r.stderr == b""
    return out.read_bytes(), rec.read_bytes()


@pytest.mark.parametrize("front", ["native", "python"])
@pytest.mark.parametrize("tname,t", ref.TYPES, ids=ref.TYPE_IDS)
def test_hash_option(built, source, plain, front, tname, t):
    from oracle import pyoracle
    d, src = source
    out, rec = d / ("%s_%s.vvc" % (front, tname)), d / ("%s_%s.yuv" % (front, tname))
    r = _run(front, _args(src, out) + ["-r", str(rec), "--hash", tname])
    assert r.stderr == b""
    stream = out.read_bytes()
    bare, sei = _sei_units(stream)
    assert bare == plain[0] and rec.read_bytes() == plain[1]
    assert len(split_raw(stream)) == 3 + 3 * N
    for i in range(N):
        (nal_type, rbsp), = split_nals(sei[i])
        got_type, values = ref.parse_sei(rbsp)
        assert (nal_type, got_type) == (ref.NAL_SUFFIX_SEI, t)
        # what the parser and the specification decoder make of the stream without the SEI units
        back = pyoracle.parse_picture(bare, i)
        decoded = pyoracle.spec_decode_record(back, QP)
        assert values == ref.picture_values(t, decoded), (i, tname)
        assert values == ref.picture_values(t, _planes(plain[1], i, W, H))
        assert sei[i] == ref.sei_nal(t, values)


@pytest.mark.parametrize("tname", ref.TYPE_IDS)
def test_same_bytes_with_any_threads_and_read_back(built, source, tname):
    d, src = source
    outs = []
    for tag, extra in (("t1", ["--threads", "1"]), ("t4", ["--threads", "4"]), ("on", ["--tokens", "on"]), ("off", ["--tokens", "off"]),
                       ("b2", ["--batch", "2", "--devices", "0,0"])):
        out = d / ("same_%s_%s.vvc" % (tname, tag))
        _run("native", _args(src, out) + extra + ["--hash", tname])
        outs.append(out.read_bytes())
    assert all(o == outs[0] for o in outs) and len(_sei_units(outs[0])[1]) == N


def test_hash_with_pad_covers_the_margin(built, tmp_path):
    """70x50 with --pad (run A) against the numpy-padded 96x64 sequence coded plainly (run B): the SEI units are B's, and
    their values are the hashes of B's reconstruction, margin included."""
    vw, vh = 70, 50
    frames = [textured(vw, vh, 20 + i) for i in range(N)]
    a_in, b_in = tmp_path / "a.yuv", tmp_path / "b.yuv"
    a_in.write_bytes(b"".join(p.tobytes() for f in frames for p in f))
    b_in.write_bytes(b"".join(p.tobytes() for f in frames for p in pad_planes(f, W, H)))
    for tname, t in ref.TYPES:
        a_out, b_out, b_rec = tmp_path / ("a_%s.vvc" % tname), tmp_path / ("b_%s.vvc" % tname), tmp_path / ("b_%s.yuv" % tname)
        _run("native", _args(a_in, a_out, (vw, vh)) + ["--pad", "--hash", tname])
        _run("native", _args(b_in, b_out) + ["-r", str(b_rec), "--hash", tname])
        sei_a, sei_b = _sei_units(a_out.read_bytes())[1], _sei_units(b_out.read_bytes())[1]
        assert sei_a == sei_b
        for i in range(N):
            values = ref.parse_sei(split_nals(sei_a[i])[0][1])[1]
            coded = _planes(b_rec.read_bytes(), i, W, H)
            assert values == ref.picture_values(t, coded)
            cropped = tuple(np.ascontiguousarray(p[:hh, :ww]) for p, (ww, hh) in zip(coded, ((vw, vh), (vw // 2, vh // 2), (vw // 2, vh // 2))))
            assert values != ref.picture_values(t, cropped)


def test_metrics_frame_bytes_include_the_sei(built, source, tmp_path):
    d, src = source
    docs = {}
    for tag, extra in (("plain", []), ("md5", ["--hash", "md5"]), ("crc", ["--hash", "crc"])):
        out, rep = tmp_path / (tag + ".vvc"), tmp_path / (tag + ".json")
        _run("native", _args(src, out) + extra + ["--metrics", str(rep)])
        docs[tag] = (json.loads(rep.read_text()), out.read_bytes())
    for tag in ("md5", "crc"):
        sei = _sei_units(docs[tag][1])[1]
        assert docs[tag][0]["frame_bytes"] == [b + len(u) for b, u in zip(docs["plain"][0]["frame_bytes"], sei)]
        assert docs[tag][0]["PSNR"] == docs["plain"][0]["PSNR"] and docs[tag][0]["SSIM"] == docs["plain"][0]["SSIM"]
