"""Device-side PSNR / SSIM (include/wrenc_gpu.h: wrenc_gpu_download_metrics, wrenc_gpu_test_metrics; the kernel is
wrenc_amd/csrc/dev_metrics.h) against wrenc_amd/metrics.py, all through the C ABI: the kernel alone on arbitrary picture
pairs, the read-back behind a real search, determinism, slot states, overlap with a queued encode call, the --metrics
option of both command lines and tools/rd_sweep.py's device path.  The comparison rules are tests/metrics_ref.py's:
squared errors and window counts exact, per-window values bit for bit, a plane's mean within 4 N 2^-53."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import metrics_ref
from content import content

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
SIZES = [(32, 32), (64, 32), (96, 64), (352, 288), (1920, 1088), (3840, 2176)]
KINDS = ("cclm", "stripes20", "noise", "flat", "ramp", "checker", "extremes", "stripes70", "cclm")
KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")
ESTATE, EINVAL = -5, -1


def _noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def _const(w, h, v):
    return tuple(np.full(s, v, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def _check_pair(enc, org, rec, refs=None):
    m, maps = enc.test_metrics(org, rec, maps=True)
    metrics_ref.check_raw(m["_raw"], org, rec, maps, refs)
    plain = enc.test_metrics(org, rec)                     # the product kernel (no maps) gives the same record
    assert plain["_raw"]["bytes"] == m["_raw"]["bytes"]
    return m


@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_against_numpy(built, w, h):
    """The kernel on picture pairs no search makes: planes narrower than a wave's strip of 1008 samples, widths that
    are not a multiple of it, many strips and many row segments."""
    from wrenc_amd import gpu, synth
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2)
    tex = synth.synth_textured_frame(w, h, 1)
    # identical planes: no error, and every window exactly 1.0f (numerator and denominator are the same integers)
    m, maps = enc.test_metrics(tex, tex, maps=True)
    assert m["_raw"]["sse"] == [0, 0, 0]
    assert all(np.all(a.view(np.uint32) == np.float32(1.0).view(np.uint32)) for a in maps)
    assert all(v == float("inf") for v in m["PSNR"].values())
    metrics_ref.check_raw(m["_raw"], tex, tex, maps)
    _check_pair(enc, _const(w, h, 0), _const(w, h, 255))
    _check_pair(enc, _noise(w, h, 11), _noise(w, h, 12))
    rng = np.random.default_rng(5)
    nudged = []
    for p in tex:      # +-1 on a seeded tenth of the samples
        step = np.where(rng.random(p.shape) < 0.1, rng.choice(np.array([-1, 1]), p.shape), 0)
        nudged.append(np.clip(p.astype(np.int64) + step, 0, 255).astype(np.uint8))
    m = _check_pair(enc, tex, tuple(nudged))
    metrics_ref.check_entry(m, tex, tuple(nudged))
    # one differing sample: the corners of every plane, and the seams between lanes' strips (x = 1008), waves' row
    # segments (y = 64) and workgroups (y = 256) where the plane has them
    ident = [(0, np.ones((p.shape[0] // 4 - 1, p.shape[1] // 4 - 1), np.float32)) for p in tex]
    for p in range(3):
        ph, pw = tex[p].shape
        spots = {(0, 0), (ph - 1, pw - 1), (min(64, ph - 1), min(1008, pw - 1)), (min(63, ph - 1), min(1007, pw - 1)),
                 (min(256, ph - 1), min(1011, pw - 1)), (min(255, ph - 1), 0)}
        for y, x in sorted(spots):
            rec = [a.copy() for a in tex]
            rec[p][y, x] ^= 0x80
            refs = list(ident)
            refs[p] = metrics_ref.plane_sums(tex[p], rec[p])
            assert refs[p][0] == 128 * 128
            _check_pair(enc, tex, tuple(rec), refs)
    enc.close()


def _encode_mixed(enc, frames, qps):
    for s, f in enumerate(frames):
        enc.upload(s, *f)
        enc.set_qp(s, qps[s % len(qps)])
    enc.encode(0, len(frames))


def test_after_a_real_search(built):
    """One encode call over 9 slots of mixed content at two QPs: the metrics of every slot are those of (what was
    uploaded, what download returns), and asking for them changes nothing in the slots."""
    from wrenc_amd import gpu
    w, h = 96, 64
    frames = [content(k, w, h, i) for i, k in enumerate(KINDS)]
    enc = gpu.Encoder(w, h, qp=30, max_split_depth=2, n_slots=len(frames))
    _encode_mixed(enc, frames, (30, 37))
    before = [enc.download(s) for s in range(len(frames))]
    mism = enc.final_pass_mismatches()
    got = enc.download_metrics(0, len(frames))
    assert len(got) == len(frames)
    for s, f in enumerate(frames):
        rec = (before[s]["rec_y"], before[s]["rec_cb"], before[s]["rec_cr"])
        metrics_ref.check_raw(got[s]["_raw"], f, rec)
        metrics_ref.check_entry(got[s], f, rec)
        # the same kernel on host copies of the two pictures gives the same record, with the maps bit for bit
        m, maps = enc.test_metrics(f, rec, maps=True)
        metrics_ref.check_raw(m["_raw"], f, rec, maps)
        assert m["_raw"]["bytes"] == got[s]["_raw"]["bytes"], s
    assert any(g["_raw"]["sse"][0] > 0 for g in got)
    sub = enc.download_metrics(3, 4)                                   # a sub-range of the slots
    assert [g["_raw"]["bytes"] for g in sub] == [g["_raw"]["bytes"] for g in got[3:7]]
    after = [enc.download(s) for s in range(len(frames))]
    for s in range(len(frames)):
        for k in KEYS:
            assert np.array_equal(after[s][k], before[s][k]), (s, k)
    assert enc.final_pass_mismatches() == mism == 0
    enc.close()


def test_determinism(built):
    """The same call twice gives the same bytes, and so does the same picture in slot 0 of a 1-picture call and in slot 5
    of a 9-picture call."""
    from wrenc_amd import gpu
    w, h = 352, 288
    frames = [content(k, w, h, i) for i, k in enumerate(KINDS)]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=9)
    enc.upload(0, *frames[5])
    enc.encode(0, 1)
    alone = enc.download_metrics(0, 1)[0]["_raw"]["bytes"]
    assert enc.download_metrics(0, 1)[0]["_raw"]["bytes"] == alone
    for s, f in enumerate(frames):
        enc.upload(s, *f)
    enc.encode(0, 9)
    first = [g["_raw"]["bytes"] for g in enc.download_metrics(0, 9)]
    again = [g["_raw"]["bytes"] for g in enc.download_metrics(0, 9)]
    assert first == again
    assert first[5] == alone
    assert enc.download_metrics(5, 1)[0]["_raw"]["bytes"] == alone
    enc.close()


def test_slot_states(built):
    """Only encoded slots have metrics; a refused call leaves the context usable."""
    from wrenc_amd import gpu
    w, h = 64, 64
    frames = [content(k, w, h, i) for i, k in enumerate(KINDS[:3])]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=3)

    def works():
        for s, f in enumerate(frames):
            enc.upload(s, *f)
        enc.encode(0, 3)
        got = enc.download_metrics(0, 3)
        for s, f in enumerate(frames):
            d = enc.download(s)
            metrics_ref.check_raw(got[s]["_raw"], f, (d["rec_y"], d["rec_cb"], d["rec_cr"]))

    def refused(first, n, code):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.download_metrics(first, n)
        assert e.value.code == code

    enc.upload(0, *frames[0])
    refused(0, 1, ESTATE)                  # only uploaded
    works()
    enc.upload(1, *frames[2])
    refused(1, 1, ESTATE)                  # encoded, then uploaded again: its originals are no longer the searched ones
    refused(0, 3, ESTATE)
    works()
    for first, n in ((3, 1), (-1, 1), (2, 2), (0, 0)):
        refused(first, n, EINVAL)
        works()
    assert enc.final_pass_mismatches() == 0
    enc.close()


def test_metrics_next_to_a_queued_encode_call(built):
    """Two sets of slots: the metrics of set A are asked for while set B's encode call is queued behind A's."""
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    w, h, qp, depth = 64, 64, 32, 2
    frames = [content(KINDS[i % len(KINDS)], w, h, i) for i in range(20)]
    enc = gpu.Encoder(w, h, qp=qp, max_split_depth=depth, n_slots=20)
    for s, f in enumerate(frames):
        enc.upload(s, *f)
    enc.encode(0, 11)
    enc.encode(11, 9)
    got = enc.download_metrics(0, 11)
    enc.sync()
    for s in range(11):
        d = enc.download(s)
        metrics_ref.check_raw(got[s]["_raw"], frames[s], (d["rec_y"], d["rec_cb"], d["rec_cr"]))
    for s in (11, 15, 19):
        d = enc.download(s)
        ref = po.encode_picture(*frames[s], qp, depth)
        for k in KEYS:
            assert np.array_equal(d[k], ref[k]), (s, k)
    assert enc.final_pass_mismatches() == 0
    enc.close()


def _planes(buf, i, w, h):
    per = w * h * 3 // 2
    a = np.frombuffer(buf, np.uint8)[i * per:(i + 1) * per]
    return (a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2))


@pytest.mark.parametrize("front", ["native", "python"])
def test_metrics_option(built, tmp_path, front):
    """7 pictures at --batch 2 (two sets of slots, a short last batch): the report's per-frame values are those of
    (input picture, --reconst picture), its summary their mean, and the stream is the one written without --metrics."""
    from wrenc_amd import bitstream, metrics
    w, h, n, qp = 96, 64, 7, 30
    frames = [content(KINDS[i], w, h, i) for i in range(n)]
    raw = b"".join(p.tobytes() for f in frames for p in f)
    src = tmp_path / "in.yuv"
    src.write_bytes(raw)
    qps = [30, 37, 30, 24, 37, 37, 30]
    qp_file = tmp_path / "qp.txt"
    qp_file.write_text(" ".join(str(q) for q in qps))
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    common = ["-i", str(src), "--input-size", "%dx%d" % (w, h), "--output-size", "%dx%d" % (w, h), "--num-pictures", str(n),
              "--qp", str(qp), "--max-split-depth", "2", "--batch", "2"]
    head = len(bitstream.write_parameter_sets(w, h, qp))
    for tag, extra, want_qp in (("plain", [], [qp] * n), ("qpfile", ["--qp-file", str(qp_file)], qps),
                                ("devices", ["--devices", "0,0"], [qp] * n)):
        out, rec, rep, bare = (tmp_path / (tag + e) for e in (".vvc", ".yuv", ".json", "_bare.vvc"))
        r = subprocess.run(cmd + common + extra + ["-o", str(out), "-r", str(rec), "--metrics", str(rep)], cwd=ROOT,
                           capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr
        line = r.stderr.decode().strip().splitlines()
        assert len(line) == 1 and "PSNR Avg" in line[0] and "SSIM All" in line[0] and line[0].startswith("%d bytes" % out.stat().st_size)
        r = subprocess.run(cmd + common + extra + ["-o", str(bare)], cwd=ROOT, capture_output=True, timeout=600)
        assert r.returncode == 0 and r.stderr == b"", r.stderr
        assert out.read_bytes() == bare.read_bytes()
        doc = json.loads(rep.read_text())
        assert (doc["width"], doc["height"], doc["frames"]) == (w, h, n)
        assert doc["frame_qp"] == want_qp
        assert len(doc["frame_bytes"]) == n and sum(doc["frame_bytes"]) == out.stat().st_size - head
        recon = rec.read_bytes()
        assert len(recon) == len(raw)
        for k in ("PSNR", "SSIM"):
            per = doc[k]["per_frame"]
            assert [p["n"] for p in per] == list(range(1, n + 1))
            want = metrics.summarise(per)
            for a in ("Avg", "Y", "U", "V"):
                assert abs(doc[k]["summary"][a] - want[a]) <= 1e-14 * abs(want[a]), (k, a)
        for i in range(n):
            entry = {k: doc[k]["per_frame"][i] for k in ("PSNR", "SSIM")}
            metrics_ref.check_entry(entry, frames[i], _planes(recon, i, w, h))


def test_metrics_report_with_lossless_pictures(built, tmp_path):
    """Flat pictures, which the encoder reconstructs exactly or nearly so: a per-frame PSNR of a picture without error is
    written as Infinity (which Python's json reads) and an infinite mean as 100, as metrics.summarise does."""
    from wrenc_amd import metrics
    w, h, n = 64, 64, 2
    f = content("flat", w, h, 0)
    src, rep, rec = tmp_path / "in.yuv", tmp_path / "m.json", tmp_path / "r.yuv"
    src.write_bytes(b"".join(p.tobytes() for p in f) * n)
    r = subprocess.run([NATIVE, "-i", str(src), "-o", str(tmp_path / "o.vvc"), "-r", str(rec), "--input-size", "64x64",
                        "--output-size", "64x64", "--num-pictures", str(n), "--qp", "22", "--metrics", str(rep)], cwd=ROOT,
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    doc = json.loads(rep.read_text())
    want = [metrics.frame_metrics(f, _planes(rec.read_bytes(), i, w, h)) for i in range(n)]
    lossless = any(np.isinf(v) for x in want for v in x["PSNR"].values())
    assert ("Infinity" in rep.read_text()) == lossless
    for i in range(n):
        metrics_ref.check_entry({k: doc[k]["per_frame"][i] for k in ("PSNR", "SSIM")}, f, _planes(rec.read_bytes(), i, w, h))
    for k in ("PSNR", "SSIM"):
        summ = metrics.summarise(doc[k]["per_frame"])
        for a in ("Avg", "Y", "U", "V"):
            assert abs(doc[k]["summary"][a] - summ[a]) <= 1e-14 * abs(summ[a]), (k, a)


def test_rd_sweep_device_metrics(built):
    spec = importlib.util.spec_from_file_location("rd_sweep", os.path.join(ROOT, "tools", "rd_sweep.py"))
    rd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rd)
    kw = dict(width=128, height=96, frames=2, verbose=False, keep_streams=True)
    host = rd.run_sweep(**kw)
    dev = rd.run_sweep(device_metrics=True, **kw)
    assert dev["config"]["device_metrics"] is True
    for a, b in zip(host["results"], dev["results"]):
        assert a["_stream"] == b["_stream"] and a["frame_bytes"] == b["frame_bytes"] and a["qp"] == b["qp"]
        for f in range(2):
            rec = (a["_recs"][f]["rec_y"], a["_recs"][f]["rec_cb"], a["_recs"][f]["rec_cr"])
            entry = {k: b["metrics"][k]["per_frame"][f] for k in ("PSNR", "SSIM")}
            metrics_ref.check_entry(entry, host["_frames"][f], rec)
            for k in ("PSNR", "SSIM"):
                assert entry[k]["n"] == a["metrics"][k]["per_frame"][f]["n"] == f + 1
