"""Per-picture QP on the device (wrenc_gpu_set_slot_qp): a call whose pictures carry different QPs gives every picture
exactly what a context created at its QP gives, whatever the schedule; the QPs a call runs at are those of the moment it
was enqueued; bad per-QP configs are refused without harming the context; and the command line's --qp-file and
rd_sweep --one-pass write the streams the per-QP paths write."""
import os
import subprocess

import numpy as np
import pytest

from content import content

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
W, H, CTX_QP = 96, 64, 32
QPS = (22, 27, 32, 37)
KINDS = ("noise", "cclm", "stripes20", "checker")
PLANES = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")
REC_KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr")


def _frames(n):
    return [content(KINDS[i % len(KINDS)], W, H, 40 + i) for i in range(n)]


def _slot_qps(n):
    return [QPS[i % len(QPS)] for i in range(n)]     # interleaved: without the grouping every workgroup mixes QPs


_REF = {}


def _reference(depth, frames, qps):
    """Each picture from a context created at its own QP (one call per QP)."""
    key = (depth, len(frames), tuple(qps))
    if key not in _REF:
        from wrenc_amd import gpu
        out = [None] * len(frames)
        for q in sorted(set(qps)):
            idx = [i for i, x in enumerate(qps) if x == q]
            enc = gpu.Encoder(W, H, qp=q, max_split_depth=depth, n_slots=len(idx))
            for s, i in enumerate(idx):
                enc.upload(s, *frames[i])
            enc.encode(0, len(idx))
            for s, i in enumerate(idx):
                out[i] = enc.download(s)
            assert enc.final_pass_mismatches() == 0
            enc.close()
        _REF[key] = out
    return _REF[key]


def _mixed_encoder(depth, frames, qps, schedule=None):
    from wrenc_amd import gpu
    enc = gpu.Encoder(W, H, qp=CTX_QP, max_split_depth=depth, n_slots=len(frames), schedule=schedule)
    for s, f in enumerate(frames):
        enc.upload(s, *f)
        enc.set_qp(s, qps[s])
    return enc


@pytest.mark.parametrize("depth", [3, 2])
@pytest.mark.parametrize("schedule", ["wave", "team", "auto"])
def test_mixed_call_equals_single_qp_contexts(built, depth, schedule):
    from wrenc_amd import gpu
    frames = _frames(16)
    qps = _slot_qps(16)
    ref = _reference(depth, frames, qps)
    sched = {"wave": gpu.Encoder.SCHEDULE_WAVE, "team": gpu.Encoder.SCHEDULE_TEAM, "auto": gpu.Encoder.SCHEDULE_AUTO}[schedule]
    enc = _mixed_encoder(depth, frames, qps, sched)
    if schedule == "auto":
        # a small call that mixes team and wave diagonals as a big one does: 16 x 1 CTU <= 40 x pct% < 16 x 2 CTUs
        enc.test_set_wave_slots(40)
    enc.encode(0, 16)
    for s in range(16):
        got = enc.download(s)
        for k in PLANES:
            assert np.array_equal(got[k], ref[s][k]), (s, qps[s], k)
    if schedule == "auto":
        assert enc.last_schedule() == 0   # both schedules ran
    assert enc.final_pass_mismatches() == 0
    assert enc.test_scratch_overflows() == 0
    enc.close()


def test_mixed_call_equals_the_oracle(built):
    from oracle import pyoracle as po
    depth = 3
    frames = _frames(8)
    qps = _slot_qps(8)
    enc = _mixed_encoder(depth, frames, qps)
    enc.encode(0, 8)
    for s in range(4):                    # one picture per QP
        got = enc.download(s)
        want = po.encode_picture(*frames[s], qps[s], depth)
        for k in PLANES:
            assert np.array_equal(got[k], want[k]), (qps[s], k)
    enc.close()


def test_mixed_call_round_trips_through_the_writer(built):
    from wrenc_amd import bitstream as bs
    from oracle import pyoracle as po
    depth = 3
    frames = _frames(8)
    qps = _slot_qps(8)
    ref = _reference(depth, frames, qps)
    enc = _mixed_encoder(depth, frames, qps)
    enc.encode(0, 8)
    dense = [enc.download(s) for s in range(8)]
    compact = enc.download_compact(0, 8)
    pool, toks = enc.download_tokens(0, 8)
    head = bs.write_parameter_sets(W, H, CTX_QP)
    for s in range(8):
        mask, pay, maps = compact[s]
        ly, lcb, lcr = enc.expand_levels(mask, pay)
        rec = dict(maps, lev_y=ly, lev_cb=lcb, lev_cr=lcr)
        a = bs.write_picture_qp(W, H, CTX_QP, qps[s], s, rec)
        b = bs.write_picture_tokens_qp(W, H, CTX_QP, qps[s], s, pool, toks[s])
        want = bs.write_picture_qp(W, H, CTX_QP, qps[s], s, ref[s])
        assert a == b == want, s
        back = po.parse_picture(head + a, 0)
        assert back["slice_qp"] == qps[s]
        for k in REC_KEYS:
            assert np.array_equal(back[k], dense[s][k]), (s, k)
        for plane, k in zip(po.spec_decode_record(back, qps[s]), ("rec_y", "rec_cb", "rec_cr")):
            assert np.array_equal(plane, dense[s][k]), (s, k)
    enc.close()


def test_two_calls_in_flight_keep_their_qps(built):
    depth = 2
    frames = _frames(16)
    first = [QPS[(i + 1) % 4] for i in range(8)] + [QPS[i % 4] for i in range(8)]
    enc = _mixed_encoder(depth, frames, first)
    enc.encode(0, 8)
    for s in range(8):                    # re-set after the first call is enqueued: it must not see these
        enc.set_qp(s, 63)
    enc.encode(8, 8)
    for s in range(8, 16):
        enc.set_qp(s, None)
    got = [enc.download(s) for s in range(16)]
    for s in range(16):
        ref = _reference(depth, frames, first)   # one picture per QP of `first`, from contexts at that QP
        for k in PLANES:
            assert np.array_equal(got[s][k], ref[s][k]), (s, first[s], k)
    # and the new settings hold for the next call
    enc.encode(0, 16)
    again = [enc.download(s) for s in (0, 8)]
    from wrenc_amd import gpu
    single = gpu.Encoder(W, H, qp=63, max_split_depth=depth)
    assert np.array_equal(again[0]["lev_y"], single.encode_picture(*frames[0])["lev_y"])
    single.close()
    single = gpu.Encoder(W, H, qp=CTX_QP, max_split_depth=depth)
    assert np.array_equal(again[1]["rec_y"], single.encode_picture(*frames[8])["rec_y"])
    single.close()
    assert enc.final_pass_mismatches() == 0
    enc.close()


def _fits(cfg):
    room = (1 << 25) - 128 * 65535
    dq = np.array(cfg.dq_table, np.int64)
    return 0 <= cfg.lambda_q < room and dq.min() >= 0 and dq.max() < room and cfg.lambda_q * int(dq.max()) < room


def test_refusals_leave_the_slot_and_the_context_usable(built):
    from wrenc_amd import gpu
    depth = 2
    extra = "quant_lambda_mul_trellis=1.5"
    at32 = gpu.default_config(W, H, 32, depth, extra_params=extra)
    at63 = gpu.default_config(W, H, 63, depth, extra_params=extra)
    assert _fits(at32) and not _fits(at63)       # the fit formula of wrenc_gpu_create, on the host
    frames = _frames(2)
    enc = gpu.Encoder(W, H, qp=32, max_split_depth=depth, n_slots=2, extra_params=extra)
    for s in range(2):
        enc.upload(s, *frames[s])
    enc.set_qp(1, 27)
    with pytest.raises(gpu.WrencGpuError) as e:
        enc.set_qp(1, 63)
    assert e.value.args and "rate model" in str(e.value)
    other = gpu.default_config(W, H, 37, depth, extra_params="quant_lv_pow=0.49")   # another dq_table
    with pytest.raises(gpu.WrencGpuError):
        enc.set_slot_config(1, other)
    relambda = gpu.default_config(W, H, 27, depth, extra_params=extra)
    relambda.lambda_rd *= 1.5                     # a second lambda set for a QP the context already has
    with pytest.raises(gpu.WrencGpuError):
        enc.set_slot_config(1, relambda)
    enc.encode(0, 2)
    got = enc.download(1)
    enc.close()
    ref = gpu.Encoder(W, H, qp=27, max_split_depth=depth, extra_params=extra)
    want = ref.encode_picture(*frames[1])
    ref.close()
    for k in PLANES:
        assert np.array_equal(got[k], want[k]), k


def _yuv(frames):
    return b"".join(p.tobytes() for f in frames for p in f)


def test_cli_qp_file(built, tmp_path):
    from oracle import pyoracle as po
    n = 7
    frames = _frames(n)
    qps = [22, 37, 27, 32, 45, 22, 30]
    src = tmp_path / "in.yuv"
    src.write_bytes(_yuv(frames))
    (tmp_path / "q.txt").write_text(" ".join(map(str, qps)) + "\n")
    common = ["-i", str(src), "--input-size", "%dx%d" % (W, H), "--output-size", "%dx%d" % (W, H),
              "--num-pictures", str(n), "--max-split-depth", "2", "--batch", "3", "--devices", "0,0"]
    for tokens in ("on", "off"):
        out, rec = tmp_path / ("o_%s.vvc" % tokens), tmp_path / ("r_%s.yuv" % tokens)
        r = subprocess.run([NATIVE] + common + ["-o", str(out), "-r", str(rec), "--qp", "32", "--qp-file",
                                                str(tmp_path / "q.txt"), "--tokens", tokens, "--ramp-down", "always"],
                           capture_output=True, timeout=600)
        assert r.returncode == 0 and b"error" not in r.stderr, r.stderr
        stream = out.read_bytes()
        assert po.parse_stream_info(stream) == {"width": W, "height": H, "init_qp": 32, "n_pictures": n}
        recon = np.frombuffer(rec.read_bytes(), np.uint8).reshape(n, -1)
        for i in range(n):
            back = po.parse_picture(stream, i)
            assert back["slice_qp"] == qps[i]
            sy, scb, scr = po.spec_decode_record(back, qps[i])
            assert np.array_equal(np.concatenate([sy.ravel(), scb.ravel(), scr.ravel()]), recon[i]), i
        if tokens == "on":
            first = stream
        else:
            assert stream == first
    # a file of one QP writes the bytes of --qp alone
    (tmp_path / "q27.txt").write_text("27 " * n)
    outs = []
    for extra in (["--qp-file", str(tmp_path / "q27.txt")], []):
        out = tmp_path / ("same%d.vvc" % len(outs))
        r = subprocess.run([NATIVE] + common + ["-o", str(out), "--qp", "27"] + extra, capture_output=True, timeout=600)
        assert r.returncode == 0 and b"error" not in r.stderr, r.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1]


def test_rd_sweep_one_pass_equals_per_qp_mode(built):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rd_sweep
    kw = dict(width=96, height=64, frames=3, depth=2, qps=(22, 27, 32, 37), threads=2, keep_streams=True, verbose=False)
    a = rd_sweep.run_sweep(**kw)
    b = rd_sweep.run_sweep(one_pass=True, **kw)
    assert len(a["results"]) == len(b["results"]) == 4
    for ra, rb in zip(a["results"], b["results"]):
        assert ra["qp"] == rb["qp"] and ra["title"] == rb["title"]
        assert ra["_stream"] == rb["_stream"] and ra["bytes"] == rb["bytes"] and ra["frame_bytes"] == rb["frame_bytes"]
        assert ra["metrics"] == rb["metrics"]
        assert rb["final_pass_mismatches"] == 0
        assert set(ra) == set(rb)
