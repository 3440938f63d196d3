"""The split cut with floors on the device (wrenc_amd/csrc/dev_search.h, split_floor_cut): a split is given up before a
child is searched once the partial cost plus the floors of the children still to come exceeds the unsplit cost.  The
decision is the reference's, so every record stays what the exhaustive search makes:

  * against the CPU oracle on every plane, on smooth, textured, noise and flat content at max-split-depth 1, 2 and 3,
    wave schedule and AUTO calls that mix team (exhaustive) and wave (cut) diagonals;
  * with mixed per-picture QPs in one call, every picture with the floors of its own QP;
  * in contexts created with extra-params, whose floors come from the tuned tables;
  * on larger pictures against the exhaustive build of the same sources (libwrenc_gpu_trace.so);
  * CIF at QP 20, depth 3.
tests/test_split_floor.py holds the rule and the floors themselves on the CPU."""
import os

import numpy as np
import pytest

from content import content

pytestmark = pytest.mark.gpu

KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr",
        "ctu_cost")
EXTRAS = ("header_bits_dq_trellis=1.0,chroma_header_bits_dq_trellis=1.5,planer_offset_dq_trellis=1.1",   # larger header bits
          "a=0.4,mpm_idx_pow=0.45,mpm_remainder_pow=0.3",                                                 # another chroma lambda
          "quant_lambda_mul_trellis=86")                                                                  # the edge rate model at QP 32


def _frame(kind, w, h, i):
    from wrenc_amd import synth
    if kind == "smooth":
        return synth.synth_frame(w, h, i)
    if kind == "textured":
        return synth.synth_textured_frame(w, h, i)
    if kind == "flat":
        y, cb, cr = content("flat", w, h, i)
        return y + np.uint8(17 * i), cb - np.uint8(9 * i), cr + np.uint8(5 * i)
    return content(kind, w, h, 60 + i)


def _same(got, ref, what):
    for k in KEYS:
        if not np.array_equal(got[k], ref[k]):
            bad = np.argwhere(got[k] != ref[k])
            raise AssertionError("%s: %s differs at %d positions, first %s" % (what, k, len(bad), bad[0]))


def _run(enc, n, refs, what):
    enc.encode(0, n)
    enc.sync()
    assert enc.final_pass_mismatches() == 0
    for s in range(n):
        _same(enc.download(s), refs[s], "%s slot %d" % (what, s))


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("kind,qp", [("smooth", 32), ("textured", 32), ("noise", 27), ("flat", 37)])
def test_records_equal_the_oracle(built, kind, qp, depth):
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    w, h, n = 160, 96, 6
    frames = [_frame(kind, w, h, i) for i in range(n)]
    refs = [po.encode_picture(*f, qp, depth) for f in frames]
    enc = gpu.Encoder(w, h, qp=qp, max_split_depth=depth, n_slots=n, schedule=gpu.Encoder.SCHEDULE_WAVE)
    for s, f in enumerate(frames):
        enc.upload(s, *f)
    _run(enc, n, refs, "%s qp%d depth %d wave" % (kind, qp, depth))
    assert enc.last_schedule() == 1
    enc.set_schedule(gpu.Encoder.SCHEDULE_AUTO)
    enc.test_set_wave_slots((200 * n - 1) // (65 if depth == 3 else 50))   # one-CTU diagonals as teams, the rest as waves
    _run(enc, n, refs, "%s qp%d depth %d auto" % (kind, qp, depth))
    assert enc.last_schedule() == 0
    enc.close()


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("schedule", ["wave", "auto"])
def test_mixed_qps_in_one_call_equal_the_oracle(built, depth, schedule):
    """Eight pictures of four kinds at QP 22 .. 46 in a context created at QP 32."""
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    w, h = 96, 64
    kinds = ("smooth", "textured", "noise", "flat")
    qps = (22, 27, 37, 46, 32, 41, 18, 51)
    frames = [_frame(kinds[i % 4], w, h, i) for i in range(8)]
    refs = [po.encode_picture(*f, q, depth) for f, q in zip(frames, qps)]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=depth, n_slots=8,
                      schedule=gpu.Encoder.SCHEDULE_WAVE if schedule == "wave" else gpu.Encoder.SCHEDULE_AUTO)
    for s, f in enumerate(frames):
        enc.upload(s, *f)
        enc.set_qp(s, qps[s])
    if schedule == "auto":
        enc.test_set_wave_slots(20)      # 8 x 1 CTU <= 20 x pct% < 8 x 2 CTUs: both schedules run
    _run(enc, 8, refs, "mixed qps depth %d %s" % (depth, schedule))
    if schedule == "auto":
        assert enc.last_schedule() == 0
    enc.close()


@pytest.mark.parametrize("extra", EXTRAS)
def test_extra_params_contexts_equal_the_oracle(built, extra):
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    w, h, qp, depth = 96, 64, 32, 3
    frames = [_frame(k, w, h, 2) for k in ("smooth", "textured", "noise", "flat")]
    po.set_extra_params(extra)
    try:
        refs = [po.encode_picture(*f, qp, depth) for f in frames]
    finally:
        po.set_extra_params(None)
    enc = gpu.Encoder(w, h, qp=qp, max_split_depth=depth, n_slots=4, schedule=gpu.Encoder.SCHEDULE_WAVE, extra_params=extra)
    for s, f in enumerate(frames):
        enc.upload(s, *f)
    _run(enc, 4, refs, extra)
    enc.close()


def _encode_with(gpu, path, frames, w, h, qp, depth):
    saved = (gpu._lib, gpu.LIB_PATH)
    gpu._lib, gpu.LIB_PATH = None, path
    try:
        enc = gpu.Encoder(w, h, qp=qp, max_split_depth=depth, n_slots=len(frames), schedule=1)
        for s, f in enumerate(frames):
            enc.upload(s, *f)
        enc.encode(0, len(frames))
        enc.sync()
        assert enc.final_pass_mismatches() == 0
        out = [enc.download(s) for s in range(len(frames))]
        enc.close()
        return out
    finally:
        gpu._lib, gpu.LIB_PATH = saved


@pytest.mark.parametrize("qp,depth", [(32, 3), (22, 3), (41, 3), (32, 2), (32, 1)])
def test_larger_pictures_equal_the_exhaustive_build(built, qp, depth):
    from wrenc_amd import gpu
    w, h = 512, 288
    frames = [_frame(k, w, h, 5) for k in ("smooth", "textured", "noise", "flat", "cclm", "extremes")]
    product = gpu.LIB_PATH
    exhaustive = os.path.join(os.path.dirname(product), "libwrenc_gpu_trace.so")
    assert os.path.exists(exhaustive), "run __graft_entry__.build() first"
    cut = _encode_with(gpu, product, frames, w, h, qp, depth)
    full = _encode_with(gpu, exhaustive, frames, w, h, qp, depth)
    for s in range(len(frames)):
        _same(cut[s], full[s], "qp%d depth %d picture %d" % (qp, depth, s))


def test_cif_qp20_depth3_equals_the_oracle(built):
    from wrenc_amd import gpu, synth
    from oracle import pyoracle as po
    w, h = 352, 288
    frames = [synth.synth_frame(w, h, 0), synth.synth_textured_frame(w, h, 0)]
    refs = [po.encode_picture(*f, 20, 3) for f in frames]
    enc = gpu.Encoder(w, h, qp=20, max_split_depth=3, n_slots=2, schedule=gpu.Encoder.SCHEDULE_WAVE)
    for s, f in enumerate(frames):
        enc.upload(s, *f)
    _run(enc, 2, refs, "cif qp20 depth 3")
    enc.close()
