"""Whole pictures through the search with the full candidates predicted and reconstructed four samples per lane
(dev_predict.h predict_full, recon_row4): all ten record planes against the CPU oracle, wave and team schedule, at
max-split-depths 0..3 so that 32x32, 16x16 and 8x8 CUs are searched AND win with every family of luma mode and both kinds
of chroma mode -- which a CPU test holds on the oracle's records before anything runs on the device."""
import functools

import numpy as np
import pytest

from content import content

KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr", "ctu_cost")
W = H = 64
CONTENT = ["stripes0", "stripes20", "stripes45", "stripes70", "stripes90", "stripes110", "stripes135", "stripes160",
           "ramp", "checker", "noise", "cclm", "extremes", "flat"]
QPS = [27, 37]
DEPTHS = [0, 1, 2, 3]
# outcomes every CU size must show: the luma mode families the predictor tells apart (PLANAR, DC, horizontal with PDPC,
# pure horizontal, horizontal without PDPC, vertical without, pure vertical, vertical with), DM and CCLM chroma
LUMA_CLASSES = [("planar", 0, 0), ("dc", 1, 1), ("2-17", 2, 17), ("18", 18, 18), ("19-33", 19, 33), ("34-49", 34, 49),
                ("50", 50, 50), ("51-66", 51, 66)]
MIN_CUS = 4


@functools.lru_cache(maxsize=None)
def _pictures():
    from wrenc_amd import synth
    pics = [content(k, W, H, 41) for k in CONTENT]
    pics.append(synth.synth_frame(W, H, 0))
    pics += [synth.synth_textured_frame(W, H, f) for f in (0, 1)]
    assert len(pics) == 17
    return pics


@functools.lru_cache(maxsize=None)
def _reference(qp, depth):
    """The oracle's records of the 17 pictures; computed once per (QP, depth) and shared, never changed."""
    from oracle import pyoracle as po
    return [po.encode_picture(y, cb, cr, qp, depth) for (y, cb, cr) in _pictures()]


def _count_outcomes(rec, counts):
    cu, lm, cm = rec["cu_log2_size"], rec["luma_mode"], rec["chroma_mode"]
    assert cu.shape == (H // 4, W // 4) and lm.shape == cu.shape and cm.shape == (H // 8, W // 8)
    for lg in (3, 4, 5):
        u = 1 << (lg - 2)
        for uy in range(0, H // 4, u):
            for ux in range(0, W // 4, u):
                if cu[uy, ux] != lg:
                    continue
                m = int(lm[uy, ux])
                for name, lo, hi in LUMA_CLASSES:
                    if lo <= m <= hi:
                        counts[(1 << lg, name)] += 1
                counts[(1 << lg, "cclm" if cm[uy // 2, ux // 2] >= 81 else "dm")] += 1


def test_the_pictures_make_every_cu_size_win_with_every_outcome(built):
    """The coverage condition, on the oracle alone: over the union of the batches below, each CU size 8 / 16 / 32 is decided
    at least MIN_CUS times with each family of luma mode, with DM chroma and with CCLM chroma."""
    outcomes = [c[0] for c in LUMA_CLASSES] + ["dm", "cclm"]
    counts = {(n, o): 0 for n in (8, 16, 32) for o in outcomes}
    for qp in QPS:
        for depth in DEPTHS:
            for rec in _reference(qp, depth):
                _count_outcomes(rec, counts)
    print(sorted(counts.items()))
    short = {k: v for k, v in counts.items() if v < MIN_CUS}
    assert not short, short


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", [1, 2])    # one wave per CTU / a team of four waves per CTU
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("qp", QPS)
def test_batches_match_the_oracle(built, qp, depth, schedule):
    """All 17 pictures in one call, then the first 5 (the last workgroup then carries padding waves)."""
    from wrenc_amd import gpu
    pics, ref = _pictures(), _reference(qp, depth)
    enc = gpu.Encoder(W, H, qp=qp, max_split_depth=depth, n_slots=len(pics), schedule=schedule)
    for s, f in enumerate(pics):
        enc.upload(s, *f)
    for n in (len(pics), 5):
        enc.encode(0, n)
        enc.sync()
        assert enc.final_pass_mismatches() == 0
        for s in range(n):
            got = enc.download(s)
            for k in KEYS:
                if not np.array_equal(got[k], ref[s][k]):
                    bad = np.argwhere(got[k] != ref[s][k])
                    raise AssertionError("picture %d of %d, qp %d depth %d schedule %d: %s differs at %d positions, first %s" % (
                        s, n, qp, depth, schedule, k, len(bad), bad[0]))
    enc.close()
