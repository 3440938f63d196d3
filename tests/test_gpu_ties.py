"""Which side of a tie the device's search takes: picture parity with the CPU oracle under a zero RD lambda.

With the default rate model two candidates that tie on distortion differ in header bits, so the other parity files say
next to nothing about the tie rules, although the device holds each of them in several copies (the strict-less updates
of leaf_candidate, leaf_offer and the packed leaf searches; pick_cclm, cclm_probe, dm_keeps, chroma_final; sp > ns in lv_decide,
ctu_step, split8_search, node8_search; the cuts that anticipate those decisions).  Under tie_cases.ZERO a cost is
(float)ssd, ties are everywhere, every split floor and candidate floor is 0.0 and both cuts run at their boundary.
tests/test_tie_cases.py holds, on the CPU, that on these pictures each of the seven rules changes the oracle's record
when it is taken the other way: a device that took the other side of any of them would differ here.

  * every case, ZERO and ZERO_CHROMA, wave schedule, team schedule and an AUTO call, all ten keys of the record;
  * the ZERO record differs from the default model's, and its ctu_cost values are whole numbers (sums of SSDs);
  * candidate level through the trace build, as test_gpu_trace.py, on cases in which R4, R6 and R7 decide;
  * the product library against the exhaustive build under ZERO: the cut at floor == best == 0;
  * one call that mixes the default model with ZERO and ZERO_CHROMA slots (per-slot configs).

A 64x64 picture has one CTU on every anti-diagonal (d = column + 2 * row), so an AUTO call resolves to one schedule
there; the 96x64 cases have a diagonal of two CTUs and their AUTO call runs team and wave launches together."""
import os

import numpy as np
import pytest

import tie_cases as tc
from test_gpu_split_cut import _encode_with, _frame, _same
from test_gpu_trace import _gpu_trace, trace_gpu  # noqa: F401  (trace_gpu is a fixture)

pytestmark = pytest.mark.gpu

GROUPS = tc.groups()


def _run(enc, cases, extra, what):
    n = len(cases)
    enc.encode(0, n)
    enc.sync()
    assert enc.final_pass_mismatches() == 0, what
    out = [enc.download(s) for s in range(n)]
    for s, c in enumerate(cases):
        _same(out[s], tc.record(c, extra), "%s %s %s" % (tc.case_id(c), extra, what))
    return out


@pytest.mark.parametrize("extra", [tc.ZERO, tc.ZERO_CHROMA], ids=["zero", "zero_chroma"])
@pytest.mark.parametrize("group", sorted(GROUPS), ids=lambda g: "%dx%d-d%d" % g)
def test_records_equal_the_oracle_on_every_schedule(built, group, extra):
    from wrenc_amd import gpu
    w, h, depth = group
    cases = GROUPS[group]
    n = len(cases)
    enc = gpu.Encoder(w, h, qp=cases[0][4], max_split_depth=depth, n_slots=n, schedule=gpu.Encoder.SCHEDULE_WAVE,
                      extra_params=extra)
    try:
        for s, c in enumerate(cases):
            enc.upload(s, *tc.frame(c))
            if c[4] != cases[0][4]:
                enc.set_qp(s, c[4])
        got = _run(enc, cases, extra, "wave")
        assert enc.last_schedule() == gpu.Encoder.SCHEDULE_WAVE
        for c, g in zip(cases, got) if extra == tc.ZERO else ():
            plain = tc.record(c, tc.DEFAULT)
            assert any(not np.array_equal(g[k], plain[k]) for k in tc.KEYS), "%s: %s changes nothing" % (tc.case_id(c), extra)
            # a cost is (float)ssd, and so is every sum of costs
            assert np.array_equal(g["ctu_cost"], np.trunc(g["ctu_cost"])) and (g["ctu_cost"] >= 0).all(), tc.case_id(c)
        enc.set_schedule(gpu.Encoder.SCHEDULE_TEAM)
        _run(enc, cases, extra, "team")
        assert enc.last_schedule() == gpu.Encoder.SCHEDULE_TEAM
        enc.set_schedule(gpu.Encoder.SCHEDULE_AUTO)
        enc.test_set_wave_slots((200 * n - 1) // (65 if depth == 3 else 50))   # one-CTU diagonals as teams, the rest as waves
        _run(enc, cases, extra, "auto")
        assert enc.last_schedule() == (gpu.Encoder.SCHEDULE_AUTO if w == 96 else gpu.Encoder.SCHEDULE_TEAM)
    finally:
        enc.close()


# between them R4 and R6 decide at 32x32 .. 4x4 and R7 at the 32x32, 16x16 and 8x8 nodes (test_tie_cases.py)
TRACED = [("flat", 64, 64, 5, 32, 1), ("stripes0", 64, 64, 5, 32, 3), ("extremes", 64, 64, 5, 32, 3),
          ("cclm", 96, 64, 7, 37, 0)]


@pytest.mark.parametrize("schedule", [1, 2])
@pytest.mark.parametrize("case", TRACED, ids=tc.case_id)
def test_every_candidate_cost_matches_oracle(trace_gpu, case, schedule):
    from oracle import pyoracle as po
    assert case in tc.CASES
    y, cb, cr = tc.frame(case)
    got, gtrace = _gpu_trace(trace_gpu, y, cb, cr, case[4], case[5], schedule, extra_params=tc.ZERO)
    po.set_extra_params(tc.ZERO)
    try:
        ref, otrace = po.encode_picture_traced(y, cb, cr, case[4], case[5])
    finally:
        po.set_extra_params(None)
    _same(got, ref, tc.case_id(case))
    for key, vals in gtrace.items():
        assert len(vals) == 1, ("GPU evaluated %s twice with different results" % (key,))
        assert key in otrace, ("GPU evaluated a candidate the reference never evaluates: %s" % (key,))
        assert vals == otrace[key], ("candidate %s: GPU %s oracle %s" % (key, vals, otrace[key]))
    assert len(gtrace) >= 0.9 * len(otrace), (len(gtrace), len(otrace))


@pytest.mark.parametrize("depth", [2, 3])
def test_records_equal_the_exhaustive_build(built, depth):
    """Every floor is 0.0 and so is many a best cost: the split cut and the candidate cut at their boundary."""
    from wrenc_amd import gpu
    w, h, qp = 256, 160, 32
    frames = [_frame(k, w, h, 3) for k in ("smooth", "textured", "noise", "flat", "flat_steps", "cclm", "checker")]
    product = gpu.LIB_PATH
    exhaustive = os.path.join(os.path.dirname(product), "libwrenc_gpu_trace.so")
    assert os.path.exists(exhaustive), "run __graft_entry__.build() first"
    cut = _encode_with(gpu, product, frames, w, h, qp, depth, extra_params=tc.ZERO)
    full = _encode_with(gpu, exhaustive, frames, w, h, qp, depth, extra_params=tc.ZERO)
    for s in range(len(frames)):
        _same(cut[s], full[s], "depth %d picture %d" % (depth, s))
        assert np.array_equal(cut[s]["ctu_cost"], np.trunc(cut[s]["ctu_cost"]))


@pytest.mark.parametrize("schedule", ["wave", "auto"])
def test_mixed_models_in_one_call_equal_the_oracle(built, schedule):
    """A context of the default model at QP 32; every second slot searched with a config resolved under ZERO, every
    fourth under ZERO_CHROMA: each picture has its own lambdas, floors and constant block.  A context holds ONE lambda
    set per QP (include/wrenc_gpu.h, wrenc_gpu_set_slot_qp), so a ZERO config at the context's own QP is refused; the
    other models come at QPs of their own, 27 and 37."""
    from wrenc_amd import gpu
    w, h, depth = 96, 64, 3
    kinds = ("flat", "stripes0", "extremes", "noise", "stripes110", "checker", "cclm", "stripes45")
    model = lambda s: (tc.ZERO, 27) if s % 2 else (tc.ZERO_CHROMA, 37) if s % 4 == 2 else (tc.DEFAULT, 32)
    cases = [(k, w, h, 5, model(s)[1], depth) for s, k in enumerate(kinds)]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=depth, n_slots=len(cases),
                      schedule=gpu.Encoder.SCHEDULE_WAVE if schedule == "wave" else gpu.Encoder.SCHEDULE_AUTO)
    try:
        with pytest.raises(gpu.WrencGpuError, match="another lambda set for this QP"):
            enc.set_slot_config(1, gpu.default_config(w, h, 32, depth, 0, len(cases), tc.ZERO))
        cfgs = {}
        for s, c in enumerate(cases):
            enc.upload(s, *tc.frame(c))
            extra, qp = model(s)
            if extra is not tc.DEFAULT:
                cfgs.setdefault(qp, gpu.default_config(w, h, qp, depth, 0, len(cases), extra))
                assert cfgs[qp].lambda_rd_chroma == 0.0 and (cfgs[qp].lambda_rd == 0.0) == (extra == tc.ZERO)
                enc.set_slot_config(s, cfgs[qp])
        if schedule == "auto":
            enc.test_set_wave_slots((200 * len(cases) - 1) // 65)
        enc.encode(0, len(cases))
        enc.sync()
        assert enc.final_pass_mismatches() == 0
        if schedule == "auto":
            assert enc.last_schedule() == gpu.Encoder.SCHEDULE_AUTO
        for s, c in enumerate(cases):
            _same(enc.download(s), tc.record(c, model(s)[0]), "slot %d %s under %s" % (s, tc.case_id(c), model(s)[0]))
    finally:
        enc.close()
