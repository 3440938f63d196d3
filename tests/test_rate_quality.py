"""The quality controller (include/wrenc_rate_quality.h, wrenc_amd/rate.py QualityController) on synthetic PSNR tables: a
"picture" is a table PSNR[q] of what a coding at q would measure and a curve whose prediction is the table plus a constant,
so every rule can be met case by case.  No device."""
import math
import os

import numpy as np
import pytest

from wrenc_amd import bitstream, rate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 32
SAMPLES = W * H


def curve_of(psnr):
    """A (3, 64) distortion curve whose luma row predicts psnr[q] (to the rounding of its integer SSE)."""
    c = np.zeros((3, 64), np.uint64)
    sse = 255.0 ** 2 * SAMPLES / 10.0 ** (np.asarray(psnr, np.float64) / 10.0)
    c[0] = np.round(sse * 4096.0).astype(np.uint64)
    return c


def sse_of(psnr):
    return int(round(255.0 ** 2 * SAMPLES / 10.0 ** (psnr / 10.0)))


def drive(ctl, picture, first_qp, table):
    """Code `picture` as the controller says until it accepts; returns (kept QP, the QPs tried in order)."""
    qp, tried = first_qp, []
    for _ in range(12):
        tried.append(qp)
        accepted, qp = ctl.report(picture, qp, sse_of(table[qp]), SAMPLES)
        if accepted:
            return qp, tried
    raise AssertionError("no acceptance after %s" % tried)


def linear(slope, at37):
    """PSNR falls by `slope` dB a QP and is 37.0 + slope / 2 at QP at37: at37 is the largest passing QP of a 37 dB target."""
    return np.array([37.0 + slope / 2 + slope * (at37 - q) for q in range(64)])


def test_header_and_exports(built):
    lib = bitstream.load_library()
    header = open(os.path.join(ROOT, "include", "wrenc_rate_quality.h")).read()
    for name in bitstream.EXPORTED_QUALITY_SYMBOLS:
        assert getattr(lib, name) and name + "(" in header
    assert "#define WRENC_QUALITY_PRIOR (%s)" % rate.QUALITY_PRIOR in header
    assert "#define WRENC_QUALITY_LEARN %s" % rate.QUALITY_LEARN in header
    assert "#define WRENC_QUALITY_MAX_RECODES %d" % rate.QUALITY_MAX_RECODES in header


def test_create_rejects_bad_configurations(built):
    for args in ((float("nan"),), (0.0,), (-3.0,), (37.0, -1, 63), (37.0, 0, 64), (37.0, 30, 29), (37.0, 0, 63, -1), (37.0, 0, 63, 9)):
        with pytest.raises(rate.RateError):
            rate.QualityController(*args)
    rate.QualityController(37.0, 30, 30, 0).close()


def test_predict_is_the_curves_psnr(built):
    table = linear(0.5, 27)
    got = rate.quality_predict(curve_of(table), W, H)
    assert np.allclose(got, table, atol=1e-3)
    zero = np.zeros((3, 64), np.uint64)
    assert np.isinf(rate.quality_predict(zero, W, H)).all()


def test_choose_takes_the_largest_qp_the_corrected_curve_allows(built):
    ctl = rate.QualityController(37.0)
    assert ctl.correction == rate.QUALITY_PRIOR
    table = linear(0.5, 27)                      # PSNR_pred(q) = 37.25 + 0.5 (27 - q)
    # pred + prior >= 37: 0.25 + 0.5 (27 - q) >= 0.9: q <= 25
    assert ctl.choose([curve_of(table), curve_of(table + 3.0)], W, H) == [25, 31]
    assert ctl.choose([], W, H) == []
    lim = rate.QualityController(37.0, 28, 30)
    assert lim.choose([curve_of(table), curve_of(table + 10.0)], W, H) == [28, 30]


def test_accepts_when_the_next_qp_is_predicted_below(built):
    """The coding is what the curve said plus the prior: at the chosen QP it passes, and the picture's own offset puts the
    next QP below the target: one coding, no recode."""
    ctl = rate.QualityController(37.0)
    pred = linear(0.5, 27)
    truth = pred + rate.QUALITY_PRIOR
    first = ctl.choose([curve_of(pred)], W, H)[0]
    assert truth[first] >= 37.0 > truth[first + 1]
    assert drive(ctl, 0, first, truth) == (first, [first])
    assert ctl.totals() == (0, 0) and ctl.tries(0) == 1


def test_steps_up_until_the_next_qp_fails(built):
    """The codings come out 1.5 dB above the curve: the first QP passes with room, the controller goes up by the curve
    shifted by the measured offset and stops where qp + 1 was tried and failed or is predicted to."""
    ctl = rate.QualityController(37.0, max_recodes=8)
    pred = linear(0.5, 27)
    truth = pred + 1.5
    best = max(q for q in range(64) if truth[q] >= 37.0)
    first = ctl.choose([curve_of(pred)], W, H)[0]
    kept, tried = drive(ctl, 0, first, truth)
    assert kept == best and first < best
    assert len(set(tried)) == len(tried)
    assert ctl.totals() == (len(tried) - 1, 0)


def test_a_slope_of_0_2_db_per_qp_is_followed_to_the_end(built):
    """0.2 dB a QP (smooth content near 34 dB): with the truth 1 dB above the curve the first QP is five QPs low; the
    controller does not stop inside any window above the target."""
    ctl = rate.QualityController(34.0, max_recodes=8)
    pred = np.array([34.1 + 0.2 * (30 - q) for q in range(64)])
    truth = pred + 0.1
    best = max(q for q in range(64) if truth[q] >= 34.0)
    first = ctl.choose([curve_of(pred)], W, H)[0]
    assert best - first >= 4
    kept, tried = drive(ctl, 0, first, truth)
    assert kept == best, tried


def test_below_the_target_steps_down_by_the_deficit_over_the_slope(built):
    ctl = rate.QualityController(37.0, max_recodes=8)
    pred = linear(0.5, 30)
    truth = pred - 3.0                              # 2.1 dB below what the prior allows for: about 4 QPs at 0.5 dB
    first = ctl.choose([curve_of(pred)], W, H)[0]
    accepted, second = ctl.report(0, first, sse_of(truth[first]), SAMPLES)
    assert not accepted and truth[first] < 37.0
    deficit = 37.0 - truth[first]
    assert second == first - math.ceil(deficit / 0.5) and second <= first - 1
    kept, tried = drive(ctl, 0, second, truth)
    assert kept == max(q for q in range(64) if truth[q] >= 37.0)
    assert first not in tried


def test_a_non_monotone_table(built):
    """QP 27 measures BELOW the target although 26 and 28 are above: the controller keeps 26 once 27 has failed, never
    returns to a tried QP, and does not look past the failure."""
    ctl = rate.QualityController(37.0, max_recodes=8)
    pred = linear(0.5, 29)
    truth = pred + rate.QUALITY_PRIOR + 1.0
    truth[27] = 36.5
    assert truth[28] >= 37.0 and truth[26] >= 37.0
    first = ctl.choose([curve_of(pred)], W, H)[0]
    assert first == 27
    assert drive(ctl, 0, first, truth) == (26, [27, 26])
    # started below the dip with a coding 0.1 dB above the curve, it goes where the shifted curve says, past the dip, and
    # 29 passes with 30 predicted below
    ctl.choose([curve_of(pred)], W, H)
    assert drive(ctl, 0, 26, truth) == (29, [26, 29])


def test_a_picture_that_cannot_reach_the_target_is_one_miss(built):
    ctl = rate.QualityController(45.0, qp_min=20, qp_max=40, max_recodes=8)
    truth = linear(0.5, 27)                          # 40.75 dB at QP 20
    first = ctl.choose([curve_of(truth)], W, H)[0]
    assert first == 20
    assert drive(ctl, 0, first, truth) == (20, [20])
    assert ctl.totals() == (0, 1)
    # from higher up: down to qp_min, then the miss
    ctl2 = rate.QualityController(45.0, qp_min=20, qp_max=40, max_recodes=8)
    ctl2.choose([curve_of(truth)], W, H)
    kept, tried = drive(ctl2, 0, 30, truth)
    assert kept == 20 and tried[-1] == 20 and ctl2.totals() == (len(tried) - 1, 1)


def test_max_recodes_0_never_recodes(built):
    ctl = rate.QualityController(37.0, max_recodes=0)
    pred = linear(0.5, 27)
    first = ctl.choose([curve_of(pred)] * 3, W, H)[0]
    assert ctl.report(0, first, sse_of(pred[first] + 2.0), SAMPLES) == (True, first)       # passes with room: kept
    assert ctl.report(1, first, sse_of(36.0), SAMPLES) == (True, first)                    # fails: kept, a miss
    assert ctl.report(2, first, 0, SAMPLES) == (True, first)                               # an SSE of 0
    assert ctl.totals() == (0, 1)


def test_recodes_used_up_keeps_the_largest_passing_qp(built):
    ctl = rate.QualityController(37.0, max_recodes=1)
    pred = linear(0.2, 30)
    truth = pred + 3.0
    first = ctl.choose([curve_of(pred)], W, H)[0]
    accepted, second = ctl.report(0, first, sse_of(truth[first]), SAMPLES)
    assert not accepted and second > first
    # the second coding fails: the first is kept, no miss
    assert ctl.report(0, second, sse_of(36.0), SAMPLES) == (True, first)
    assert ctl.totals() == (1, 0)
    # all failing: the lowest QP tried is kept, a miss
    ctl.choose([curve_of(pred)], W, H)
    accepted, second = ctl.report(0, 40, sse_of(30.0), SAMPLES)
    assert not accepted and second < 40
    assert ctl.report(0, second, sse_of(31.0), SAMPLES) == (True, second)
    assert ctl.totals() == (2, 1)


def test_qp_min_equals_qp_max(built):
    ctl = rate.QualityController(37.0, qp_min=30, qp_max=30, max_recodes=3)
    assert ctl.choose([curve_of(linear(0.5, 27))] * 2, W, H) == [30, 30]
    assert ctl.report(0, 30, sse_of(40.0), SAMPLES) == (True, 30)
    assert ctl.report(1, 30, sse_of(30.0), SAMPLES) == (True, 30)
    assert ctl.totals() == (0, 1)


def test_argument_errors(built):
    ctl = rate.QualityController(37.0, qp_min=10, qp_max=50)
    with pytest.raises(rate.RateError):
        ctl.report(0, 30, 100, SAMPLES)                 # no batch
    ctl.choose([curve_of(linear(0.5, 27))], W, H)
    for args in ((1, 30, 100, SAMPLES), (-1, 30, 100, SAMPLES), (0, 9, 100, SAMPLES), (0, 51, 100, SAMPLES), (0, 30, 100, 0)):
        with pytest.raises(rate.RateError):
            ctl.report(*args)
    accepted, nxt = ctl.report(0, 30, sse_of(30.0), SAMPLES)
    assert not accepted
    with pytest.raises(rate.RateError):
        ctl.report(0, 30, sse_of(30.0), SAMPLES)         # a QP tried before
    with pytest.raises(rate.RateError):
        ctl.choose(np.zeros((2, 64), np.uint64), W, H)


def test_the_correction_is_learnt_and_the_same_calls_give_the_same_answers(built):
    def run():
        ctl = rate.QualityController(37.0, max_recodes=8)
        log = []
        pred = linear(0.5, 27)
        truth = pred - 2.0
        for batch in range(3):
            qps = ctl.choose([curve_of(pred + k) for k in range(4)], W, H)
            for k, q in enumerate(qps):
                log.append((batch, k) + drive(ctl, k, q, truth + k) + (ctl.correction,))
        return log, ctl.totals()
    a, b = run(), run()
    assert a == b
    log, (reencoded, misses) = a
    assert misses == 0
    # the offset is -2 dB everywhere: the correction goes from the prior towards it and the later batches need no recodes
    assert abs(log[-1][-1] + 2.0) < 0.1
    assert all(len(tried) == 1 for batch, _, _, tried, _ in log if batch == 2)
    assert reencoded == sum(len(t) - 1 for _, _, _, t, _ in log)


NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")


@pytest.mark.parametrize("front", ["native", "python"])
@pytest.mark.parametrize("args,message", [
    (["--target-psnr", "37", "--bitrate", "500"], b"--target-psnr excludes --bitrate, --vbv-bufsize and --qp-file"),
    (["--target-psnr", "37", "--bitrate", "500", "--vbv-bufsize", "100"], b"--target-psnr excludes --bitrate, --vbv-bufsize and --qp-file"),
    (["--target-psnr", "37", "--qp-file", "q.txt"], b"--target-psnr excludes --bitrate, --vbv-bufsize and --qp-file"),
    (["--max-recodes", "2"], b"--max-recodes needs --target-psnr"),
    (["--target-psnr", "37", "--max-recodes", "9"], b"Invalid max-recodes: 9 (0 .. 8)"),
    (["--target-psnr", "37", "--max-recodes", "-1"], b"Invalid max-recodes: -1"),
    (["--target-psnr", "37", "--max-recodes", "2x"], b"Invalid max-recodes: 2x"),
    (["--target-psnr", "0"], b"Invalid target-psnr: 0"),
    (["--target-psnr", "-3"], b"Invalid target-psnr: -3"),
    (["--target-psnr", "37dB"], b"Invalid target-psnr: 37dB"),
    (["--target-psnr", "nan"], b"Invalid target-psnr: nan"),
    (["--qp", "30", "--target-psnr"], b"option --target-psnr needs a value"),
])
def test_option_errors_of_both_front_ends(built, tmp_path, front, args, message):
    """Refused while the options are parsed: no device is opened, nothing is written."""
    import subprocess
    import sys
    (tmp_path / "q.txt").write_text("32 32\n")
    out = tmp_path / "o.vvc"
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    r = subprocess.run(cmd + ["-i", str(tmp_path / "missing.yuv"), "-o", str(out), "--input-size", "64x64", "--output-size", "64x64",
                              "--num-pictures", "2", "--qp", "32"] + args, cwd=ROOT, capture_output=True, timeout=60)
    assert r.returncode == 0 and b"error: " + message in r.stderr, r.stderr
    assert not out.exists() or out.stat().st_size == 0
