"""The rate controller (include/wrenc_rate.h, wrenc_amd/csrc/host/rate_control.cpp) against a synthetic encoder whose
bytes follow the controller's model form, bytes = K a N (C / N)^b 2^(-qp / step): b the prior's, K a quarter and four
times the prior's scale, step 6 QPs per factor two -- and, second, the prior's own s, the form exact in every constant.
The prior's s is fitted and need not be 6, so "K times the prior" can hold at one QP only: at the QP at which the prior
predicts the run's target, where the batches chosen without feedback run (the anchor of _scale below).  Nothing here
needs a GPU.  Reports arrive two batches late, as in the native program's pipeline
(batch k is reported before batch k + 2 is chosen), so two batches of every run are chosen on the prior alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 352, 288
N = W * H
BATCHES, BATCH, LAG = 8, 16, 2
HALF_STEP = 2.0 ** (1.0 / 12.0)      # half a QP step of the synthetic encoder: what the best constant QP guarantees


def _complexities(seed=3):
    """(BATCHES * BATCH, 3) plane sums: weighted sums log-uniform over a factor 10 around 6 per sample, chroma a sixth."""
    rng = np.random.default_rng(seed)
    per_sample = 6.0 * 10.0 ** rng.uniform(-0.5, 0.5, BATCHES * BATCH)
    total = per_sample * N
    return np.stack([total * 4 / 6, total / 6, total / 6], axis=1).astype(np.uint64)


def _units(satd, b):
    from wrenc_amd import rate
    c = satd[:, 0].astype(np.float64) + rate.CHROMA_WEIGHT * (satd[:, 1].astype(np.float64) + satd[:, 2].astype(np.float64))
    return N * (c / N) ** b


def _scale(k_factor, anchor, step):
    """The synthetic encoder's scale: K times the prior's prediction at QP `anchor`, from where it moves in its own steps."""
    from wrenc_amd import rate
    a, _, s = rate.prior()
    step = step or s
    return k_factor * a * 2.0 ** (-anchor / s + anchor / step), step


def _run(k_factor, target, qp_min=0, qp_max=63, seed=3, anchor=32.0, step=6.0):
    """One run of the synthetic encoder under the controller: (QPs per batch, bytes per picture)."""
    from wrenc_amd import rate
    _, b, _ = rate.prior()
    scale, step = _scale(k_factor, anchor, step)
    satd = _complexities(seed)
    unit = _units(satd, b)
    ctl = rate.Controller(W, H, target, BATCHES * BATCH, qp_min, qp_max)
    qps, nbytes = [], []
    for j in range(BATCHES):
        if j >= LAG:
            ctl.report(nbytes[j - LAG])
        sl = slice(j * BATCH, (j + 1) * BATCH)
        q = ctl.choose(satd[sl])
        qps.append(q)
        nbytes.append(np.rint(scale * unit[sl] * 2.0 ** (-np.array(q) / step)).astype(np.uint64))
    for j in range(BATCHES - LAG, BATCHES):
        ctl.report(nbytes[j])
    with pytest.raises(rate.RateError):
        ctl.report([1])                                    # nothing outstanding any more
    ctl.close()
    return qps, np.concatenate(nbytes)


def _target_at(k_factor, qp, anchor=32.0, step=6.0):
    """Bytes per picture the synthetic encoder makes at a constant QP."""
    from wrenc_amd import rate
    scale, step = _scale(k_factor, anchor, step)
    return float(np.mean(scale * _units(_complexities(), rate.prior()[1]) * 2.0 ** (-qp / step)))


def _prior_target(qp):
    """Bytes per picture the PRIOR predicts at a constant QP."""
    from wrenc_amd import rate
    a, b, s = rate.prior()
    return float(np.mean(a * _units(_complexities(), b) * 2.0 ** (-qp / s)))


# The two feedback-free batches are a quarter of the run and miss by the factor K, so the other six need room inside
# 0..63 to make up for it.  K = 4: the first quarter alone spends the whole run's bytes and the rest must go to the top
# of the range, so the prior's QP is 10 (the encoder's: 10 + 6 log2 4 = 22); K = 1/4: the prior's QP is 52 (the encoder's 40).
@pytest.mark.parametrize("step", [6.0, None], ids=["step6", "prior_s"])
@pytest.mark.parametrize("k_factor,prior_qp", [(0.25, 52.0), (4.0, 10.0), (0.25, 42.5), (1.0, 33.3)])
def test_total_lands_within_half_a_qp_step(built, k_factor, prior_qp, step):
    target = _prior_target(prior_qp)
    qps, nbytes = _run(k_factor, target, anchor=prior_qp, step=step)
    ratio = float(nbytes.sum()) / (target * BATCHES * BATCH)
    print("K = %g: total / target = %.4f, QPs per batch %s" % (k_factor, ratio, [sorted(set(q)) for q in qps]))
    assert 1.0 / HALF_STEP < ratio < HALF_STEP, ratio
    for q in qps:
        assert len(q) == BATCH and all(0 <= v <= 63 for v in q)
        assert max(q) - min(q) <= 1, q                      # one QP, or two adjacent ones
        assert q == sorted(q)                              # q first, q + 1 from the split on


def test_qp_range_is_kept_and_pins(built):
    """A target 100 times what the range can spend pins qp_min, one 100 times below what it must spend pins qp_max."""
    lo, hi = 20, 40
    for k_factor in (0.25, 4.0):
        qps, _ = _run(k_factor, 100.0 * _target_at(k_factor, lo), lo, hi)
        assert all(v == lo for q in qps for v in q), qps
        qps, _ = _run(k_factor, 0.01 * _target_at(k_factor, hi), lo, hi)
        assert all(v == hi for q in qps for v in q), qps
        qps, _ = _run(k_factor, _target_at(k_factor, 30.0), lo, hi)
        assert all(lo <= v <= hi for q in qps for v in q), qps
    qps, _ = _run(1.0, _target_at(1.0, 31.0), 31, 31)      # a range of one QP
    assert all(v == 31 for q in qps for v in q)


def test_same_calls_same_qps(built):
    target = _target_at(4.0, 22.0)
    first, b1 = _run(4.0, target)
    second, b2 = _run(4.0, target)
    assert first == second and np.array_equal(b1, b2)
    other, _ = _run(4.0, target, seed=4)                   # (and the QPs do depend on the complexities)
    assert other != first


def test_feed_forward_follows_complexity(built):
    """With no report at all, a batch ten times as complex gets the higher QP: the prediction, not feedback, moves it."""
    from wrenc_amd import rate
    satd = _complexities()
    target = _target_at(1.0, 30.0)
    ctl = rate.Controller(W, H, target, 10 * BATCH)
    easy = ctl.choose(satd[:BATCH])
    hard = ctl.choose(satd[:BATCH] * np.uint64(10))
    ctl.close()
    assert min(hard) > max(easy), (easy, hard)


def test_bad_arguments(built):
    from wrenc_amd import rate
    for kw in (dict(qp_min=-1), dict(qp_max=64), dict(qp_min=40, qp_max=39), dict(num_pictures=0), dict(target_bytes=0.0),
               dict(target_bytes=float("nan")), dict(width=0), dict(header_bytes=-1.0)):
        args = dict(width=W, height=H, target_bytes=1000.0, num_pictures=10, qp_min=0, qp_max=63, header_bytes=0.0)
        args.update(kw)
        with pytest.raises(rate.RateError):
            rate.Controller(**args)
    ctl = rate.Controller(W, H, 1000.0, 10)
    with pytest.raises(rate.RateError):
        ctl.report([5])                                    # nothing chosen yet
    ctl.close()


def test_header_and_symbols(built):
    """Every function the header declares is exported by the host library and listed in bitstream.py, and nothing else is."""
    from wrenc_amd import bitstream, rate
    header = open(os.path.join(ROOT, "include", "wrenc_rate.h")).read()
    declared = sorted(set(re.findall(r"\b(wrenc_rate_[a-z_]+)\s*\(", header)))
    assert declared == sorted(bitstream.EXPORTED_RATE_SYMBOLS) and len(declared) == 5
    lib = C.CDLL(bitstream.LIB_PATH)
    for name in declared:
        assert getattr(lib, name)
    assert C.sizeof(rate.Config) == 40
    assert "#define WRENC_RATE_WINDOW %d\n" % rate.WINDOW in header
    assert "#define WRENC_RATE_CHROMA_WEIGHT %r\n" % rate.CHROMA_WEIGHT in header
    a, b, s = rate.prior()
    assert a > 0 and 0.5 < b < 2.5 and 3.0 < s < 12.0
