"""The buffer model of the rate controller (include/wrenc_rate.h: wrenc_rate_enable_vbv, _choose_vbv, _vbv_allowance,
_recode) through wrenc_amd/rate.py, on synthetic histograms and made-up sizes: no device, no pictures."""
import ctypes as C

import numpy as np
import pytest

W, H, CTUS = 352, 288, 11 * 9
TARGET = 4000.0                       # bytes per picture: R = 32,000 bits
HEADER = 120.0


def _hist(spread, seed=0):
    """A (3, 64) histogram of a W x H picture: log-magnitudes around `spread` bins, a third of the coefficients zero."""
    rng = np.random.default_rng(seed)
    out = np.zeros((3, 64), np.uint64)
    occupied = [b for b in range(1, 57) if b not in (2, 3, 4, 6, 8)]
    for p, n in enumerate((W * H, W * H // 4, W * H // 4)):
        weights = np.exp(-0.5 * ((np.array(occupied) - spread) / 6.0) ** 2) * rng.uniform(0.8, 1.2, len(occupied))
        counts = np.floor(weights / weights.sum() * (n * 2 // 3)).astype(np.uint64)
        out[p, occupied] = counts
        out[p, 0] = n - int(counts.sum())
    return out


def _controller(bufsize=None, num=64, qp_max=63, header=HEADER, target=TARGET):
    from wrenc_amd import rate
    rc = rate.Controller(W, H, target, num, qp_max=qp_max, header_bytes=header)
    if bufsize is not None:
        rc.enable_vbv(bufsize)
    return rc


def _predict(hist, qp, a=None):
    from wrenc_amd import rate
    pa, pc = rate.curve_prior()
    return (pa if a is None else a) * rate.curve(hist)[qp] + pc * CTUS


def _run(sizes_of):
    """Six batches of four pictures, smooth then busy; sizes_of(hist, qp, index) makes the bytes.  Returns everything asked
    and answered."""
    rc = _controller(bufsize=4 * 8 * TARGET)
    log, index = [], 0
    for b in range(6):
        hists = np.stack([_hist(16 if b < 3 else 30, seed=4 * b + k) for k in range(4)])
        qps, allow = rc.choose_vbv(hists, allowances=True)
        log.append(("qp", qps, allow))
        for k, q in enumerate(qps):
            state = rc.vbv_allowance()
            nbytes = sizes_of(hists[k], q, index)
            log.append(("allowance", state["allowance"], state["fullness"], nbytes))
            assert state["bufsize"] == 4 * 8 * TARGET
            rc.report([nbytes])
            index += 1
    rc.close()
    return log


def test_the_same_calls_give_the_same_answers(built):
    sizes = lambda h, q, i: int(_predict(h, q) * (1.0 + 0.3 * np.sin(i)))
    first, second = _run(sizes), _run(sizes)
    assert first == second
    qps = [q for e in first if e[0] == "qp" for q in e[1]]
    assert len(set(qps)) > 2 and all(0 <= q <= 63 for q in qps)


def test_sizes_as_predicted_never_violate_the_bucket(built):
    """The reports equal the predictions the QPs were chosen by (a stays the prior): every picture fits its allowance, the
    walk's expected allowance is the real one, and the bucket never holds more than B."""
    log = _run(lambda h, q, i: int(_predict(h, q)))
    expected = [a for e in log if e[0] == "qp" for a in e[2]]
    seen = [e for e in log if e[0] == "allowance"]
    assert len(expected) == len(seen) == 24
    for i, (want, (_, allowance, fullness, nbytes)) in enumerate(zip(expected, seen)):
        assert 8 * nbytes <= allowance, i                       # no re-encode would be asked for
        assert allowance == fullness - (8 * HEADER if i == 0 else 0)
        assert fullness <= 4 * 8 * TARGET
        assert abs(want - allowance) <= 8.0 * 24, (i, want, allowance)        # (the reports are whole bytes: < 1 byte a picture)


def test_the_bucket_follows_the_reports(built):
    rc = _controller(bufsize=100000.0)
    rc.choose_vbv(np.stack([_hist(20, k) for k in range(3)]))
    assert rc.vbv_allowance() == {"allowance": 100000.0 - 8 * HEADER, "bufsize": 100000.0, "fullness": 100000.0}
    rc.report([5000])                                            # F1 = min(B, B - 8 (5000 + 120) + R)
    assert rc.vbv_allowance()["fullness"] == 100000.0 - 8 * 5120 + 8 * TARGET == rc.vbv_allowance()["allowance"]
    rc.report([100])                                             # refills, capped at B
    assert rc.vbv_allowance()["fullness"] == 100000.0
    rc.report([20000])                                           # a violation is taken out all the same: F goes on from it
    assert rc.vbv_allowance()["fullness"] == 100000.0 - 160000.0 + 8 * TARGET
    rc.close()


def test_a_picture_at_three_times_its_prediction_is_coded_again_higher(built):
    from wrenc_amd import rate
    rc = _controller(bufsize=2 * 8 * TARGET)
    hist = _hist(30, 5)
    qp = rc.choose_vbv(hist[None])[0]
    allowance = rc.vbv_allowance()["allowance"]
    predicted = _predict(hist, qp)
    assert 8 * predicted <= rate.VBV_SAFETY * allowance
    actual = int(3 * predicted)
    assert 8 * actual > allowance                                # the input is one where enforcement matters
    again = rc.recode(actual, allowance)
    assert qp < again <= 63
    # by the picture's own curve, scaled by actual / predicted, the new QP fits and the one below it does not
    scale = actual / predicted
    assert 8 * scale * _predict(hist, again) <= rate.VBV_SAFETY * allowance
    assert again == qp + 1 or 8 * scale * _predict(hist, again - 1) > rate.VBV_SAFETY * allowance
    # the picture now stands at that QP: the same miss again goes higher still
    third = rc.recode(int(3 * _predict(hist, again)), allowance)
    assert third > again
    rc.report([int(_predict(hist, third))])
    with pytest.raises(rate.RateError):                          # nothing outstanding
        rc.recode(1000, allowance)
    rc.close()


def test_qp_max_pins(built):
    rc = _controller(bufsize=8 * TARGET, qp_max=40, target=TARGET)
    hist = _hist(44, 1)                                          # far beyond the target at QP 40
    assert _predict(hist, 40) > TARGET
    qp = rc.choose_vbv(np.stack([hist, hist]))
    assert qp == [40, 40]
    assert rc.recode(int(_predict(hist, 40)), 1000.0) == 40      # at the bound already: the same QP back
    rc.close()
    rc = _controller(bufsize=8 * TARGET, qp_max=40)
    qp = rc.choose_vbv(_hist(24, 2)[None])[0]
    assert qp < 40 and rc.recode(10 ** 7, 8.0) == 40             # nothing fits: the bound
    rc.close()


def test_refusals(built):
    from wrenc_amd import rate
    lib = rate._lib()
    hist = _hist(20)
    satd = np.array([[10 ** 6, 10 ** 5, 10 ** 5]], np.uint64)
    for bad in (8 * TARGET - 1, 0.0, -5.0, float("nan"), float("inf")):      # below R; not a size
        with pytest.raises(rate.RateError):
            _controller(bufsize=bad)
    with pytest.raises(rate.RateError):                                      # does not hold the parameter sets
        _controller(bufsize=8 * TARGET, header=TARGET)
    rc = _controller()                                                       # no buffer model: its calls are refused
    with pytest.raises(rate.RateError):
        rc.choose_vbv(hist[None])
    with pytest.raises(rate.RateError):
        rc.vbv_allowance()
    with pytest.raises(rate.RateError):
        rc.recode(1000, 1000.0)
    rc.choose(satd)
    with pytest.raises(rate.RateError):                                      # pictures already chosen
        rc.enable_vbv(10 * 8 * TARGET)
    rc.close()
    rc = _controller(bufsize=10 * 8 * TARGET)
    with pytest.raises(rate.RateError):                                      # with the model the complexity chooser is refused
        rc.choose(satd)
    with pytest.raises(rate.RateError):
        rc.choose_vbv(np.zeros((1, 3, 32), np.uint64))
    with pytest.raises(rate.RateError):
        rc.recode(1000, 1000.0)                                              # nothing chosen yet
    qp = np.zeros(1, np.int32)
    assert lib.wrenc_rate_choose_vbv(rc.rc, 0, hist.ctypes.data, qp.ctypes.data, None) == -1
    assert lib.wrenc_rate_choose_vbv(rc.rc, 1, None, qp.ctypes.data, None) == -1
    assert lib.wrenc_rate_choose_vbv(rc.rc, 1, hist.ctypes.data, None, None) == -1
    assert lib.wrenc_rate_choose_vbv(None, 1, hist.ctypes.data, qp.ctypes.data, None) == -1
    assert lib.wrenc_rate_enable_vbv(None, 1e6) == -1 and lib.wrenc_rate_vbv_allowance(None, None, None, None) == -1
    assert lib.wrenc_rate_curve(None, None) == -1
    rc.choose_vbv(hist[None])
    with pytest.raises(rate.RateError):
        rc.recode(0, 1000.0)
    with pytest.raises(rate.RateError):
        rc.recode(1000, float("nan"))
    with pytest.raises(rate.RateError):
        rc.report([1, 2])                                                    # more than are outstanding
    rc.close()


def test_without_a_buffer_the_complexity_chooser_is_the_parent_commits(built):
    """One fixed call sequence -- six batches of eight, a report one batch behind -- and the QPs the commit before the
    buffer model gave for it."""
    rc = _controller(num=48, header=120.0, target=5000.0)
    got, pend = [], []
    for b in range(6):
        satd = np.array([[(900000 + 70000 * ((7 * b + k) % 5)) * (1 if b < 3 else 4), 90000 + 1000 * k, 80000 + 500 * b] for k in range(8)], np.uint64)
        qp = rc.choose(satd)
        got.append(qp)
        pend.append((b, qp))
        if len(pend) == 2:
            pb, pq = pend.pop(0)
            rc.report([int(60000 * (1 if pb < 3 else 3) * 2.0 ** (-q / 6.0)) + 40 * k for k, q in enumerate(pq)])
    rc.close()
    assert got == [[13, 13, 13, 13, 14, 14, 14, 14], [14, 14, 14, 14, 14, 14, 14, 14], [37, 37, 38, 38, 38, 38, 38, 38],
                   [48, 48, 48, 48, 49, 49, 49, 49], [47, 47, 47, 48, 48, 48, 48, 48], [42, 42, 43, 43, 43, 43, 43, 43]]
