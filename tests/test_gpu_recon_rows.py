"""The row reconstruction of the search (dev_predict.h recon_row4: four samples per lane) on rows the test brings:
reconstruction bytes and squared error against the formula in NumPy (tests/pk16_model.py recon_rows), on 4,096 seeded
rows and on the corners of every argument (residuals -32,768 and 32,767 -- the ends of i16 --, +-255 and 0; prediction
and originals 0 and 255), each corner in every sample position and in all four at once."""
import numpy as np
import pytest

import pk16_model as m

pytestmark = pytest.mark.gpu


def _rows():
    rng = np.random.default_rng(1611)
    n = 4096
    pred, org = rng.integers(0, 256, (n, 4)), rng.integers(0, 256, (n, 4))
    res = rng.integers(-32768, 32768, (n, 4))
    res[: n // 2] = rng.integers(-300, 301, (n // 2, 4))      # the range a search produces
    # corners: every combination in every sample position, the other three samples of the row seeded
    cp, cr, co = np.meshgrid([0, 255], [-32768, 32767, -255, 255, 0], [0, 255], indexing="ij")
    k = cp.size
    pc, oc = rng.integers(0, 256, (4 * k, 4)), rng.integers(0, 256, (4 * k, 4))
    rc = rng.integers(-32768, 32768, (4 * k, 4))
    for pos in range(4):
        pc[pos * k:(pos + 1) * k, pos], rc[pos * k:(pos + 1) * k, pos], oc[pos * k:(pos + 1) * k, pos] = cp.ravel(), cr.ravel(), co.ravel()
    # ... and the same corner in all four samples at once (the largest SSD of a row: 4 x 255^2)
    pa, ra, oa = (np.repeat(a.reshape(-1, 1), 4, 1) for a in (cp, cr, co))
    pred = np.concatenate([pred, pc, pa]).astype(np.uint8)
    res = np.concatenate([res, rc, ra]).astype(np.int16)
    org = np.concatenate([org, oc, oa]).astype(np.uint8)
    return pred, res, org


def test_recon_rows_match_the_scalar_formula(built):
    from wrenc_amd import gpu
    pred, res, org = _rows()
    assert len(pred) % 64 != 0                   # a last wavefront of fewer rows
    want_rec, want_ssd = m.recon_rows(pred, res, org)
    assert want_ssd.max() == 4 * 255 * 255
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2)
    try:
        rec, ssd = enc.recon_rows(pred, res, org)
        one_rec, one_ssd = enc.recon_rows(pred[:1], res[:1], org[:1])
    finally:
        enc.close()
    bad = np.argwhere(rec != want_rec)
    assert len(bad) == 0, "row %d sample %d: pred %d res %d -> %d, want %d" % (
        bad[0][0], bad[0][1], pred[tuple(bad[0])], res[tuple(bad[0])], rec[tuple(bad[0])], want_rec[tuple(bad[0])])
    bad = np.flatnonzero(ssd != want_ssd)
    assert len(bad) == 0, "row %d: ssd %d, want %d" % (bad[0], ssd[bad[0]], want_ssd[bad[0]])
    assert np.array_equal(one_rec, want_rec[:1]) and np.array_equal(one_ssd, want_ssd[:1])
