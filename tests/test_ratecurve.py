"""The rate histogram on the host (include/wrenc_ratecurve.h, exported as wrenc_gpu_rate_hist_bin and _rate_hist_host)
against its restatement in Python (tests/ratecurve_ref.py), by hand-made blocks; and the curve include/wrenc_rate.h draws
from a histogram.  No device."""
import numpy as np
import pytest

import ratecurve_ref as rr
from content import content

EINVAL = -1
KINDS = ["flat", "ramp", "stripes0", "stripes30", "stripes90", "checker", "noise", "cclm", "extremes"]


def _picture(y):
    """A picture whose chroma planes are flat 128 (one DC coefficient of 0: all zeros) around the luma plane y."""
    h, w = y.shape
    return np.ascontiguousarray(y, np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)


def _both(pic):
    from wrenc_amd import gpu
    got, ref = gpu.rate_hist_host(*pic), rr.rate_hist(*pic)
    assert got.shape == (3, 64) and np.array_equal(got, ref), np.argwhere(got != ref)[:8].tolist()
    return got


def test_bin_boundaries(built):
    from wrenc_amd import gpu
    want = {0: 0, 1: 1, 2: 5, 3: 7, 4: 9, 5: 10, 6: 11, 7: 12, 8: 13, 15: 16, 16: 17, 8191: 52, 8192: 53, 16319: 56, 16320: 56}
    for m, b in want.items():
        assert gpu.rate_hist_bin(m) == b == rr.bin_of(m), m
    assert all(gpu.rate_hist_bin(m) == rr.bin_of(m) for m in range(0, 16321, 7))
    assert rr.TOP_BIN == 56 and [rr.bin_floor(b) for b in (0, 1, 5, 7, 9, 12, 13, 56)] == [0, 1, 2, 3, 4, 7, 8, 14336]
    for m in (-1, 16321, 1 << 20):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.rate_hist_bin(m)
        assert e.value.code == EINVAL


def test_a_flat_block_is_all_zeros(built):
    """Flat 128 everywhere: the first block is predicted as 128 and every other from equal neighbours."""
    got = _both(_picture(np.full((32, 32), 128, np.uint8)))
    assert got[:, 0].tolist() == [1024, 256, 256] and not got[:, 1:].any()
    # another flat value: the first block alone has its DC coefficient, 64 x (93 - 128)
    got = _both(_picture(np.full((32, 32), 93, np.uint8)))
    assert got[0, 0] == 1023 and got[0, rr.bin_of(64 * 35)] == 1


def test_the_checker_reaches_the_top_bin(built):
    pic = rr.checker8(32, 32)
    got = _both(pic)
    assert abs(rr.block_coefficients(pic[0], 1, 0)[0, 0]) == 16320 == rr.MAX_MAGNITUDE
    assert got[0, rr.TOP_BIN] == 15 and got[0, rr.bin_of(8192)] == 1 and got[0, 0] == 1024 - 16      # 64 x 128 in block 0
    assert got[1:, rr.TOP_BIN].tolist() == [3, 3]


def test_candidates_at_corners_and_edges(built):
    """A 24x24 corner of a 32x32 picture: rows grow downwards, so H (a row's own value to its left) predicts exactly where
    a left neighbour exists, V never fits, and DC is all a block on the left edge has besides it."""
    yy, xx = np.mgrid[0:32, 0:32]
    y = (8 * yy + 3).astype(np.uint8)          # constant along a row
    assert rr.predict(y, 0, 0)[0] == "DC"                                        # corner: 128 only
    assert rr.predict(y, 1, 0)[0] == "H" and rr.predict(y, 3, 0)[0] == "H"        # top edge: DC (of left) or H
    assert rr.predict(y, 0, 1)[0] == "DC" and rr.predict(y, 0, 3)[0] == "DC"      # left edge: DC (of top) or V; V = the row above, worse
    assert rr.predict(y, 2, 2)[0] == "H" and rr.predict(y, 3, 3)[0] == "H"        # inside and the far corner
    assert not rr.block_coefficients(y, 3, 3).any()
    _both(_picture(y))
    x = (8 * xx + 3).astype(np.uint8)          # constant along a column: V where a top neighbour exists
    assert [rr.predict(x, bx, by)[0] for bx, by in ((0, 0), (2, 0), (0, 2), (3, 1), (3, 3))] == ["DC", "DC", "V", "V", "V"]
    assert rr.predict(x, 0, 1)[1][0].tolist() == x[7, 0:8].tolist()
    _both(_picture(x))
    # the DC values: both neighbours, one, none
    rng = np.random.default_rng(3)
    n = rng.integers(0, 256, (32, 32), dtype=np.uint8)
    top, left = n[7, 8:16].astype(int), n[8:16, 7].astype(int)
    from wrenc_amd import gpu
    dcs = {(0, 0): 128, (1, 0): (n[0:8, 7].astype(int).sum() + 4) >> 3, (0, 1): (n[7, 0:8].astype(int).sum() + 4) >> 3,
           (1, 1): (top.sum() + left.sum() + 8) >> 4}
    for (bx, by), dc in dcs.items():
        m = n.copy()
        m[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = dc      # a block that equals its DC prediction: nothing but zeros
        assert rr.predict(m, bx, by)[0] == "DC" and not rr.block_coefficients(m, bx, by).any(), (bx, by)
        _both(_picture(m))


def test_a_sad_tie_goes_to_the_earlier_candidate(built):
    """The order is DC, V, H, and a later candidate needs a strictly smaller SAD: a tie of all three keeps DC, a tie of V and
    H below DC keeps V."""
    y = np.zeros((32, 32), np.uint8)
    y[8:16, 8:16] = 255
    name, pred = rr.predict(y, 1, 1)
    assert name == "DC" and not pred.any()
    assert rr.block_coefficients(y, 1, 1)[0, 0] == 16320
    _both(_picture(y))
    # again all three at 640: a block of 100 | 120 in halves under a row and beside a column of 110
    z = np.full((32, 32), 110, np.uint8)
    z[8:16, 8:12] = 100
    z[8:16, 12:16] = 120
    assert rr.predict(z, 1, 1)[0] == "DC"
    _both(_picture(z))
    # V strictly better than DC, H equal to V: V (the earlier of the two) is kept.  s(x, y) = 100 + a(x) + a(y) with a = 60 at
    # index 7 and 0 elsewhere, under a row above of 100 + a(x) and beside a column of 100 + a(y): SAD V = SAD H = 480, DC (108) 1232
    a = np.array([0, 0, 0, 0, 0, 0, 0, 60])
    v = np.full((32, 32), 100, np.uint8)
    v[7, 8:16] = 100 + a
    v[8:16, 7] = 100 + a
    v[8:16, 8:16] = 100 + a[None, :] + a[:, None]
    blk = v[8:16, 8:16].astype(int)
    sad = {"V": int(np.abs(blk - v[7, 8:16].astype(int)[None, :]).sum()), "H": int(np.abs(blk - v[8:16, 7].astype(int)[:, None]).sum()),
           "DC": int(np.abs(blk - 108).sum())}
    assert sad == {"V": 480, "H": 480, "DC": 1232}
    assert rr.predict(v, 1, 1)[0] == "V"
    _both(_picture(v))


@pytest.mark.parametrize("w,h", [(32, 32), (96, 64), (352, 288)])
def test_counts_add_up_to_the_samples(built, w, h):
    for kind in ("noise", "cclm", "extremes"):
        got = _both(content(kind, w, h, 2))
        assert got.sum(axis=1).tolist() == [w * h, w * h // 4, w * h // 4] and not got[:, 57:].any()


def test_the_curve_does_not_rise_with_the_qp(built):
    from wrenc_amd import rate
    for kind in KINDS:
        hist = rr.rate_hist(*content(kind, 96, 64, 1))
        p = rate.curve(hist)
        assert p.shape == (64,) and np.all(np.diff(p) <= 0) and p[0] >= 0, kind
        assert np.allclose(p, rr.curve(hist), rtol=1e-12, atol=0), kind
        if kind != "flat":
            assert p[0] > p[63], kind
    assert (rate.CURVE_DEAD, rate.CURVE_TAIL, rate.CURVE_BITS0, rate.CURVE_BITS1, rate.CURVE_CHROMA_WEIGHT) == (
        rr.DEAD, rr.TAIL, rr.BITS0, rr.BITS1, rr.CHROMA_WEIGHT)


def test_host_entry_points_refuse_bad_arguments(built):
    from wrenc_amd import gpu, rate
    good = rr.flat(32, 32)
    gpu.rate_hist_host(*good)
    for planes in ((good[0][:, :24], good[1], good[2]),                    # a width that is no multiple of 16
                   (good[0], good[1][:8], good[2]),                         # a chroma plane of the wrong size
                   (good[0].ravel(), good[1], good[2]),                     # not a plane
                   (np.zeros((8, 8), np.uint8), np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8))):   # below 16
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.rate_hist_host(*planes)
        assert e.value.code == EINVAL
    lib = gpu.load_library()
    assert lib.wrenc_gpu_rate_hist_host(32, 32, None, None, None, None) == EINVAL
    with pytest.raises(rate.RateError):
        rate.curve(np.zeros((3, 63), np.uint64))
    with pytest.raises(rate.RateError):
        rate.curve(np.zeros((2, 3, 64), np.uint64))
