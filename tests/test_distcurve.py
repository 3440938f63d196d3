"""The distortion curve on the host (include/wrenc_distcurve.h, exported as wrenc_gpu_dist_curve_host) against its
restatement in Python (tests/distcurve_ref.py): closed cases worked out by hand, structured and random pictures.  No
device."""
import numpy as np
import pytest

import distcurve_ref as dr
import ratecurve_ref as rr
from content import content

EINVAL = -1
KINDS = ["flat", "ramp", "stripes0", "stripes30", "stripes90", "checker", "noise", "cclm", "extremes"]


def _picture(y):
    """A picture whose chroma planes are flat 128 (no coefficient at all) around the luma plane y."""
    h, w = y.shape
    return np.ascontiguousarray(y, np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8)


def _both(pic):
    from wrenc_amd import gpu
    got, ref = gpu.dist_curve_host(*pic), dr.dist_curve(*pic)
    assert got.shape == (3, 64) and got.dtype == np.uint64
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8].tolist()
    return got


def test_a_flat_picture_is_all_zeros(built):
    """Flat 128 everywhere: the first block is predicted as 128 and every other from equal neighbours: no coefficient, no
    error at any QP."""
    got = _both(_picture(np.full((32, 32), 128, np.uint8)))
    assert not got.any()


def test_a_single_coefficient_by_hand(built):
    """Flat 93: the first block alone has a coefficient, its DC 64 x (93 - 128) = -2240, m = 17,920."""
    got = _both(_picture(np.full((32, 32), 93, np.uint8)))
    assert not got[1:].any()
    m = 8 * 2240
    # the steps the hand values below stand on: 64 x 2^((q - 4) / 6) to within 1 %, the largest error below 2^15
    assert [dr.step(q) for q in (0, 1, 2, 3, 4, 5, 6, 10, 63)] == [40, 45, 51, 57, 64, 72, 80, 128, 57 << 10]
    assert all(abs(dr.step(q) / (64.0 * 2.0 ** ((q - 4) / 6.0)) - 1.0) < 0.01 for q in range(64))
    assert dr.step(63) // 2 == 29184 and 29184 ** 2 < 1 << 30
    # q = 0: T = 40 divides m.  q = 4: T = 64 divides m.  q = 22: T = 64 << 3 = 512 = m / 35.
    assert got[0, 0] == 0 and got[0, 4] == 0 and got[0, 22] == 0
    # q = 1: T = 45, l = (17,920 + 22) / 45 = 398, e = 17,920 - 17,910 = 10
    assert got[0, 1] == 10 * 10
    # q = 29: T = 72 << 4 = 1152, l = (17,920 + 576) / 1152 = 16, e = 17,920 - 18,432 = -512: rounded up, |e| <= T / 2
    assert got[0, 29] == 512 * 512
    # q = 59: T = 72 << 9 = 36,864 > 2 m - 1: l = (17,920 + 18,432) / 36,864 = 0, e = m: the "min" form's other branch
    assert got[0, 59] == m * m
    # q = 58: T = 64 << 9 = 32,768, l = (17,920 + 16,384) / 32,768 = 1, e = 17,920 - 32,768 = -14,848
    assert got[0, 58] == 14848 * 14848
    for q in range(64):
        t = dr.step(q)
        assert got[0, q] <= min(m, t // 2) ** 2, q


def test_the_checker_reaches_the_magnitude_bound(built):
    """0 / 255 squares: every block but the first has the one coefficient 64 x 255, m = 130,560, the largest there is."""
    pic = rr.checker8(32, 32)
    got = _both(pic)
    assert abs(rr.block_coefficients(pic[0], 1, 0)[0, 0]) == 16320
    big = dr.errors([16320])[0]
    first = dr.errors([8192])[0]              # block 0: 64 x (0 - 128)
    assert got[0].tolist() == (15 * big * big + first * first).tolist()
    assert (np.abs(big) <= dr.STEPS // 2).all()


@pytest.mark.parametrize("kind", KINDS)
def test_content_against_numpy(built, kind):
    got = _both(content(kind, 96, 64, 1))
    # no error exceeds half a step or the coefficient itself
    samples = np.array([96 * 64, 48 * 32, 48 * 32], np.float64)[:, None]
    assert (got.astype(np.float64) <= samples * (dr.STEPS[None, :] // 2) ** 2).all()


def test_random_pictures_and_sizes(built):
    for k, (w, h) in enumerate(((16, 16), (48, 16), (16, 48), (64, 32))):
        _both(rr.noise(w, h, 11 + k))


def test_the_curve_predicts_the_quantisers_error(built):
    """sse8 / 4096 is a sample-domain SSE: for noise at a mid QP it is what a uniform quantiser of step T / 64 per sample
    leaves, T^2 / 12 per coefficient in the units of m (within a few per cent when most coefficients exceed the step)."""
    pic = rr.noise(64, 64, 3)
    got = _both(pic)
    q = 22
    assert got[0, q] / (64 * 64) == pytest.approx(dr.step(q) ** 2 / 12.0, rel=0.05)


def test_arguments(built):
    from wrenc_amd import gpu
    good = rr.noise(32, 32, 1)
    gpu.dist_curve_host(*good)
    for planes in ((good[0][:, :24], good[1], good[2]), (good[0], good[1][:8], good[2]), (good[0][0], good[1], good[2]),
                   (np.zeros((8, 8), np.uint8), np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8)),
                   (np.zeros((24, 32), np.uint8), np.zeros((12, 16), np.uint8), np.zeros((12, 16), np.uint8))):
        with pytest.raises(gpu.WrencGpuError):
            gpu.dist_curve_host(*planes)
    lib = gpu.load_library()
    assert lib.wrenc_gpu_dist_curve_host(32, 32, None, None, None, None) == EINVAL
