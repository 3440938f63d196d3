"""include/wrenc_recon.h restated in numpy: the output formats of the reconstruction, the centre-sited bilinear chroma in
sixteenths, the integer conversion to RGB and the frame layouts.  Shared by test_recon.py (which holds the library's host
converter against it) and the GPU tests (which hold the device against it)."""
import math
from fractions import Fraction

import numpy as np

RGB24, BGR24, RGB0, BGR0, GBRP, YUV420P, NV12 = range(7)
NAMES = ("rgb24", "bgr24", "rgb0", "bgr0", "gbrp", "yuv420p", "nv12")
ALIASES = {"rgba": RGB0, "bgra": BGR0}
BT709, BT601 = 0, 1
TV, PC = 0, 1
K = {BT709: (Fraction(2126, 10000), Fraction(722, 10000)), BT601: (Fraction(299, 1000), Fraction(114, 1000))}   # Kr, Kb
SCALE = {TV: (Fraction(219, 255), Fraction(224, 255), 16), PC: (Fraction(1), Fraction(1), 0)}                   # sy, sc, yoff


def is_rgb(fmt):
    return fmt <= GBRP


def _round(x):
    """Nearest integer of a rational (no coefficient of the header lies on a tie)."""
    assert x.denominator == 1 or (2 * x).denominator != 1
    return math.floor(x + Fraction(1, 2))


def coefficients(matrix, rng):
    """[cy, rv, gu, gv, bu, yoff] by the header's rule, in exact rationals."""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    sy, sc, yoff = SCALE[rng]
    one = 1 << 14
    return [_round(one / sy), _round(2 * (1 - kr) / sc * one), _round(-2 * kb * (1 - kb) / (kg * sc) * one),
            _round(-2 * kr * (1 - kr) / (kg * sc) * one), _round(2 * (1 - kb) / sc * one), yoff]


def real_coefficients(matrix, rng):
    """The real-valued formula's (1 / sy, rv, gu, gv, bu, yoff) as floats."""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    sy, sc, yoff = SCALE[rng]
    return [float(1 / sy), float(2 * (1 - kr) / sc), float(-2 * kb * (1 - kb) / (kg * sc)), float(-2 * kr * (1 - kr) / (kg * sc)),
            float(2 * (1 - kb) / sc), yoff]


def chroma16(c):
    """A ch x cw chroma plane -> the 2ch x 2cw plane of sixteenths at the luma positions (int64)."""
    c = np.asarray(c).astype(np.int64)
    ch, cw = c.shape
    x, y = np.arange(2 * cw), np.arange(2 * ch)
    i, j = x >> 1, y >> 1
    i2 = np.clip(i + np.where(x & 1, 1, -1), 0, cw - 1)
    j2 = np.clip(j + np.where(y & 1, 1, -1), 0, ch - 1)
    return 9 * c[j][:, i] + 3 * c[j][:, i2] + 3 * c[j2][:, i] + c[j2][:, i2]


def accumulators(k, y, cb16, cr16):
    """The three sums in front of the shift (int64: the caller checks that they fit 32 bits)."""
    y, cb16, cr16 = (np.asarray(a).astype(np.int64) for a in (y, cb16, cr16))
    yd, u, v = 16 * (y - k[5]), cb16 - 2048, cr16 - 2048
    base = k[0] * yd + (1 << 17)
    return base + k[1] * v, base + k[2] * u + k[3] * v, base + k[4] * u


def rgb_unclipped(k, y, cb16, cr16):
    return tuple(a >> 18 for a in accumulators(k, y, cb16, cr16))        # numpy's >> of a signed integer is the floor shift


def rgb(matrix, rng, y, cb, cr):
    """The visible planes -> an (h, w, 3) uint8 array R, G, B."""
    k = coefficients(matrix, rng)
    return np.stack([np.clip(a, 0, 255) for a in rgb_unclipped(k, y, chroma16(cb), chroma16(cr))], axis=2).astype(np.uint8)


def layout(fmt, w, h):
    """[(rows, row_bytes)] of the planes of a tightly packed frame."""
    if fmt in (RGB24, BGR24):
        return [(h, 3 * w)]
    if fmt in (RGB0, BGR0):
        return [(h, 4 * w)]
    if fmt == GBRP:
        return [(h, w)] * 3
    if fmt == YUV420P:
        return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    assert fmt == NV12
    return [(h, w), (h // 2, w)]


def convert(fmt, matrix, rng, y, cb, cr):
    """The planes of output format `fmt`, tightly packed 2-D uint8 arrays as the layout numbers them."""
    y, cb, cr = (np.asarray(a, np.uint8) for a in (y, cb, cr))
    h, w = y.shape
    assert cb.shape == cr.shape == (h // 2, w // 2)
    if fmt == YUV420P:
        return [y.copy(), cb.copy(), cr.copy()]
    if fmt == NV12:
        return [y.copy(), np.stack([cb, cr], axis=2).reshape(h // 2, w)]
    p = rgb(matrix, rng, y, cb, cr)
    if fmt == GBRP:
        return [np.ascontiguousarray(p[:, :, c]) for c in (1, 2, 0)]
    if fmt in (BGR24, BGR0):
        p = p[:, :, ::-1]
    if fmt in (RGB0, BGR0):
        p = np.concatenate([p, np.full((h, w, 1), 255, np.uint8)], axis=2)
    return [np.ascontiguousarray(p).reshape(h, -1)]


def crop(planes, w, h):
    """The visible planes of coded-size planes."""
    return planes[0][:h, :w], planes[1][:h // 2, :w // 2], planes[2][:h // 2, :w // 2]


def noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


def corners(w, h):
    """Extreme (Y, Cb, Cr) in blocks of 2 x 2 chroma samples: every combination of 0 / 255 (and some mid values) next to
    every other, so that R, G and B clip at both ends and the bilinear steps are the largest there are."""
    vals = np.array([0, 255, 128, 16, 240, 1, 254, 235], np.uint8)
    jj, ii = np.indices((h // 2, w // 2))
    cb = vals[((ii // 2) + 3 * (jj // 2)) % 8]
    cr = vals[((ii // 2) * 5 + (jj // 2) + 1) % 8]
    yy, xx = np.indices((h, w))
    y = vals[(xx // 3 + yy // 3 * 7) % 8]
    return y, cb, cr


def with_margin(vis, coded_w, coded_h, seed=99):
    """Visible planes inside coded-size planes whose margin is UNLIKE the visible edge: where the edge sample is below 128 the
    margin is 255 less a little noise, else a little noise -- a kernel that reads the margin for an edge pixel is far off."""
    rng = np.random.default_rng(seed)
    out = []
    for p, plane in enumerate(vis):
        cw, ch = (coded_w, coded_h) if p == 0 else (coded_w // 2, coded_h // 2)
        h, w = plane.shape
        big = np.zeros((ch, cw), np.uint8)
        big[:h, :w] = plane
        if w < cw:
            big[:h, w:] = np.where(plane[:, -1:] < 128, 255, 0) ^ rng.integers(0, 8, (h, cw - w), dtype=np.uint8)
        if h < ch:
            big[h:, :] = np.where(big[h - 1:h, :] < 128, 255, 0) ^ rng.integers(0, 8, (ch - h, cw), dtype=np.uint8)
        out.append(big)
    return tuple(out)
