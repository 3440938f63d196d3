"""Reference side of the scaling tests: the filter of include/wrenc_scale.h restated in Python -- the taps in Python
ints, applied with numpy in int64 -- and the sizes and pictures the tests share."""
import functools

import numpy as np

from content import content

UNITY = 4096

# n_in -> n_out of one axis: the tap tables are compared for every output index of each
AXIS_PAIRS = [(3840, 1920), (2160, 1080), (3840, 1280), (8192, 2050), (960, 1920), (70, 34), (50, 62), (35, 17), (17, 47),
              (64, 16), (16, 64), (100, 100)]

# source -> visible (coded): 2:1 (8 taps); 4:1 (16 taps, the limit); x4 up (4 taps); a non-integer ratio with chroma widths
# 35 -> 17 and a margin to pad; shrinking in x while growing in y; identity
SIZES = [((64, 64), (32, 32), (32, 32)), ((128, 128), (32, 32), (32, 32)), ((16, 16), (64, 64), (64, 64)),
         ((70, 50), (34, 30), (64, 32)), ((96, 32), (62, 34), (64, 64)), ((64, 64), (64, 64), (64, 64))]
SIZE_IDS = ["%dx%d-%dx%d" % (s + v) for s, v, _ in SIZES]


def taps(n_in, n_out, o):
    """(first input index, [coefficients]) of output sample o; the indices may lie outside [0, n_in - 1]."""
    assert 0 < n_in <= 4 * n_out and 0 < n_out <= 4 * n_in and 0 <= o < n_out
    D, C, M = 2 * n_out, (2 * o + 1) * n_in - n_out, 2 * max(n_in, n_out)
    idx = [i for i in range((C - 2 * M) // D - 2, (C + 2 * M) // D + 3) if abs(i * D - C) < 2 * M]
    assert idx == list(range(idx[0], idx[-1] + 1))
    W = []
    for i in idx:
        N = abs(i * D - C)
        W.append(3 * N ** 3 - 5 * N ** 2 * M + 2 * M ** 3 if N < M else -N ** 3 + 5 * N ** 2 * M - 8 * N * M ** 2 + 4 * M ** 3)
    T = sum(W)
    assert T > 0
    k = [(8192 * w + T) // (2 * T) for w in W]
    k[W.index(max(W))] += UNITY - sum(k)        # list.index: the lowest i on a tie
    while len(k) > 1 and k[0] == 0:             # zero coefficients at the ends are not listed
        idx, k = idx[1:], k[1:]
    while len(k) > 1 and k[-1] == 0:
        idx, k = idx[:-1], k[:-1]
    return idx[0], k


@functools.lru_cache(maxsize=None)
def axis_tables(n_in, n_out):
    """(first[n_out], coef[n_out, taps]) as int64 arrays, the shorter lists padded with zero coefficients."""
    rows = [taps(n_in, n_out, o) for o in range(n_out)]
    width = max(len(k) for _, k in rows)
    first = np.array([f for f, _ in rows], np.int64)
    coef = np.zeros((n_out, width), np.int64)
    for o, (_, k) in enumerate(rows):
        coef[o, :len(k)] = k
    return first, coef


def _pass(x, n_out, rounding, shift):
    """x: (rows, n_in) int64 -> (rows, n_out): the taps along the last axis, out-of-plane taps reading the edge sample."""
    n_in = x.shape[1]
    first, coef = axis_tables(n_in, n_out)
    acc = np.zeros((x.shape[0], n_out), np.int64)
    for j in range(coef.shape[1]):
        acc += coef[:, j] * x[:, np.clip(first + j, 0, n_in - 1)]
    return (acc + rounding) >> shift


def scale_plane(plane, w_out, h_out):
    t = _pass(plane.astype(np.int64), w_out, 32, 6)
    assert t.min() >= -32768 and t.max() <= 32767
    out = _pass(np.ascontiguousarray(t.T), h_out, 1 << 17, 18).T
    return np.ascontiguousarray(np.clip(out, 0, 255).astype(np.uint8))


def scale_planes(planes, w_out, h_out):
    """(y, cb, cr) -> the picture of w_out x h_out."""
    y, cb, cr = planes
    return scale_plane(y, w_out, h_out), scale_plane(cb, w_out // 2, h_out // 2), scale_plane(cr, w_out // 2, h_out // 2)


def checker1(w, h):
    """0 / 255 at period 1 in every plane: the filter's overshoot clips at both ends."""
    yy, xx = np.mgrid[0:h, 0:w]
    y = (255 * ((xx + yy) & 1)).astype(np.uint8)
    c = np.ascontiguousarray(y[:h // 2, :w // 2])
    return y, c, (255 - c).astype(np.uint8)


PICTURES = ("textured", "checker1", "zeros", "ones", "noise")   # the contents the slot test walks through


def picture(name, w, h):
    """(y, cb, cr) of w x h."""
    if name in ("zeros", "ones"):
        v = 0 if name == "zeros" else 255
        return np.full((h, w), v, np.uint8), np.full((h // 2, w // 2), v, np.uint8), np.full((h // 2, w // 2), v, np.uint8)
    if name == "checker1":
        return checker1(w, h)
    return content({"textured": "cclm", "noise": "noise"}[name], w, h, 11)
