"""Shared by test_source_geometry.py and test_gpu_source_geometry.py: the picture sizes that take the three source kernels
(wrenc_amd/csrc/dev_format.h, dev_rgb.h, dev_scale.h) past their first workgroup in x and past one scaler tile, and a plain
Python restatement of the launch geometry those sizes are chosen against -- the grids of wrenc_gpu_io.hip and its
build_scale_axis.  The kernels' constants are read out of the headers: a changed constant changes what the restatement says
of a case, and test_source_geometry.py then fails on the properties the case is named for."""
import functools
import os
import re

import numpy as np

import scale_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wrenc_amd", "csrc")
WAVE = 64                                        # lanes along a row per workgroup of the two converters


def _constants():
    """The constants of the three headers, by name."""
    want = {"dev_format.h": ("kFormatGroup", "kFormatRows"), "dev_rgb.h": ("kRgbRows",),
            "dev_scale.h": ("kScaleTileW", "kScaleTileH", "kScaleSpanX", "kScaleSpanY", "kScaleCoefs")}
    out = {}
    for header, names in want.items():
        src = open(os.path.join(CSRC, header)).read()
        for name in names:
            m = re.search(r"constexpr int [^;]*\b%s = (\d+)\s*[,;]" % name, src)
            assert m, (header, name)
            out[name] = int(m.group(1))
    # the RGB converter's lane makes as many luma samples as the format converter's
    assert re.search(r"constexpr int kRgbGroup = kFormatGroup;", open(os.path.join(CSRC, "dev_rgb.h")).read())
    return out


K = _constants()
GROUP, FORMAT_ROWS, RGB_ROWS = K["kFormatGroup"], K["kFormatRows"], K["kRgbRows"]
TILE_W, TILE_H, SPAN_X, SPAN_Y, COEFS = K["kScaleTileW"], K["kScaleTileH"], K["kScaleSpanX"], K["kScaleSpanY"], K["kScaleCoefs"]

# name -> (source, visible, coded); test_source_geometry.py asserts what each is here for
CASES = {
    "wide": ((1030, 18), (1030, 18), (1056, 32)),        # no scaling: three workgroups along a luma row, a row tail in the last
    "wide_last": ((1022, 18), (1022, 18), (1024, 32)),   # the last lane of the last workgroup in x is live, and a row tail
    "s4to1": ((1040, 272), (260, 68), (288, 96)),        # 16 taps on both axes, full 64 x 16 tiles, the largest row span
    "s_span": ((1156, 72), (290, 18), (320, 32)),        # the largest column span; chroma 145 wide: one byte in the last dword
    "s1to4": ((66, 18), (264, 72), (288, 96)),           # 4 taps; chroma source 33 wide: dwords over the right edge
    "s_mixed": ((1030, 50), (274, 170), (288, 192)),     # 3.76 : 1 down in x, 3.4 x up in y
}
UNSCALED = ("wide", "wide_last")
SCALED = ("s4to1", "s_span", "s1to4", "s_mixed")


def ceil_div(a, b):
    return -(-a // b)


# ---- the converters' grids (wrenc_gpu_io.hip: upload_planes_from, launch_rgb) ----

def row_lanes(width):
    """One row of `width` output samples: (live lanes, workgroups in x that hold a live lane, `left` of the last live lane)."""
    lanes = ceil_div(width, GROUP)
    return lanes, ceil_div(lanes, WAVE), width - GROUP * (lanes - 1)


def row_groups(rows, per_group):
    """Rows (or row pairs) in workgroups of per_group: (workgroups, rows in the last)."""
    groups = ceil_div(rows, per_group)
    return groups, rows - per_group * (groups - 1)


def format_grid(w, h, interleaved):
    """convert_format_kernel's grid (x, y) over a w x h picture; interleaved: nv12 / p010le, whose CbCr plane is walked once."""
    row_blocks = (ceil_div(h, FORMAT_ROWS), ceil_div(h // 2, FORMAT_ROWS))
    return ceil_div(w, WAVE * GROUP), row_blocks[0] + (1 if interleaved else 2) * row_blocks[1]


def rgb_grid(w, h):
    """convert_rgb_kernel's grid (x, y)."""
    return ceil_div(w, WAVE * GROUP), ceil_div(h // 2, RGB_ROWS)


# ---- the scaler's tables (wrenc_gpu_io.hip: build_scale_axis) ----

@functools.lru_cache(maxsize=None)
def _rows(n_in, n_out):
    return [scale_ref.taps(n_in, n_out, o) for o in range(n_out)]


class Axis:
    """One axis of one plane size as build_scale_axis makes it: first[n_out], coef[n_out, kScaleCoefs] (zero behind a
    sample's own taps), lengths[n_out] (a sample's own taps), taps (the longest list, rounded up to even), tile_base[tiles],
    spans[tiles] (hi + taps - lo of each tile) and span, their maximum."""

    def __init__(self, n_in, n_out, tile, align4):
        rows = _rows(n_in, n_out)
        self.n_in, self.n_out, self.tile = n_in, n_out, tile
        self.first = np.array([f for f, _ in rows], np.int64)
        self.lengths = np.array([len(k) for _, k in rows], np.int64)
        assert int(self.lengths.max()) <= COEFS
        self.coef = np.zeros((n_out, COEFS), np.int64)
        for o, (_, k) in enumerate(rows):
            self.coef[o, :len(k)] = k
        self.taps = (int(self.lengths.max()) + 1) & ~1
        self.tiles = ceil_div(n_out, tile)
        self.tile_base, self.spans = [], []
        for t in range(self.tiles):
            f = self.first[t * tile:(t + 1) * tile]
            lo, hi = int(f.min()), int(f.max())
            if align4:
                lo &= ~3                         # rounds down for a negative lo too, as in C
            self.tile_base.append(lo)
            self.spans.append(hi + self.taps - lo)
        self.span = max(self.spans)

    def full_tiles(self):
        return self.n_out // self.tile

    def clamps_right(self, t):
        """Tile t reads past the last input sample: the edge rule applies on its right."""
        return self.tile_base[t] + self.spans[t] > self.n_in

    def clamps_left(self, t):
        return self.tile_base[t] < 0


@functools.lru_cache(maxsize=None)
def axis(n_in, n_out, tile, align4):
    return Axis(n_in, n_out, tile, align4)


def plane_axes(source, visible, chroma):
    """(x, y) axes of the luma or the chroma planes of one case."""
    s = 1 if chroma else 0
    return (axis(source[0] >> s, visible[0] >> s, TILE_W, True), axis(source[1] >> s, visible[1] >> s, TILE_H, False))


def scale_grid(source, visible):
    """scale_kernel's grid: the tiles of the luma plane and twice those of a chroma plane."""
    (lx, ly), (cx, cy) = plane_axes(source, visible, False), plane_axes(source, visible, True)
    return lx.tiles * ly.tiles + 2 * cx.tiles * cy.tiles


def span_bound(n_in, n_out, tile, align4):
    """An upper bound on build_scale_axis's span less one, in closed form, for one n_out and an ARRAY of n_in: every sample
    taken to have the untrimmed list of include/wrenc_scale.h, from lo(o) = floor((C - 2 M) / D) + 1 on, run over
    kScaleCoefs taps.  lo grows with o, so a tile's smallest lo is that of its first sample and its largest that of its
    last.  Returns (bound[len(n_in)], tile of the maximum[len(n_in)]).

    Why `less one`: the real first(o) is lo(o) or, where the leading coefficient came out as 0 and is not listed, lo(o) + 1
    (within the 16-tap ratios, above 3.5 : 1, the second tap lies at least 1/4 of the kernel's unit inside the support, where
    its weight is far from rounding to 0), while the passes still run over the axis' whole tap count; the tile base only
    moves up with first.  So span <= bound + 1, and the tests ask bound + 1 <= kScaleSpanX / kScaleSpanY."""
    n_in = np.asarray(n_in, np.int64)[:, None]
    D, M = 2 * n_out, 2 * np.maximum(n_in, n_out)
    t = np.arange(ceil_div(n_out, tile), dtype=np.int64)[None, :]
    o0, o1 = t * tile, np.minimum(n_out, (t + 1) * tile) - 1

    def lo(o):
        return ((2 * o + 1) * n_in - n_out - 2 * M) // D + 1

    base = lo(o0)
    if align4:
        base = base & ~3
    spans = lo(o1) + COEFS - base
    return spans.max(axis=1), spans.argmax(axis=1)


def coefficient_sums(n_in, n_out, outputs):
    """(sum of the positive coefficients, sum of the negative ones) of include/wrenc_scale.h's lists, exact, for one n_out,
    an ARRAY of n_in and an array of output indices: two int64 arrays of len(n_in) x len(outputs).  Coefficients that are
    not listed are zeros and add nothing to either."""
    n_in = np.asarray(n_in, np.int64)[:, None, None]
    o = np.asarray(outputs, np.int64)[None, :, None]
    D, M = 2 * n_out, 2 * np.maximum(n_in, n_out)
    C = (2 * o + 1) * n_in - n_out
    slots = int(4 * max(int(n_in.max()), n_out) // n_out) + 1          # the open interval is 4 M / D samples long
    i = (C - 2 * M) // D + 1 + np.arange(slots, dtype=np.int64)[None, None, :]
    N = np.abs(i * D - C)
    W = np.where(N < M, (3 * N - 5 * M) * N * N + 2 * M ** 3, ((5 * M - N) * N - 8 * M * M) * N + 4 * M ** 3)
    W = np.where(N < 2 * M, W, 0)
    T = W.sum(axis=2, keepdims=True)
    assert T.min() > 0
    k = (8192 * W + T) // (2 * T)
    k = np.where(N < 2 * M, k, 0)
    fix = scale_ref.UNITY - k.sum(axis=2)        # goes to the tap of the largest weight, which is positive
    assert np.all(np.take_along_axis(k, W.argmax(axis=2)[:, :, None], axis=2)[:, :, 0] + fix > 0)
    return np.maximum(k, 0).sum(axis=2) + fix, np.minimum(k, 0).sum(axis=2)


def edge_tile_outputs(n_out):
    """The output indices of the first and the last tile of an axis of n_out samples, x tiles: the y tiles' lie inside."""
    last = (ceil_div(n_out, TILE_W) - 1) * TILE_W
    return np.unique(np.concatenate([np.arange(min(TILE_W, n_out)), np.arange(last, n_out)]))
