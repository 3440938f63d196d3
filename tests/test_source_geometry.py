"""The launch geometry of the source kernels, without a device (tests/source_geometry.py restates it): the cases of
test_gpu_source_geometry.py reach the workgroups, tiles and tails they are named for; the restated scaler tables are the
library's; every size pair the ABI accepts (wrenc_gpu_set_source_size: even, at least 16, within a factor of 4 per axis --
planes of 8 samples on for chroma) gets tables that fit the scaler's tile; and the filter's sums stay inside the 16- and
32-bit intermediates of dev_scale.h for every such pair."""
import numpy as np
import pytest

import scale_ref
import source_geometry as sg

# n_in -> n_out of one axis, near each limit: 4 : 1 and 1 : 4 at the largest size, ratios just under 4, and the pair of the
# largest bound of the sweep scaled up
LARGE_PAIRS = [(16384, 4096), (16382, 4096), (4096, 16384), (4098, 16384), (16380, 4096), (16383, 4096), (8191, 2048), (15999, 4000),
               (16184, 4060), (2047, 8186), (9248, 2320), (16384, 8192)]
SWEEP = range(8, 701)                            # n_out; n_in: ceil(n_out / 4) .. 4 n_out


def _sweep_inputs(n_out):
    return np.arange(sg.ceil_div(n_out, 4), 4 * n_out + 1, dtype=np.int64)


def test_wide_reaches_the_workgroups_and_tails_it_names():
    source, visible, coded = sg.CASES["wide"]
    assert source == visible                     # no scaling
    w, h = source
    assert sg.row_lanes(w) == (129, 3, 6)        # luma: 129 lanes in 3 workgroups, 6 samples in the last lane's eight
    assert sg.row_lanes(w // 2) == (65, 2, 3)    # chroma 515 wide: a second workgroup for one lane, and that lane a tail
    assert sg.row_groups(h, sg.FORMAT_ROWS) == (5, 2)         # 18 luma rows: a partial last workgroup
    assert sg.row_groups(h // 2, sg.FORMAT_ROWS) == (3, 1)    # 9 chroma rows
    assert sg.row_groups(h // 2, sg.RGB_ROWS) == (3, 1)       # 9 row pairs
    assert sg.format_grid(w, h, False) == (3, 5 + 2 * 3) and sg.format_grid(w, h, True) == (3, 5 + 3)
    assert sg.rgb_grid(w, h) == (3, 3)
    # what the old sizes reach: the first workgroup alone, at most 9 lanes
    for ow, oh in ((32, 32), (34, 30), (70, 50), (64, 64)):
        assert sg.row_lanes(ow)[:2] <= (9, 1) and sg.format_grid(ow, oh, False)[0] == 1 and sg.rgb_grid(ow, oh)[0] == 1
    assert coded == ((w + 31) // 32 * 32, (h + 31) // 32 * 32) and coded[0] // 32 == 33 and coded[1] // 32 == 1   # 33 x 1 CTUs


def test_wide_last_fills_the_last_workgroup():
    """At `wide` the third workgroup holds one live lane: a lane index made of blockIdx.x * 63 would still reach every
    lane, twice some, and nothing would show.  Here the last lane of the last workgroup is live, and a tail: every lane of
    the grid has bytes of its own."""
    source, visible, coded = sg.CASES["wide_last"]
    assert source == visible and coded == (1024, 32)
    w, h = source
    lanes, groups, left = sg.row_lanes(w)
    assert (lanes, groups, left) == (128, 2, 6) and lanes == groups * sg.WAVE
    assert sg.format_grid(w, h, False)[0] == sg.rgb_grid(w, h)[0] == groups
    assert (groups - 1) * (sg.WAVE - 1) + sg.WAVE - 1 < lanes - 1      # 63 lanes a workgroup fall short of the last lane
    assert sg.row_lanes(w // 2) == (64, 1, 7)    # chroma 511 wide: the whole first workgroup, a tail of seven
    lanes, groups, _ = sg.row_lanes(sg.CASES["wide"][0][0])
    assert (groups - 1) * (sg.WAVE - 1) + sg.WAVE - 1 >= lanes - 1     # ... and do not at `wide`


@pytest.mark.parametrize("name", sg.SCALED)
def test_scaled_cases_reach_the_tiles_they_name(name):
    source, visible, coded = sg.CASES[name]
    assert coded == ((visible[0] + 31) // 32 * 32, (visible[1] + 31) // 32 * 32)
    (lx, ly), (cx, cy) = sg.plane_axes(source, visible, False), sg.plane_axes(source, visible, True)
    for a in (lx, cx):
        assert a.span <= sg.SPAN_X and all(b % 4 == 0 for b in a.tile_base)
    for a in (ly, cy):
        assert a.span <= sg.SPAN_Y
    # every case: more than one tile in x (tile_base[tx] for tx > 0), and a last tile that is not the first and clamps on
    # its right
    for a in (lx, cx):
        assert a.tiles > 1 and a.clamps_right(a.tiles - 1) and not a.clamps_left(a.tiles - 1), name
        assert len(set(a.tile_base)) == a.tiles
    if name == "s4to1":
        assert (lx.taps, ly.taps, cx.taps, cy.taps) == (16, 16, 16, 16)
        assert (lx.tiles, ly.tiles, lx.full_tiles(), ly.full_tiles()) == (5, 5, 4, 4)
        assert (cx.tiles, cy.tiles) == (3, 3)
        assert (lx.span, ly.span) == (270, 76) and (sg.SPAN_X, sg.SPAN_Y) == (288, 96)
        assert lx.tile_base[0] < 0 and ly.tile_base[0] < 0
        assert cx.n_out % 4 == 2 and cx.tiles - 1 == 2          # the byte-wise tail store: two bytes, in tile 2
    elif name == "s_span":
        assert lx.taps == 16 and lx.span == 271 and lx.spans.index(271) == 3 and lx.tiles == 5
        assert (cx.n_in, cx.n_out) == (578, 145) and cx.n_out % 4 == 1 and cx.tiles - 1 == 2   # one visible byte, in tile 2
        assert lx.n_out % 4 == 2 and lx.tiles - 1 == 4          # luma 290: two bytes, in tile 4
    elif name == "s1to4":
        assert (lx.taps, ly.taps, cx.taps, cy.taps) == (4, 4, 4, 4)
        assert (lx.tiles, ly.tiles, cx.tiles, cy.tiles) == (5, 5, 3, 3)
        assert (cx.n_in, cy.n_in) == (33, 9)
        # the last chroma tile loads the dword at column 32 of 33: three of its bytes lie over the right edge
        t = cx.tiles - 1
        assert cx.n_in % 4 == 1 and cx.tile_base[t] <= cx.n_in - 1 < cx.tile_base[t] + cx.spans[t] - 1
        assert lx.n_in % 4 == 2 and lx.clamps_right(lx.tiles - 1)
    else:
        assert name == "s_mixed"
        assert lx.taps == 16 and lx.span == 256 and 3.75 < lx.n_in / lx.n_out < 3.77
        assert ly.taps == 4 and ly.tiles == 11 and 3.39 < ly.n_out / ly.n_in < 3.41
        assert (cx.n_in, cx.n_out) == (515, 137) and cx.n_out % 4 == 1 and cx.tiles == 3
    # what scale_ref.SIZES reach: one tile in x, always
    for s, v, _ in scale_ref.SIZES:
        assert all(a.tiles == 1 for a in (sg.plane_axes(s, v, False)[0], sg.plane_axes(s, v, True)[0]))


@pytest.mark.parametrize("name", sg.SCALED)
def test_restated_tables_are_the_librarys(built, name):
    """first, tap count and coefficients of every output sample of the four axes of a case."""
    from wrenc_amd import gpu
    source, visible, _ = sg.CASES[name]
    for chroma in (False, True):
        for a in sg.plane_axes(source, visible, chroma):
            longest = 0
            for o in range(a.n_out):
                first, coef = gpu.scale_taps(a.n_in, a.n_out, o)
                assert first == a.first[o] and len(coef) == a.lengths[o], (a.n_in, a.n_out, o)
                assert coef == a.coef[o, :len(coef)].tolist() and not a.coef[o, len(coef):].any(), (a.n_in, a.n_out, o)
                longest = max(longest, len(coef))
            assert a.taps == (longest + 1) & ~1


def _exact_pairs():
    pairs = set(LARGE_PAIRS)
    for name in sg.SCALED:
        source, visible, _ = sg.CASES[name]
        pairs.update((source[d] >> s, visible[d] >> s) for d in (0, 1) for s in (0, 1))
    return sorted(pairs)


@pytest.mark.parametrize("n_in,n_out", _exact_pairs(), ids=["%d-%d" % p for p in _exact_pairs()])
def test_the_closed_form_bounds_the_exact_span(n_in, n_out):
    """The named cases' axes and the large pairs, as x and as y: the tables build_scale_axis would make fit the tile, and
    their span is at most the closed form's bound plus one (source_geometry.span_bound tells why plus one)."""
    for tile, align4, room in ((sg.TILE_W, True, sg.SPAN_X), (sg.TILE_H, False, sg.SPAN_Y)):
        a = sg.axis(n_in, n_out, tile, align4)
        bound = int(sg.span_bound([n_in], n_out, tile, align4)[0][0])
        assert a.span <= bound + 1 <= room, (tile, a.span, bound)
        # the bound's premises: first is lo or lo + 1 where 16 taps run, and never below lo
        lo = ((2 * np.arange(n_out, dtype=np.int64) + 1) * n_in - n_out - 4 * max(n_in, n_out)) // (2 * n_out) + 1
        trimmed = a.first - lo
        assert trimmed.min() >= 0 and (a.taps < 16 or trimmed.max() <= 1), (tile, int(trimmed.max()))
        assert int((a.first + a.taps - lo).max()) <= sg.COEFS + 1


def test_every_legal_pair_fits_the_tile():
    """Every n_out of 8 .. 700 with every n_in within a factor of 4: the bound on the span, plus one, is within kScaleSpanX
    for tiles of kScaleTileW columns and within kScaleSpanY for tiles of kScaleTileH rows.  The largest bounds: 271 columns
    at 1156 -> 290 in tile 3, and 76 rows, first at 64 -> 16."""
    worst = {}
    for tile, align4, room in ((sg.TILE_W, True, sg.SPAN_X), (sg.TILE_H, False, sg.SPAN_Y)):
        best = (0, None)
        for n_out in SWEEP:
            n_in = _sweep_inputs(n_out)
            bound, where = sg.span_bound(n_in, n_out, tile, align4)
            at = int(bound.argmax())
            assert int(bound[at]) + 1 <= room, (tile, int(n_in[at]), n_out, int(bound[at]))
            if int(bound[at]) > best[0]:
                best = (int(bound[at]), (int(n_in[at]), n_out, int(where[at])))
        worst[tile] = best
    print("largest span bounds:", worst)
    assert worst[sg.TILE_W] == (271, (1156, 290, 3))
    assert worst[sg.TILE_H][0] == 76 and worst[sg.TILE_H][1][:2] == (64, 16)
    for n_in, n_out in LARGE_PAIRS:
        assert n_in <= 4 * n_out and n_out <= 4 * n_in
        assert int(sg.span_bound([n_in], n_out, sg.TILE_W, True)[0][0]) + 1 <= sg.SPAN_X, (n_in, n_out)
        assert int(sg.span_bound([n_in], n_out, sg.TILE_H, False)[0][0]) + 1 <= sg.SPAN_Y, (n_in, n_out)


def _check_sums(pos, neg, what):
    """The horizontal pass of an all-255 (or 0 / 255) row stays inside int16 at both ends, and the vertical pass of
    int16 extremes inside int32."""
    assert np.all(pos + neg == scale_ref.UNITY), what
    assert int(((pos * 255 + 32) >> 6).max()) <= 32767, (what, int(pos.max()))
    assert int(((neg * 255 + 32) >> 6).min()) >= -32768, (what, int(neg.min()))
    assert int(((pos - neg) * 32767 + (1 << 17)).max()) < 1 << 31, (what, int((pos - neg).max()))


@pytest.mark.parametrize("part", range(7))
def test_intermediates_stay_in_range(part):
    """Every pair of the sweep (n_out of 100 per part), every output sample of the first and the last tile: exact
    coefficients, their positive and negative sums."""
    for n_out in SWEEP[part * 100:(part + 1) * 100]:
        n_in = _sweep_inputs(n_out)
        outputs = sg.edge_tile_outputs(n_out)
        # by tap count: the lists of n_in <= n_out hold 4 slots, those of 4 n_out 16
        for chunk in np.array_split(n_in, 8):
            pos, neg = sg.coefficient_sums(chunk, n_out, outputs)
            _check_sums(pos, neg, (n_out, int(chunk[0]), int(chunk[-1])))


@pytest.mark.parametrize("n_in,n_out", _exact_pairs(), ids=["%d-%d" % p for p in _exact_pairs()])
def test_intermediates_stay_in_range_at_size(n_in, n_out):
    """... and the named cases' axes and the large pairs; the vectorised sums are those of scale_ref.taps."""
    outputs = sg.edge_tile_outputs(n_out)
    pos, neg = sg.coefficient_sums([n_in], n_out, outputs)
    _check_sums(pos, neg, (n_in, n_out))
    for j in (0, len(outputs) // 2, len(outputs) - 1):
        k = scale_ref.taps(n_in, n_out, int(outputs[j]))[1]
        assert (sum(c for c in k if c > 0), sum(c for c in k if c < 0)) == (int(pos[0, j]), int(neg[0, j]))
