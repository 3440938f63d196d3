"""SAD lists (sad_list_angular) through each of its three loops, for each of the two instantiations of the component's
body (luma block, chroma pair) and for both in one call.  The list code chooses per list and component between SAMPLES
(entry by entry, one sample per lane), LINES (a row of four per lane) and BLOCKS (a 4x4 block per lane) by a cost count;
_loop() below restates that rule, and every case asserts on the CPU which loop it reaches, so that a later change of the
rule cannot quietly move a case to another loop.

Mode lists are arithmetic progressions (first mode, entries, stride) chosen so that within one iteration
  * lanes differ in filter_flag (8x8: 3 | 4, 32 | 33, 35 | 36, 64 | 65; 16x16: around 16..20 and 48..52),
  * some entries have PDPC and some do not (around 18 and 50),
  * one list per length has no PDPC entry at all (modes 19..49), which reaches the row code without PDPC,
  * modes 2, 34 and 66 appear (filtered references of luma blocks above 32 samples),
  * an entry lies past 66 (not evaluated: SAD 0).
Blocks at picture corners, on the top row, in the left column and inside a CTU, on the three kinds of plane of
tests/test_gpu_predict.py; each entry's SAD equals the one computed from the ORACLE's prediction of that mode."""
import functools

import numpy as np
import pytest

from test_gpu_predict import H, W, _planes
from test_gpu_sad_small_lists import _blocks

SAMPLES, LINES, BLOCKS = "samples", "lines", "blocks"


def _loop(lg_luma, comp, nmodes):
    """The loop sad_list_angular takes for component comp (0 luma, 1 the chroma pair) of a block of 1 << lg_luma luma
    samples a side and a list of nmodes entries: cost1_ / cost4_ / costL_ of wrenc_amd/csrc/dev_predict.h."""
    cs, nb = (1, 2) if comp else (0, 1)
    lg = lg_luma - cs
    nn = 1 << (2 * lg)
    lg_g4 = 2 * (lg - 2) + (1 if nb == 2 else 0)
    lg_gl = lg_g4 + 2
    cost1 = nmodes * ((nb * nn + 63) >> 6)
    cost4 = 9 * ((nmodes + (64 >> lg_g4) - 1) >> (6 - lg_g4)) if nb * nn > 32 else 1 << 20
    cost_l = 3 * ((nmodes + (64 >> lg_gl) - 1) >> (6 - lg_gl)) if lg_gl <= 6 else 1 << 20
    if cost4 < cost1 and cost4 < cost_l:
        return BLOCKS
    if cost_l <= cost1:
        return LINES
    return SAMPLES


# (log2 luma size, comps) -> {entries: (luma's loop, the chroma pair's loop)}; None: the component is not in the call.
# One entry over the chroma pair of a 32x32 costs 8 sample iterations against 9 for one block iteration, so it goes
# entry by entry; two entries are the shortest list of that pair that goes by blocks.
CASES = {
    (2, 1): {1: (SAMPLES, None), 3: (LINES, None), 16: (LINES, None)},
    (3, 1): {2: (SAMPLES, None), 6: (LINES, None), 13: (BLOCKS, None)},
    (4, 1): {1: (LINES, None), 2: (LINES, None), 13: (BLOCKS, None)},
    (5, 1): {1: (BLOCKS, None), 13: (BLOCKS, None)},
    (3, 2): {2: (None, SAMPLES), 13: (None, LINES)},
    (4, 2): {2: (None, LINES), 13: (None, BLOCKS)},
    (5, 2): {1: (None, SAMPLES), 2: (None, BLOCKS), 13: (None, BLOCKS)},
    (3, 3): {2: (SAMPLES, SAMPLES), 6: (LINES, LINES), 13: (BLOCKS, LINES)},
    (4, 3): {2: (LINES, LINES), 6: (LINES, LINES), 13: (BLOCKS, BLOCKS)},
    (5, 3): {2: (BLOCKS, BLOCKS), 6: (BLOCKS, BLOCKS), 13: (BLOCKS, BLOCKS)},
}

# entries -> [(first mode, stride)]
LISTS = {
    1: [(m, 1) for m in (2, 10, 18, 25, 34, 50, 58, 66)],
    2: [(2, 32), (34, 32), (66, 1),                            # 2 | 34, 34 | 66, 66 | past 66
        (17, 1), (18, 1), (49, 1), (50, 1),                    # PDPC kinds meet: 17 | 18, 18 | 19, 49 | 50, 50 | 51
        (3, 1), (32, 1), (35, 1), (64, 1),                     # 8x8: filter_flag differs
        (15, 1), (20, 1), (47, 1), (52, 1),                    # 16x16: filter_flag differs
        (25, 3)],                                              # no PDPC entry
    3: [(2, 32), (17, 1), (49, 1), (65, 1), (20, 5)],
    6: [(2, 16),                                               # 2, 18, 34, 50, 66, past 66
        (2, 1), (30, 1), (33, 1), (61, 1), (63, 1),            # 3 | 4, 32 | 33, 35 | 36, 64 | 65, past 66
        (15, 1), (47, 1),                                      # 15..20, 47..52
        (19, 5)],                                              # 19..44: no PDPC entry
    13: [(2, 8),                                               # 2, 10, 18, .. 66, four entries past 66
         (2, 1), (12, 1), (44, 1), (56, 1), (2, 5),
         (26, 1), (20, 2)],                                    # 26..38 and 20..44: no PDPC entry
    16: [(3, 1), (35, 1), (2, 4), (55, 1),
         (19, 2)],                                             # 19..49: no PDPC entry
}


def test_every_list_length_has_a_list_without_pdpc_and_the_lists_cover_the_special_modes():
    seen = set()
    for nm, lists in LISTS.items():
        modes = [[m0 + j * st for j in range(nm)] for (m0, st) in lists]
        assert any(all(19 <= m <= 49 for m in ms) for ms in modes), nm
        seen.update(m for ms in modes for m in ms)
    assert {2, 18, 34, 50, 66} <= seen and max(seen) > 66


@pytest.mark.parametrize("lg,comps", sorted(CASES))
def test_cases_reach_the_loops_they_name(lg, comps):
    for nm, (luma, pair) in CASES[(lg, comps)].items():
        assert (luma is not None) == bool(comps & 1) and (pair is not None) == bool(comps & 2)
        if comps & 1:
            assert _loop(lg, 0, nm) == luma, (lg, comps, nm)
        if comps & 2:
            assert _loop(lg, 1, nm) == pair, (lg, comps, nm)
    # each instantiation goes through each of its loops somewhere (a 4x4 luma block never goes by blocks)
    for comp in (0, 1):
        reached = {loops[comp] for (_, c), per in CASES.items() if c == 1 + comp for loops in per.values()}
        assert reached == {SAMPLES, LINES, BLOCKS}, (comp, reached)


def _aligned_blocks(n):
    return [(x, y) for (x, y) in _blocks(n) if x % n == 0 and y % n == 0]


@functools.lru_cache(maxsize=None)
def _oracle_sads(kind, lg):
    """(planes, {(x, y, mode): (luma SAD, chroma pair SAD)}) of every aligned block position and mode 2..66, once per
    kind of plane and block size; read-only for the tests that share it."""
    from oracle import pyoracle as po
    planes = _planes(kind, 1900 + lg)
    n = 1 << lg
    blocks = _aligned_blocks(n)
    with_pair = lg >= 3
    ora = []
    for (x, y) in blocks:
        for m in range(2, 67):
            ora.append((x, y, lg, 1 if lg == 2 else 0, 0, m))
            if with_pair:
                ora.append((x, y, lg, 0, 1, m))
                ora.append((x, y, lg, 0, 2, m))
    preds = po.predict_blocks(*planes, np.array(ora, np.int32))
    per = 3 if with_pair else 1
    sad = {}
    for bi, (x, y) in enumerate(blocks):
        oy = planes[0][y:y + n, x:x + n].astype(np.int64)
        ocb = planes[1][y // 2:(y + n) // 2, x // 2:(x + n) // 2].astype(np.int64)
        ocr = planes[2][y // 2:(y + n) // 2, x // 2:(x + n) // 2].astype(np.int64)
        for mi, m in enumerate(range(2, 67)):
            at = (bi * 65 + mi) * per
            luma = int(np.abs(oy - preds[at].astype(np.int64)).sum())
            pair = 0
            if with_pair:
                pair = int(np.abs(ocb - preds[at + 1].astype(np.int64)).sum()) + int(np.abs(ocr - preds[at + 2].astype(np.int64)).sum())
            sad[(x, y, m)] = (luma, pair)
    return planes, sad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["smooth", "noise", "extreme"])
@pytest.mark.parametrize("lg,comps", sorted(CASES))
def test_sad_lists_through_every_loop_against_the_oracles_predictions(built, kind, lg, comps):
    from wrenc_amd import gpu
    planes, sad = _oracle_sads(kind, lg)
    blocks = _aligned_blocks(1 << lg)
    items = [(x, y, lg, comps, m0, nm, st) for (x, y) in blocks for nm in CASES[(lg, comps)] for (m0, st) in LISTS[nm]]
    enc = gpu.Encoder(W, H, qp=32, max_split_depth=3)
    got = enc.sad_lists(*planes, np.array(items, np.int32))
    enc.close()
    for item, row in zip(items, got):
        x, y, _, _, m0, nm, st = item
        for j in range(16):
            m = m0 + j * st
            want = 0
            if j < nm and m <= 66:
                luma, pair = sad[(x, y, m)]
                want = (luma if comps & 1 else 0) + (pair if comps & 2 else 0)
            assert int(row[j]) == want, (kind, item, j, m, int(row[j]), want)
