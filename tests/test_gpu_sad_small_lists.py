"""SAD lists of small blocks through the row-of-four-per-lane code of sad_list_angular (a lane predicts the four samples
that lie next to each other across the prediction direction; 4x4 luma: sixteen entries share an iteration, the 4x4
chroma pair of an 8x8 block: eight): what the lists of tests/test_gpu_predict.py do not reach.  Lists of sixteen
consecutive modes started so that the changes of kind around modes 18 and 50 (angle >= 0 with PDPC | mode 18 / 50 |
negative angle, its own projected table) fall on every position of an iteration; lists whose length does not fill an
iteration (1, 3, 5, 13) and one that does (16); lists that run past mode 66 (entries that are not evaluated: SAD 0).  At
picture corners, on the top row, in the left column and inside, on the three kinds of plane of test_gpu_predict.py;
each entry's SAD equals the one computed from the ORACLE's prediction of that mode."""
import numpy as np
import pytest

from test_gpu_predict import H, W, _planes

pytestmark = pytest.mark.gpu

# (first mode, entries, stride)
LISTS = ([(m0, 16, 1) for m0 in range(3, 19)]            # 17 | 18 | 19 at every position of sixteen
         + [(m0, 16, 1) for m0 in range(35, 51)]         # 49 | 50 | 51 likewise
         + [(m0, nm, 1) for nm in (1, 3, 5, 13) for m0 in (2, 17, 18, 33, 34, 48, 50)]
         + [(2, 16, 4), (6, 16, 4), (2, 13, 5), (17, 5, 8), (18, 3, 16), (66, 1, 1)]
         + [(60, 16, 1), (64, 5, 1), (66, 3, 1), (55, 13, 1), (50, 16, 2)])     # past mode 66


def _blocks(n):
    """Corners, top row, left column, right column, bottom row and inside; CTU corners and positions inside a CTU."""
    fixed = [(0, 0), (W - n, 0), (0, H - n), (W - n, H - n),                    # picture corners
             (n, 0), (32, 0), (32 + n, 0), (64 - n, 0),                         # top row
             (0, n), (0, 32), (0, 32 + n), (0, 64 - n),                         # left column
             (W - n, 32), (32, H - n),                                          # right column, bottom row
             (32, 32), (32 + n, 32), (32, 32 + n), (32 + n, 32 + n), (64 - n, 64 - n), (40, 48), (64, 32 + n)]
    seen, out = set(), []
    for b in fixed:
        if b not in seen:
            seen.add(b)
            out.append(b)
    return out


@pytest.mark.parametrize("kind", ["smooth", "noise", "extreme"])
@pytest.mark.parametrize("lg,comps", [(2, 1), (3, 2), (3, 3)])
def test_small_sad_lists_against_the_oracles_predictions(built, kind, lg, comps):
    """lg 2, comps 1: a 4x4 luma block; lg 3, comps 2: the 4x4 chroma pair of an 8x8 block alone; comps 3: the 8x8 luma
    block and its chroma pair summed, as the single-tree 8x8 leaf search asks."""
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    planes = _planes(kind, 500 + 10 * lg + comps)
    n = 1 << lg
    blocks = _blocks(n)
    items = [(x, y, lg, comps, m0, nm, st) for (x, y) in blocks for (m0, nm, st) in LISTS]
    enc = gpu.Encoder(W, H, qp=32, max_split_depth=3)
    got = enc.sad_lists(*planes, np.array(items, np.int32))
    enc.close()
    # the oracle's predictions of every mode of every block, as tests/test_gpu_predict.py asks for them
    ora = []
    for (x, y) in blocks:
        for m in range(2, 67):
            ora.append((x, y, lg, 1 if lg == 2 else 0, 0, m))
            if comps & 2:
                ora.append((x, y, lg, 0, 1, m))
                ora.append((x, y, lg, 0, 2, m))
    preds = po.predict_blocks(*planes, np.array(ora, np.int32))
    per = 3 if comps & 2 else 1
    sad = {}
    for bi, (x, y) in enumerate(blocks):
        oy = planes[0][y:y + n, x:x + n].astype(np.int64)
        ocb = planes[1][y // 2:(y + n) // 2, x // 2:(x + n) // 2].astype(np.int64)
        ocr = planes[2][y // 2:(y + n) // 2, x // 2:(x + n) // 2].astype(np.int64)
        for mi, m in enumerate(range(2, 67)):
            at = (bi * 65 + mi) * per
            v = int(np.abs(oy - preds[at].astype(np.int64)).sum()) if comps & 1 else 0
            if comps & 2:
                v += int(np.abs(ocb - preds[at + 1].astype(np.int64)).sum()) + int(np.abs(ocr - preds[at + 2].astype(np.int64)).sum())
            sad[(x, y, m)] = v
    for item, row in zip(items, got):
        x, y, _, _, m0, nm, st = item
        for j in range(16):
            m = m0 + j * st
            want = sad[(x, y, m)] if j < nm and m <= 66 else 0
            assert int(row[j]) == want, (kind, item, j, m, int(row[j]), want)
