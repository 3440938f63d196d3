"""The CCLM building blocks of the search against the oracle's Predictor on a picture of 2 x 2 CTUs (64x64): the SAD list of
the three CCLM modes (sad_list_cclm) and the CCLM prediction of the pair (predict_blocks).  8x8, 16x16 and 32x32 blocks at
the four corners of the picture -- left neighbour and row above available or not -- and at one offset inside it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 64
LT, L, T = 81, 82, 83
KINDS = ("smooth", "noise", "extreme")


def _planes(kind):
    rng = np.random.default_rng(640 + KINDS.index(kind))
    shapes = ((H, W), (H // 2, W // 2), (H // 2, W // 2))
    if kind == "noise":
        return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    if kind == "extreme":   # 0 / 255 patches: the clips of the models
        return [(rng.integers(0, 2, (s[0] // 2, s[1] // 2)).repeat(2, 0).repeat(2, 1) * 255).astype(np.uint8) for s in shapes]
    yy, xx = np.indices((H, W))
    y = (128 + 60 * np.sin(xx / 7.0) + 50 * np.cos(yy / 5.0) + rng.normal(0, 6, (H, W))).clip(0, 255).astype(np.uint8)
    cb = (y[::2, ::2].astype(np.int32) // 2 + 40 + rng.integers(-4, 5, (H // 2, W // 2))).clip(0, 255).astype(np.uint8)
    cr = (200 - y[::2, ::2].astype(np.int32) // 3 + rng.integers(-4, 5, (H // 2, W // 2))).clip(0, 255).astype(np.uint8)
    return [y, cb, cr]


def _blocks(lg):
    n = 1 << lg
    corners = [(0, 0), (W - n, 0), (0, H - n), (W - n, H - n)]
    inside = {3: [(24, 40)], 4: [(16, 32)], 5: []}[lg]     # (a 32x32 block of a 64x64 picture is always a corner)
    return corners + inside


@functools.lru_cache(maxsize=None)
def _reference(kind, lg):
    """Per block: the oracle's predictions {mode: (2, n/2, n/2)} of the three CCLM modes and their SADs against the block's
    own chroma samples.  Computed once per (kind, lg) and shared by the tests; nothing of it comes from the device."""
    from oracle import pyoracle as po
    planes = _planes(kind)
    n = 1 << lg
    blocks = _blocks(lg)
    ora = [(x, y, lg, 0, pc, m) for (x, y) in blocks for m in (LT, T, L) for pc in (1, 2)]
    preds = po.predict_blocks(*planes, np.array(ora, np.int32))
    out = []
    for bi, (x, y) in enumerate(blocks):
        org = np.stack([planes[pc][y // 2:(y + n) // 2, x // 2:(x + n) // 2] for pc in (1, 2)]).astype(np.int64)
        pred, sad = {}, {}
        for mi, m in enumerate((LT, T, L)):
            at = (bi * 3 + mi) * 2
            pred[m] = np.stack(preds[at:at + 2])
            sad[m] = int(np.abs(org - pred[m].astype(np.int64)).sum())
        out.append((pred, sad))
    return planes, blocks, out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", [3, 4, 5])
def test_cclm_sad_list_and_prediction(built, kind, lg):
    """The three SADs of the list and the prediction of each mode's pair equal the oracle's at every block."""
    from wrenc_amd import gpu
    planes, blocks, ref = _reference(kind, lg)
    enc = gpu.Encoder(W, H, qp=32, max_split_depth=3)
    try:
        sads = enc.sad_lists(*planes, np.array([(x, y, lg, 4, 0, 0, 0) for (x, y) in blocks], np.int32))
        got = enc.predict_blocks(*planes, np.array([(x, y, lg, 1, m) for (x, y) in blocks for m in (LT, T, L)], np.int32))
    finally:
        enc.close()
    for bi, ((x, y), (pred, sad)) in enumerate(zip(blocks, ref)):
        for mi, m in enumerate((LT, T, L)):
            assert int(sads[bi][mi]) == sad[m], (kind, (x, y, lg), m, int(sads[bi][mi]), sad[m])
            assert np.array_equal(got[bi * 3 + mi], pred[m]), (kind, (x, y, lg), m)
        assert not sads[bi][3:].any()

