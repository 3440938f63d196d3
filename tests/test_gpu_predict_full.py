"""Kernel-level parity of the FULL candidates' predictor (dev_predict.h, predict_full: four samples per lane, the
horizontal modes transposed inside a quad) in every destination the search gives it -- the recon tile, the LDS park of an
8x8 pack, the three-piece park of a 16x16 pack -- against the oracle's Predictor: every mode at every block position of a
3x3-CTU picture (every availability pattern), prediction bytes as read back from the destination and the i16 residuals
against the block's own samples.  (The fourth destination, the test entry's scratch, is what tests/test_gpu_predict.py
reads.)"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 96
KINDS = ["smooth", "noise", "extreme"]
CCLM = [81, 82, 83]
NO = 255   # gpu.Encoder.NO_MODE


@functools.lru_cache(maxsize=None)
def _planes(kind):
    rng = np.random.default_rng({"smooth": 11, "noise": 12, "extreme": 13}[kind])
    shapes = ((H, W), (H // 2, W // 2), (H // 2, W // 2))
    if kind == "noise":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in shapes)
    if kind == "extreme":   # 0 / 255 patches: PDPC and CCLM clips, planar i16 range, residuals of +-255
        return tuple((rng.integers(0, 2, (s[0] // 2, s[1] // 2)).repeat(2, 0).repeat(2, 1) * 255).astype(np.uint8) for s in shapes)
    yy, xx = np.indices((H, W))
    y = (128 + 60 * np.sin(xx / 7.0) + 50 * np.cos(yy / 5.0) + rng.normal(0, 6, (H, W))).clip(0, 255).astype(np.uint8)
    cb = (y[::2, ::2].astype(np.int32) // 2 + 40 + rng.integers(-4, 5, (H // 2, W // 2))).clip(0, 255).astype(np.uint8)
    cr = (200 - y[::2, ::2].astype(np.int32) // 3 + rng.integers(-4, 5, (H // 2, W // 2))).clip(0, 255).astype(np.uint8)
    return (y, cb, cr)


def _blocks(lg):
    n = 1 << lg
    return [(x, y) for y in range(0, H, n) for x in range(0, W, n)]


@functools.lru_cache(maxsize=None)
def _ref_luma(kind, lg):
    """The oracle's luma predictions: {(x, y, mode): (n, n)}; computed once per content and size, never changed."""
    from oracle import pyoracle as po
    keys = [(x, y, m) for (x, y) in _blocks(lg) for m in range(67)]
    preds = po.predict_blocks(*_planes(kind), np.array([(x, y, lg, 0, 0, m) for (x, y, m) in keys], np.int32))
    return {k: np.asarray(p) for k, p in zip(keys, preds)}


@functools.lru_cache(maxsize=None)
def _ref_chroma(kind, lg):
    """The oracle's predictions of the Cb+Cr pair of a CU of log2 size lg: {(x, y, mode): (2, n/2, n/2)}."""
    from oracle import pyoracle as po
    keys = [(x, y, m) for (x, y) in _blocks(lg) for m in list(range(67)) + CCLM]
    items = [(x, y, lg, 0, pc, m) for (x, y, m) in keys for pc in (1, 2)]
    preds = po.predict_blocks(*_planes(kind), np.array(items, np.int32))
    return {k: np.stack(preds[2 * i:2 * i + 2]) for i, k in enumerate(keys)}


def _org_luma(kind, x, y, lg):
    n = 1 << lg
    return _planes(kind)[0][y:y + n, x:x + n].astype(np.int16)


def _org_chroma(kind, x, y, lg):
    n = 1 << (lg - 1)
    p = _planes(kind)
    return np.stack([p[pc][y // 2:y // 2 + n, x // 2:x // 2 + n] for pc in (1, 2)]).astype(np.int16)


def _run(kind, items):
    from wrenc_amd import gpu
    enc = gpu.Encoder(W, H, qp=32, max_split_depth=3)
    got = enc.predict_full_blocks(*_planes(kind), np.array(items, np.int32))
    enc.close()
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", [3, 4, 5])
def test_luma_block_into_the_tile(built, kind, lg):
    ref = _ref_luma(kind, lg)
    items = [(x, y, lg, 8, m) for (x, y, m) in ref]
    for item, (pred, res) in zip(items, _run(kind, items)):
        x, y, _, _, m = item
        assert np.array_equal(pred, ref[(x, y, m)]), (kind, item)
        assert np.array_equal(res, _org_luma(kind, x, y, lg) - ref[(x, y, m)].astype(np.int16)), (kind, item)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", [3, 4, 5])   # pairs of 4x4 (the final pass of an 8x8 CU), 8x8 and 16x16 blocks
def test_chroma_pair_into_the_tile(built, kind, lg):
    ref = _ref_chroma(kind, lg)
    items = [(x, y, lg, 9, m) for (x, y, m) in ref]
    for item, (pred, res) in zip(items, _run(kind, items)):
        x, y, _, _, m = item
        assert np.array_equal(pred, ref[(x, y, m)]), (kind, item)
        assert np.array_equal(res, _org_chroma(kind, x, y, lg) - ref[(x, y, m)].astype(np.int16)), (kind, item)


def _packs(width):
    """Candidate lists of a pack of up to `width`: every mode 0..66 in order, every placement of a candidate that is not
    evaluated, and candidates that mix horizontal (< 34) and vertical modes, PDPC kinds and PLANAR / DC."""
    modes = list(range(67))
    packs = [modes[i:i + width] for i in range(0, 67, width)]
    if width == 3:
        packs += [[NO, 7, 61], [7, NO, 61], [7, 61, NO], [NO, NO, 30], [NO, 44, NO], [12, NO, NO], [NO, 1], [0, NO], [NO],
                  [10, 50, 26], [58, 2, 34], [18, 66, 1], [0, 17, 51], [40, 5]]
    else:
        packs += [[NO, 7], [61, NO], [NO], [NO, NO], [10, 50], [60, 3], [18, 66], [0, 17], [51, 1], [34, 2]]
    return packs


def _zero_or(ref, key, shape):
    return np.zeros(shape, np.uint8) if key[2] == NO else ref[key]


@pytest.mark.parametrize("kind", KINDS)
def test_luma_of_an_8x8_pack_into_its_park(built, kind):
    from wrenc_amd import gpu
    ref = _ref_luma(kind, 3)
    packs = _packs(3)
    items = [(x, y, 3, 10, gpu.Encoder.pack_modes(p)) for (x, y) in _blocks(3) for p in packs]
    cands = [p for _ in _blocks(3) for p in packs]
    for item, p, (pred, res) in zip(items, cands, _run(kind, items)):
        x, y = item[:2]
        assert pred.shape == (len(p), 8, 8)
        for cd, m in enumerate(p):
            want = _zero_or(ref, (x, y, m), (8, 8))
            assert np.array_equal(pred[cd], want), (kind, (x, y), p, cd)
            want_res = np.zeros((8, 8), np.int16) if m == NO else _org_luma(kind, x, y, 3) - want.astype(np.int16)
            assert np.array_equal(res[cd], want_res), (kind, (x, y), p, cd)


@pytest.mark.parametrize("kind", KINDS)
def test_16x16_pack_into_its_park(built, kind):
    from wrenc_amd import gpu
    ref_y, ref_c = _ref_luma(kind, 4), _ref_chroma(kind, 4)
    packs = _packs(2)
    items = [(x, y, 4, 11, gpu.Encoder.pack_modes(p)) for (x, y) in _blocks(4) for p in packs]
    cands = [p for _ in _blocks(4) for p in packs]
    for item, p, (pred, res) in zip(items, cands, _run(kind, items)):
        x, y = item[:2]
        assert pred[0].shape == (len(p), 16, 16) and pred[1].shape == (len(p), 2, 8, 8)
        for cd, m in enumerate(p):
            want_y, want_c = _zero_or(ref_y, (x, y, m), (16, 16)), _zero_or(ref_c, (x, y, m), (2, 8, 8))
            assert np.array_equal(pred[0][cd], want_y), (kind, (x, y), p, cd)
            assert np.array_equal(pred[1][cd], want_c), (kind, (x, y), p, cd)
            if m == NO:
                assert not res[0][cd].any() and not res[1][cd].any(), (kind, (x, y), p, cd)
            else:
                assert np.array_equal(res[0][cd], _org_luma(kind, x, y, 4) - want_y.astype(np.int16)), (kind, (x, y), p, cd)
                assert np.array_equal(res[1][cd], _org_chroma(kind, x, y, 4) - want_c.astype(np.int16)), (kind, (x, y), p, cd)
