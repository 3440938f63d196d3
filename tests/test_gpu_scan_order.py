"""The scan order of the quantiser kernels (wrenc_amd/csrc/dev_scan.h through dev_quant.h) against the oracle, position
by position: the impulse and dense blocks of tests/test_scan_inputs.py through every entry point the search uses --
quantize at 4 .. 32, quantize_p16 with a partial last wavefront, quantize_pk at (3; 1, 2, 3 candidates) and (4; 1, 2) with
the impulse in every position of every luma and chroma block of every candidate.  An impulse ends the proven-zero head
at its own sub-block, so the traces start at every sub-block and share what is left 1, 2, 4, 8 or 16 positions to a
lane.  Levels and level cost must equal the oracle's; nothing expected here comes from device code."""
import numpy as np
import pytest

import test_scan_inputs as si

pytestmark = pytest.mark.gpu

PACKS = ((3, 1), (3, 2), (3, 3), (4, 1), (4, 2))


def _encoder(qp):
    from wrenc_amd import gpu
    return gpu.Encoder(64, 64, qp=qp, max_split_depth=0)


def _assert_blocks(got, cost, levels, ref_cost, what):
    if not np.array_equal(got, levels):
        i = int(np.flatnonzero((got != levels).reshape(len(got), -1).any(axis=1))[0])
        raise AssertionError("%s: block %d: levels at raster %s, the oracle's at %s" % (
            what, i, np.flatnonzero(got[i]).tolist()[:8], np.flatnonzero(levels[i]).tolist()[:8]))
    assert np.array_equal(np.asarray(cost, np.int64), ref_cost), (what, "level cost")


@pytest.mark.parametrize("qp", si.QPS)
@pytest.mark.parametrize("n", si.SIZES)
def test_quantize(built, qp, n):
    e = _encoder(qp)
    try:
        for kind in ("impulse", "dense"):
            blocks, levels, ref_cost = si.reference(kind, qp, n)
            got, cost = e.quantize(blocks)
            _assert_blocks(got, cost, levels, ref_cost, ("quantize", kind, qp, n))
    finally:
        e.close()


@pytest.mark.parametrize("qp", si.QPS)
def test_quantize_p16(built, qp):
    """Four blocks per wavefront: 16 impulses and 2 dense blocks are four full wavefronts and one of two blocks; the
    same without the first block ends on one of a single block, without the first three on one of three."""
    imp, imp_lv, imp_cost = si.reference("impulse", qp, 4)
    den, den_lv, den_cost = si.reference("dense", qp, 4)
    blocks, levels, ref_cost = np.concatenate([imp, den]), np.concatenate([imp_lv, den_lv]), np.concatenate([imp_cost, den_cost])
    e = _encoder(qp)
    try:
        for skip in (0, 1, 3):
            assert (len(blocks) - skip) % 4 == (2, 1, 3)[(0, 1, 3).index(skip)]
            got, cost = e.quantize_p16(blocks[skip:])
            _assert_blocks(got, cost, levels[skip:], ref_cost[skip:], ("quantize_p16", qp, skip))
    finally:
        e.close()


def _packs(qp, log2n, nc):
    """(packs, expected levels, expected cost[n_packs, nc, 2]): per candidate and per block of it (luma, Cb, Cr) one pack
    for every position of that block, the impulse there and every other block of the pack zero; then packs of dense
    blocks alone."""
    n, nch = 1 << log2n, 1 << (log2n - 1)
    pl, pc = n * n, nch * nch
    limp, limp_lv, limp_cost = si.reference("impulse", qp, n)
    cimp, cimp_lv, cimp_cost = si.reference("impulse", qp, nch)
    lden, lden_lv, lden_cost = si.reference("dense", qp, n)
    cden, cden_lv, cden_cost = si.reference("dense", qp, nch)
    width = nc * (pl + 2 * pc)
    packs, want, cost = [], [], []
    for c in range(nc):
        for at, count, src, lv, cst, col in ((c * pl, pl, limp, limp_lv, limp_cost, 0),
                                             (nc * pl + (2 * c) * pc, pc, cimp, cimp_lv, cimp_cost, 1),
                                             (nc * pl + (2 * c + 1) * pc, pc, cimp, cimp_lv, cimp_cost, 1)):
            a, w = np.zeros((count, width), np.int16), np.zeros((count, width), np.int16)
            a[:, at:at + count] = src.reshape(count, count)
            w[:, at:at + count] = lv.reshape(count, count)
            k = np.zeros((count, nc, 2), np.int64)
            k[:, c, col] = cst
            packs.append(a)
            want.append(w)
            cost.append(k)
    for shift in range(si.DENSE_PER_SIZE):
        a, w, k = np.zeros((1, width), np.int16), np.zeros((1, width), np.int16), np.zeros((1, nc, 2), np.int64)
        for c in range(nc):
            i = (c + shift) % si.DENSE_PER_SIZE
            a[0, c * pl:(c + 1) * pl], w[0, c * pl:(c + 1) * pl] = lden[i].ravel(), lden_lv[i].ravel()
            k[0, c, 0] = lden_cost[i]
            for plane in range(2):
                j, at = (c + shift + plane) % si.DENSE_PER_SIZE, nc * pl + (2 * c + plane) * pc
                a[0, at:at + pc], w[0, at:at + pc] = cden[j].ravel(), cden_lv[j].ravel()
                k[0, c, 1] += cden_cost[j]
        packs.append(a)
        want.append(w)
        cost.append(k)
    return np.concatenate(packs), np.concatenate(want), np.concatenate(cost)


@pytest.mark.parametrize("qp", si.QPS)
@pytest.mark.parametrize("log2n,nc", PACKS)
def test_quantize_pk(built, qp, log2n, nc):
    packs, want, want_cost = _packs(qp, log2n, nc)
    assert len(packs) == nc * 6 * (1 << (2 * log2n)) // 4 + si.DENSE_PER_SIZE
    e = _encoder(qp)
    try:
        got, cost = e.quantize_pk(packs, log2n, nc)
    finally:
        e.close()
    _assert_blocks(got, cost, want, want_cost, ("quantize_pk", qp, log2n, nc))
