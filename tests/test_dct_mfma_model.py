"""The 8x8 and 16x16 transforms as i8 MFMAs (wrenc_amd/csrc/dev_transform.h fwd_dct_mfma / inv_dct_mfma), modelled in numpy
lane by lane (tests/dct_mfma_model.py) and held against the oracle, with no tolerance; and the magnitude of every
intermediate of the model against the bounds the device code states: digits and bytes in i8, every sum in i32.  Runs without
a device; tests/test_gpu_dct_mfma.py runs the same inputs through the kernels."""
import numpy as np
import pytest

import dct_mfma_model as mm
from oracle import pyoracle as po

I32 = 2 ** 31 - 1


def _run(model, oracle, blocks, n):
    """every block alone, then groups of 2, 3, 4 and (one round more than an MFMA holds) 5 blocks of different kinds"""
    bounds = mm.Bounds()
    names = list(blocks)
    want = {k: oracle(blocks[k]) for k in names}
    for k in names:
        got = model(blocks[k][None], bounds)
        assert np.array_equal(got[0], want[k]), "%dx%d %s" % (n, n, k)
    for nb in (2, 3, 4, 5):
        groups = mm.as_groups([blocks[k] for k in names], nb)
        for g in range(0, len(groups), 37):               # a sample of the groups: the device test runs all of them
            got = model(groups[g], bounds)
            for i in range(nb):
                k = names[(g + i * max(len(names) // nb, 1)) % len(names)]
                assert np.array_equal(got[i], want[k]), "%dx%d group %d of %d, block %d (%s)" % (n, n, g, nb, i, k)
    return bounds


@pytest.mark.parametrize("n", [8, 16])
def test_forward_model_equals_the_oracle_and_keeps_its_bounds(n):
    blocks = mm.fwd_inputs(n)
    assert all(np.abs(b.astype(np.int64)).max() <= 255 for b in blocks.values())
    b = _run(mm.fwd_model, po.fwd_dct, blocks, n)
    s = mm.basis_abs_row_sum(n)
    assert s == 64 * n, "the bounds in dev_transform.h take S = 64 N"
    # what dev_transform.h states (and its static_asserts use)
    assert b.worst["fwd stage-1 digit"][0] >= -128 and b.worst["fwd stage-1 digit"][1] <= 127
    assert b.mag("fwd stage 1 sum of |products|") <= 128 * s
    assert b.mag("fwd H") <= 32640                         # all +-255 reaches it: (255 * 64 N + d) >> (LG - 1)
    assert b.mag("fwd H") == 32640
    assert b.mag("fwd stage-2 digit 2") <= 1
    # before the last digit's product the chained accumulator is the whole sum less that product, |P0| <= 128 S
    assert b.mag("fwd stage 2 shifted") <= 32640 * s + 128 * s + (1 << 10)
    for name, (lo, hi) in b.worst.items():
        assert -I32 - 1 <= lo and hi <= I32, name
    assert b.mag("fwd stage 2 sum of |products|") <= 32640 * s + 128 * s + (1 << 10) + 128 * s


@pytest.mark.parametrize("n", [8, 16])
def test_inverse_model_equals_the_oracle_and_keeps_its_bounds(n):
    blocks = mm.inv_inputs(n)
    b = _run(mm.inv_model, po.inv_dct, blocks, n)
    s = mm.basis_abs_row_sum(n)
    assert int(np.abs(mm.basis(n)).sum(axis=0).max()) <= s  # (the inverse contracts over the basis' columns)
    assert b.mag("inv stage 1 sum of |products|") <= 128 * s and b.mag("inv stage 2 sum of |products|") <= 128 * s + 128 * s + 2048
    assert b.mag("inv stage 1 recombined") <= 32768 * s + 128 * s + 64
    assert b.mag("inv stage 2 recombined") <= 32768 * s + 128 * s + 2048
    for name, (lo, hi) in b.worst.items():
        assert -I32 - 1 <= lo and hi <= I32, name


@pytest.mark.parametrize("n", [8, 16])
def test_a_block_past_the_group_or_beside_it_leaves_no_trace(n):
    """the same block alone and as every member of a group of other kinds: the same coefficients / residuals"""
    f, i = mm.fwd_inputs(n), mm.inv_inputs(n)
    for model, blocks, probe in ((mm.fwd_model, f, "noise0"), (mm.inv_model, i, "full0")):
        alone = model(blocks[probe][None], mm.Bounds())[0]
        others = [blocks[k] for k in list(blocks)[:3]]
        for nb in (2, 3, 4):
            for at in range(nb):
                g = [others[j % 3] for j in range(nb)]
                g[at] = blocks[probe]
                assert np.array_equal(model(np.stack(g), mm.Bounds())[at], alone)


def test_the_model_rejects_a_transposed_operand():
    """what the impulse cases are for: with the first stage's basis operand transposed, off-diagonal values move"""
    n = 8
    t = mm.tables(n)
    saved = t["fdct_b"].copy()
    try:
        for m in range(32):
            for h in range(2):
                for j in range(16):
                    if m // n == 2 * h + j // 8:
                        t["fdct_b"][m, h, j] = mm.basis(n)[j % 8, m % n]
        blk = mm.fwd_inputs(n)["impulse+255@1,2"]
        assert not np.array_equal(mm.fwd_model(blk[None], mm.Bounds())[0], po.fwd_dct(blk))
    finally:
        t["fdct_b"][...] = saved
    assert np.array_equal(mm.fwd_model(blk[None], mm.Bounds())[0], po.fwd_dct(blk))
