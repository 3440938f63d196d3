"""Inputs that pin the coefficient scan of the quantiser kernels (wrenc_amd/csrc/dev_scan.h, dev_quant.h), and what
the oracle makes of them.  tests/test_gpu_scan_order.py sends the same blocks through every entry point of the search.

(a) Impulse blocks: one coefficient, every other zero, at every raster position of 4x4, 8x8, 16x16 and 32x32.  The oracle
    keeps exactly that position, so a device that gathered or wrote back through a wrong scan index puts the level
    somewhere else -- or, with a wrong sub-block, starts its trace in the wrong place.
(b) Dense blocks: pairwise distinct magnitudes at all positions, such that the sixteen levels of every 4x4 sub-block of
    the oracle's output are pairwise distinct: exchanging any two positions of a sub-block changes the output.

Nothing here comes from device code; the properties are asserted on the oracle's output for every block generated."""
import functools

import numpy as np
import pytest

import quant_inputs as qi

QPS = (22, 32, 42)
SIZES = qi.SIZES
DENSE_PER_SIZE = 2
IMPULSE_LEVEL = 4       # the level the lone coefficient aims at: far from zero at every QP and size, inside 16 bits
DENSE_CLASSES = 8       # magnitudes per sub-block; each with either sign: sixteen values
DENSE_SEED = 7301       # chosen on the CPU: the sixteen levels of every sub-block differ in the oracle's output, at QP 42 and
                        # 4x4 too, where 16 bits hold the eight classes only one level apart (the test below asserts it)


def impulse_amplitude(qp, n):
    return qi.coef_for_level(IMPULSE_LEVEL, qp, n)


def impulse_blocks(qp, n):
    """(n * n, n, n): block i holds its one coefficient at raster position i, signs alternating like a checkerboard."""
    a = impulse_amplitude(qp, n)
    out = np.zeros((n * n, n, n), np.int16)
    for i in range(n * n):
        y, x = divmod(i, n)
        out[i, y, x] = -a if (x + y) & 1 else a
    return out


def dense_step(qp, n):
    """Distance of two magnitude classes of a dense block: four quotient units (two levels) plus room for the per-sub-block
    offsets that keep all magnitudes of the block apart; two quotient units where 16 bits do not hold eight such classes."""
    unit = max(1, qi.level_scale(qp) >> qi.shift(n))      # coefficient units per quotient unit
    room = 2 * (n // 4) ** 2
    step = 4 * unit + room
    return step if DENSE_CLASSES * step + room <= 30000 else 2 * unit + room


def dense_block(qp, n, seed):
    """Every sub-block holds the classes 1 .. 8 with either sign in an order of its own draw; class k of sub-block j is
    the magnitude k * step + 2 j (+ 1 if negative): no two positions of the block share a magnitude."""
    rng = np.random.default_rng(DENSE_SEED + 100 * seed + qp + 1000 * n)
    step = dense_step(qp, n)
    g = n // 4
    b = np.zeros((n, n), np.int16)
    for j in range(g * g):
        sy, sx = divmod(j, g)
        for i, slot in enumerate(rng.permutation(16)):
            y, x = divmod(i, 4)
            k, neg = int(slot) // 2 + 1, int(slot) & 1
            mag = k * step + 2 * j + neg
            b[4 * sy + y, 4 * sx + x] = -mag if neg else mag
    return b


def dense_blocks(qp, n):
    return np.stack([dense_block(qp, n, s) for s in range(DENSE_PER_SIZE)])


def equal_pairs_in_sub_blocks(levels):
    """Pairs of positions of one 4x4 sub-block whose exchange leaves the block of levels as it is."""
    n = levels.shape[0]
    count = 0
    for sy in range(0, n, 4):
        for sx in range(0, n, 4):
            v = levels[sy:sy + 4, sx:sx + 4].ravel()
            count += sum(int(v[a] == v[b]) for a in range(16) for b in range(a + 1, 16))
    return count


@functools.lru_cache(maxsize=None)
def reference(kind, qp, n):
    """(blocks, the oracle's levels, the oracle's level costs) of impulse_blocks or dense_blocks: computed once per
    process and shared; callers do not write to them."""
    from oracle import pyoracle as po
    blocks = impulse_blocks(qp, n) if kind == "impulse" else dense_blocks(qp, n)
    levels = np.stack([po.quantize(b, qp) for b in blocks])
    cost = np.array([po.level_cost(l) for l in levels], np.int64)
    for a in (blocks, levels, cost):
        a.setflags(write=False)
    return blocks, levels, cost


@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("n", SIZES)
def test_impulses_stay_where_they_are(qp, n):
    blocks, levels, cost = reference("impulse", qp, n)
    assert blocks.shape == (n * n, n, n)
    for i in range(n * n):
        assert np.count_nonzero(blocks[i]) == 1 and blocks.reshape(n * n, -1)[i, i] != 0, (qp, n, i)
        nz = np.flatnonzero(levels[i])
        assert nz.tolist() == [i], (qp, n, i, nz)
    assert (cost > 0).all()


@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("n", SIZES)
def test_dense_blocks_tell_every_exchange_inside_a_sub_block(qp, n):
    blocks, levels, cost = reference("dense", qp, n)
    assert len(blocks) == DENSE_PER_SIZE
    for b, l in zip(blocks, levels):
        mags = np.abs(b.astype(np.int64)).ravel()
        assert len(set(mags.tolist())) == n * n and mags.min() > 0, (qp, n)
        assert equal_pairs_in_sub_blocks(l) == 0, (qp, n)
    assert not np.array_equal(blocks[0], blocks[1])
