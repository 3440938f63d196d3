"""The generators of tests/pair_inputs.py against the oracle alone: what test_gpu_solo_groups.py relies on -- the kinds
of block, where the head proof ends each block's walk, the classes at every QP, the bounds, the level limit, the
transform groups -- is checked here without a device, and the comparison the GPU tests use is shown to reject a swap."""
import numpy as np
import pytest

import pair_inputs as pi
import quant_inputs as qi
from oracle import pyoracle as po


def _walk(b, qp):
    """(sub-blocks of the head the oracle's model of the head proof skips, whole block proven zero) for one block; the
    model's levels equal the literal search's."""
    lg = b.shape[0].bit_length() - 1
    po.dq_sc_stats_enable(True)
    try:
        got = po.quantize_sc(b, qp, use_head=True)
        mism, stats = po.dq_sc_stats_read()
    finally:
        po.dq_sc_stats_enable(False)
    assert mism == 0 and np.array_equal(got, po.quantize(b, qp))
    assert stats[lg]["blocks"] == 1
    return stats[lg]["head_sb_skipped"], stats[lg]["whole_zero"] == 1


def _last_sub_block(levels):
    n = levels.shape[0]
    return [levels[p] for p in (qi.scan(n)[-4:] if n == 4 else qi.scan(n)[-16:])]


@pytest.mark.parametrize("qp", pi.QPS)
def test_the_five_kinds_are_what_they_claim(qp):
    """Of the oracle's output, for both places of a pair: zero has no coefficient; quiet has coefficients and no level; live
    has a level; low has levels, none outside its first LOW_K sub-blocks of the scan (the first eight positions at side 4);
    stray has a level in the last sub-block of the scan (its last four positions at side 4)."""
    for n in pi.SIDES:
        pairs = pi.mixtures(qp, n)
        assert [k for k, _ in pairs] == [(a, b) for a in pi.KINDS for b in pi.KINDS] and len(pairs) == 25
        order = qi.scan(n)
        for kinds, blocks in pairs:
            for place, (kind, b) in enumerate(zip(kinds, blocks)):
                ref = po.quantize(b, qp)
                if kind == "zero":
                    assert not b.any()
                elif kind == "quiet":
                    assert b.any() and not ref.any(), (qp, n, place)
                elif kind == "live":
                    assert ref.any(), (qp, n, place)
                else:
                    keep = 8 if n == 4 else 16 * pi.low_k(n, place)
                    assert any(ref[p] != 0 for p in order[:keep]), (qp, n, kind, place)
                    if kind == "low":
                        assert all(ref[p] == 0 for p in order[keep:]), (qp, n, kind, place)
                    else:   # (behind a stray coefficient the walk is in other states: quiet positions may get a level)
                        assert any(v != 0 for v in _last_sub_block(ref)), (qp, n, place)
                        assert max(abs(int(v)) for v in _last_sub_block(b)) >= qi.coef_for_level(3, qp, n, True) - 1


@pytest.mark.parametrize("qp", pi.QPS)
def test_where_the_walks_end(qp):
    """Read off the oracle's model of the device's shortcuts (quantize_sc with the head proof, its statistics): a quiet block
    is proven zero as a whole; the head proof skips sub-blocks of a low block and none of a stray one (a block of side 4 is
    one sub-block: nothing to skip); two low blocks side by side end at different sub-blocks; and the 25 mixtures hold the
    combinations whole-record contents do not -- a block proven zero from end to end beside one that needs its whole chain,
    in both orders, and two heads that end at different sub-blocks, neither at an end of the chain."""
    for n in pi.SIDES:
        nsb = n * n // 16
        ends = {}
        for kinds, blocks in pi.mixtures(qp, n):
            ends[kinds] = tuple(_walk(b, qp) for b in blocks)
        for (k0, k1), (w0, w1) in ends.items():
            for kind, (skipped, whole) in ((k0, w0), (k1, w1)):
                assert whole == (kind == "quiet"), (qp, n, kind)
                if kind == "stray" or n == 4:
                    assert skipped == 0, (qp, n, kind)
                elif kind == "low":
                    assert 0 < skipped < nsb, (qp, n, kind, skipped)
        assert ends[("quiet", "stray")][0][1] and ends[("quiet", "stray")][1] == (0, False)
        assert ends[("stray", "quiet")][1][1] and ends[("stray", "quiet")][0] == (0, False)
        if n > 4:
            (a, _), (b, _) = ends[("low", "low")]
            assert a != b and 0 < a < nsb and 0 < b < nsb, (qp, n, a, b)
            assert ends[("low", "stray")][0][0] > 0 == ends[("low", "stray")][1][0]


@pytest.mark.parametrize("qp", range(64))
def test_every_class_meets_another_one_in_both_positions(qp):
    """The every-QP pairs: both positions hold every class the 16-bit range allows at that QP and size (read off the
    oracle), and every class -- by the generator's tag -- sits beside a block of another class in position 0 and in
    position 1.  Cutting the draws per class to one keeps both."""
    for n in pi.SIDES:
        for seeds in (qi.CLASS_SEEDS, 1):
            first, second = pi.qp_pairs(qp, n, seeds)
            assert len(first) == len(second) and sorted(b.tobytes() for _, b in first) == sorted(b.tobytes() for _, b in second)
            for part in (first, second):
                assert qi.missing_classes(qp, n, part, [po.quantize(b, qp) for _, b in part]) == [], (qp, n, seeds)
            tags = {t for t, _ in first}
            assert {t0 for (t0, _), (t1, _) in zip(first, second) if t0 != t1} == tags, (qp, n, seeds)
            assert {t1 for (t0, _), (t1, _) in zip(first, second) if t0 != t1} == tags, (qp, n, seeds)


@pytest.mark.parametrize("qp,extra", qi.BOUND_MODELS)
def test_the_bound_pairs(qp, extra):
    """Every bound block beside itself, a zero block and noise, in both positions; the bound block of each pair holds a
    level of qi.bound_level_floor or more and none makes the oracle raise."""
    po.set_extra_params(extra)
    try:
        for n in pi.SIDES:
            pairs = pi.bound_pairs(qp, n)
            assert len(pairs) == 5 * len(qi.bound_blocks(qp, n))
            for name, pair in pairs:
                tops = [int(qi.trellis_levels(po.quantize(b, qp)).max()) for b in pair]
                assert qi.bound_level_floor(qp, n) <= max(tops) <= 1023, (qp, extra, n, name)
                if name.endswith("+self"):
                    assert np.array_equal(pair[0], pair[1])
                else:
                    assert min(tops) <= 1 or qi.bound_level_floor(qp, n) <= 1, (qp, extra, n, name)
    finally:
        po.set_extra_params(None)


def test_the_limit_pairs():
    """At the two largest QPs at which 16 bits pass the tables' end: the pairs at the limit quantise in the oracle, block by
    block, and exactly one block of every pair over it makes the oracle raise -- in position 0 and in position 1."""
    for n in pi.SIDES:
        for qp in qi.limit_qps(n):
            for seed in range(pi.LIMIT_SEEDS):
                at, over = pi.limit_pairs(qp, n, seed)
                for pair in at:
                    tables = []
                    for b in pair:
                        po.quantize(b, qp)
                        tables.append(po.last_table_index())
                    assert max(tables) == 1023, (n, qp, seed)
                raised = []
                for pair in over:
                    row = []
                    for b in pair:
                        try:
                            po.quantize(b, qp)
                            row.append(False)
                        except OverflowError:
                            row.append(True)
                    raised.append(row)
                assert raised == [[True, False], [False, True]], (n, qp, seed)


def test_the_transform_groups():
    """The shapes the search uses fit the wavefront's buffers; in the groups of every shape each kind of block sits in every
    position, the blocks of a group differ from one another, residuals stay within 9 bits, and the inverse transform's
    +-32767 blocks do reach the first stage's clip in the oracle (a single row of 32767 does not)."""
    assert len(set(pi.TRANSFORM_SHAPES)) == len(pi.TRANSFORM_SHAPES)
    for log2n, nb, o1 in pi.TRANSFORM_SHAPES:
        n = 1 << log2n
        assert o1 % 2 == 0 and o1 + nb * n * n <= 1024
        for make, kinds in ((pi.residual_groups, pi.RESIDUAL_KINDS), (pi.coef_groups, pi.COEF_KINDS), (pi.level_groups, pi.LEVEL_KINDS)):
            groups = make(log2n, nb)
            assert groups.shape == (len(kinds) + 1, nb, n, n) and groups.dtype == np.int16
            for g in groups:
                assert len({b.tobytes() for b in g}) == nb
            for j in range(nb):
                assert len({groups[r, j].tobytes() for r in range(len(kinds))}) == len(kinds)
        assert np.abs(pi.residual_groups(log2n, nb)).max() == 255
        assert np.abs(pi.level_groups(log2n, nb).astype(np.int32)).max() == 2046
        # the first stage is V[y][x] = clamp16((sum_i T[i][y] d[i][x] + 64) >> 7), T the oracle's basis
        basis = po.dct64()[::64 // n, :n].astype(np.int64)
        assert ((np.abs(basis.sum(axis=0)).max() * 32767 + 64) >> 7) > 32767
        assert ((np.abs(basis).max() * 32767 + 64) >> 7) <= 32767


@pytest.mark.parametrize("n", pi.SIDES)
def test_the_comparison_rejects_swapped_blocks(n):
    """The helper the GPU tests compare with: equal to itself, and an expected output whose two blocks changed places --
    what a kernel that mixed up its halves would deliver -- is rejected, as is a wrong cost or a wrong `any` alone."""
    qp = 32
    oracle = pi.Oracle(qp)
    kinds, pair = [(k, p) for k, p in pi.mixtures(qp, n) if k == ("live", "quiet")][0]
    want = pi.expected([pair, pair[::-1]], oracle)
    assert want[2].tolist() == [True, True] and want[1][0] == want[1][1] > 0
    assert pi.differences(want, want) == []
    swapped = (want[0][:, ::-1].copy(), want[1], want[2])
    assert not np.array_equal(swapped[0], want[0])
    assert {i for i, _ in pi.differences(swapped, want)} == {0, 1}
    assert pi.differences((want[0], want[1] + np.array([0, 1]), want[2]), want) == [(1, "cost")]
    assert pi.differences((want[0], want[1], np.array([False, True])), want) == [(0, "any")]
    # ... and `any` is the pair's, not a block's: a quiet block beside a zero one has none
    quiet = pi.expected([(pi.block("quiet", qp, n, 0), pi.block("zero", qp, n, 1))], oracle)
    assert quiet[2].tolist() == [False] and int(quiet[1][0]) == 0
