"""The device functions the search calls on more than one block at a time, at block level against the oracle:
quantize_solo's two-block path (the Cb + Cr pair of every CU: wrenc_amd/csrc/dev_quant.h) and fwd_dct_lg / inv_dct_lg /
dequantize_t on groups of blocks at a base offset (dev_transform.h, dev_quant.h), through the wrenc_gpu_test_*_nb entries.

Every expectation is exact and comes from the oracle block by block (po.quantize, po.level_cost, po.dequantize, po.fwd_dct,
po.inv_dct): a pair's cost is the sum of its blocks' costs, its `any` is "some level of the pair is non-zero", and a pair's
levels are also what Encoder.quantize gives the two blocks alone -- a block must not depend on its partner.
tests/pair_inputs.py builds the inputs and test_pair_inputs.py holds them against the oracle on the CPU."""
import numpy as np
import pytest

import pair_inputs as pi
import quant_inputs as qi

pytestmark = pytest.mark.gpu

EINVAL, ELEVEL = -1, -6   # WRENC_GPU_EINVAL, WRENC_GPU_ELEVEL


def _check_pairs(e, oracle, pairs, what):
    """quantize_groups of a list of pairs of equal-sized blocks against the oracle, the one-block entry and -- through
    dequantize_groups -- the oracle's dequantised levels; returns the pairs compared."""
    arr = np.stack([np.stack(p) for p in pairs])
    got = e.quantize_groups(arr)
    diff = pi.differences(got, pi.expected(pairs, oracle))
    assert diff == [], (what, diff[:4])
    alone, alone_cost = e.quantize(arr.reshape((-1,) + arr.shape[2:]))
    assert np.array_equal(alone.reshape(arr.shape), got[0]), (what, "a block depends on its partner")
    assert np.array_equal(alone_cost.reshape(-1, 2).sum(axis=1), got[1]), (what, "cost against the one-block entry")
    deq = e.dequantize_groups(got[0])
    for i, pair in enumerate(pairs):
        for j, b in enumerate(pair):
            assert np.array_equal(deq[i, j], oracle(b)[2]), (what, i, j, "dequantised")
    return len(pairs)


@pytest.mark.parametrize("qp", pi.QPS)
def test_the_mixtures_of_kinds(built, qp):
    """Every ordered pair of zero, quiet, live, low and stray blocks at side 4, 8 and 16: a block proven zero from end to
    end beside one that needs its whole chain, heads that end at different sub-blocks (test_pair_inputs.py reads where each
    walk ends off the oracle's model), and every other mixture; each pair once more with its two blocks exchanged in
    the same call."""
    from wrenc_amd import gpu
    oracle = pi.Oracle(qp)
    compared = 0
    e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
    try:
        for n in pi.SIDES:
            pairs = [blocks for _, blocks in pi.mixtures(qp, n)]
            assert len(pairs) == 25
            compared += _check_pairs(e, oracle, pairs + [p[::-1] for p in pairs], (qp, n))
    finally:
        e.close()
    print("qp %d: %d pairs compared" % (qp, compared))


@pytest.mark.parametrize("qp", range(64))
def test_pairs_of_every_class_at_every_qp(built, qp):
    """The blocks of test_every_entry_point_at_every_qp (test_gpu_quant_bounds.py) as pairs, each list against itself reversed
    and rotated so that every class meets another one in both positions: levels, summed cost, `any` and the dequantised
    levels of every pair at side 4, 8 and 16 equal the oracle's.  Both positions hold every class the 16-bit range allows
    at that QP and size, asserted here of what is sent."""
    from wrenc_amd import gpu
    oracle = pi.Oracle(qp)
    counts, compared = {}, 0
    e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
    try:
        for n in pi.SIDES:
            first, second = pi.qp_pairs(qp, n)
            for part in (first, second):
                refs = [oracle(b)[0] for _, b in part]
                assert qi.missing_classes(qp, n, part, refs) == [], (qp, n)
            qi.class_counts(qp, first, [oracle(b)[0] for _, b in first], counts)
            compared += _check_pairs(e, oracle, [(a, b) for (_, a), (_, b) in zip(first, second)], (qp, n))
    finally:
        e.close()
    print("qp %d: %d pairs compared, classes per position %s" % (qp, compared, sorted(counts.items())))


@pytest.mark.parametrize("qp,extra", qi.BOUND_MODELS)
def test_pairs_built_against_the_stated_bounds(built, qp, extra):
    """The blocks of nothing but the maximum magnitude and its relatives (quant_inputs.bound_blocks) beside themselves, beside
    a zero block and beside +-3 noise, in both positions, at both ends of the QP range, under the two rate models at the
    edge of what wrenc_gpu_create accepts and at the QPs where the maximum is a level of 900 and more: the two walkers'
    shared renormalisation and the shared cost sum at the ends of the 32-bit range."""
    from wrenc_amd import gpu
    oracle = pi.Oracle(qp)
    oracle.po.set_extra_params(extra)
    e = None
    compared = 0
    try:
        e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0, extra_params=extra)
        for n in pi.SIDES:
            named = pi.bound_pairs(qp, n)
            for name, pair in named:
                top = max(int(qi.trellis_levels(oracle(b)[0]).max()) for b in pair)
                assert qi.bound_level_floor(qp, n) <= top <= 1023, (qp, extra, n, name, top)
            compared += _check_pairs(e, oracle, [pair for _, pair in named], (qp, extra, n))
    finally:
        if e is not None:
            e.close()
        oracle.po.set_extra_params(None)
    print("qp %d %s: %d pairs compared" % (qp, extra, compared))


@pytest.mark.parametrize("n", pi.SIDES)
def test_the_level_limit_in_either_block(built, n):
    """A coefficient at the tables' last entry in block 0 or in block 1, beside a harmless block, compares equal and raises
    nothing; one step larger and the entry returns WRENC_GPU_ELEVEL whichever block holds it (the oracle raises for that
    block and not for its partner: test_pair_inputs.py); the next call on the same context succeeds and compares equal.
    At the two largest QPs at which 16 bits pass the limit at that size."""
    from wrenc_amd import gpu
    compared = 0
    for qp in qi.limit_qps(n):
        oracle = pi.Oracle(qp)
        e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
        try:
            for seed in range(pi.LIMIT_SEEDS):
                at, over = pi.limit_pairs(qp, n, seed)
                for pair in at:                                   # one pair per call: no partner pair to hide behind
                    compared += _check_pairs(e, oracle, [pair], (n, qp, seed, "at the limit"))
                for where, pair in enumerate(over):
                    with pytest.raises(gpu.WrencGpuError) as err:
                        e.quantize_groups(np.stack([np.stack(pair)]))
                    assert err.value.code == ELEVEL, (n, qp, seed, where, err.value)
                    compared += _check_pairs(e, oracle, [at[where]], (n, qp, seed, where, "after the refusal"))
                with pytest.raises(gpu.WrencGpuError) as err:     # ... and among other pairs of one call
                    e.quantize_groups(np.stack([np.stack(p) for p in at + over[1:] + at]))
                assert err.value.code == ELEVEL, (n, qp, seed, err.value)
                compared += _check_pairs(e, oracle, at, (n, qp, seed, "after the refusal of a call of five"))
        finally:
            e.close()
    print("%d: %d pairs compared" % (n, compared))


@pytest.fixture(scope="module")
def enc(built):
    from wrenc_amd import gpu
    e = gpu.Encoder(64, 64, qp=32, max_split_depth=0)
    yield e
    e.close()


def _against_blocks(got, groups, ref, alone, what):
    """A group entry's output against the oracle block by block and against the one-block entry; returns the groups."""
    flat = groups.reshape((-1,) + groups.shape[2:])
    single = alone(flat).reshape(groups.shape)
    for g in range(groups.shape[0]):
        for j in range(groups.shape[1]):
            assert np.array_equal(got[g, j], ref(groups[g, j])), (what, g, j)
    assert np.array_equal(got, single), (what, "against the one-block entry")
    return groups.shape[0]


@pytest.mark.parametrize("log2n,nb,o1", pi.TRANSFORM_SHAPES)
def test_transform_and_dequantiser_groups(enc, log2n, nb, o1):
    """fwd_dct_lg, inv_dct_lg and dequantize_t on the groups the search hands them -- the chroma pair of an 8x8, 16x16 and
    32x32 CU (two 16x16 blocks: the forward transform's block-after-block branch), the luma blocks of a pack, the chroma
    of a 16x16 pack behind its luma at r1[256] and r1[512] -- with every block of a group another kind (all +255, all
    -255, the checkerboard, zero, noise; for the inverse +-32767 and a single row of 32767 beside small blocks): a value
    that leaks into the neighbour or a wrong round of the branch shows.  Also at base offset 0 where the shape has one."""
    from oracle import pyoracle as po
    compared = 0
    for at in sorted({0, o1}):
        res = pi.residual_groups(log2n, nb)
        compared += _against_blocks(enc.fwd_dct_groups(res, at), res, po.fwd_dct, enc.fwd_dct, ("fwd", log2n, nb, at))
        coef = pi.coef_groups(log2n, nb)
        compared += _against_blocks(enc.inv_dct_groups(coef, at), coef, po.inv_dct, enc.inv_dct, ("inv", log2n, nb, at))
        lev = pi.level_groups(log2n, nb)
        compared += _against_blocks(enc.dequantize_groups(lev, at), lev, lambda b: po.dequantize(b, 32), enc.dequantize,
                                    ("dequantize", log2n, nb, at))
    print("(%d, %d, %d): %d groups compared" % (log2n, nb, o1, compared))


def test_the_chain_of_a_pair(enc):
    """The chroma pair through the whole chain its caller runs: forward transform, quantiser, dequantiser, inverse
    transform, each on the pair, each stage's output the next one's input, against the oracle's chain block by block."""
    from oracle import pyoracle as po
    for log2n in (2, 3, 4):
        res = pi.residual_groups(log2n, 2)
        coef = enc.fwd_dct_groups(res)
        levels, cost, any_level = enc.quantize_groups(coef)
        rec = enc.inv_dct_groups(enc.dequantize_groups(levels))
        for g in range(res.shape[0]):
            want_cost = 0
            for j in range(2):
                ref = po.quantize(po.fwd_dct(res[g, j]), 32)
                want_cost += po.level_cost(ref)
                assert np.array_equal(levels[g, j], ref), (log2n, g, j)
                assert np.array_equal(rec[g, j], po.inv_dct(po.dequantize(ref, 32))), (log2n, g, j)
            assert int(cost[g]) == want_cost and bool(any_level[g]) == bool(levels[g].any()), (log2n, g)


def test_what_the_group_entries_refuse(enc):
    """WRENC_GPU_EINVAL before any launch for what the device code is not written for (include/wrenc_gpu.h): a quantiser
    group of other than one or two blocks, a 32x32 block with company, an odd or negative base offset, a group that leaves
    r1 behind its offset or r2, a 32x32 residual outside 9 bits; the context stays usable."""
    from wrenc_amd import gpu

    def refused(call, *args):
        with pytest.raises(gpu.WrencGpuError) as err:
            call(*args)
        assert err.value.code == EINVAL, (call.__name__, err.value)

    def z(nb, n):
        return np.zeros((1, nb, n, n), np.int16)
    transforms = (enc.fwd_dct_groups, enc.inv_dct_groups, enc.dequantize_groups)
    refused(enc.quantize_groups, z(3, 4))
    refused(enc.quantize_groups, z(0, 4))
    refused(enc.quantize_groups, z(2, 32))
    for call in transforms:
        refused(call, z(0, 8))
        refused(call, z(2, 32))
        refused(call, z(2, 8), 1)
        refused(call, z(2, 8), 255)
        refused(call, z(2, 8), -2)
        refused(call, z(2, 8), 898)          # 898 + 128 > 1024
        refused(call, z(1, 32), 2)
        refused(call, z(5, 16))              # 5 * 256 > 1024: r2
        refused(call, z(4, 16), 2)
        assert not call(z(2, 8), 896).any()  # the last place a pair of 8x8 blocks fits
        assert not call(z(4, 16)).any()
    big = z(1, 32)
    big[0, 0, 3, 3] = 256
    refused(enc.fwd_dct_groups, big)
    assert not enc.quantize_groups(z(2, 16))[0].any()
