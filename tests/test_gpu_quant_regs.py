"""The quantiser entry points (wrenc_amd/csrc/dev_quant.h) against the oracle's literal search on the blocks of
quant_regs_inputs.py: quotients of both parities at every position of a sub-block, levels on both sides of the tables'
LDS edge in one lane and in all, heads whose test passes (at every start of a trace) and fails, single coefficients at
either end of the scan, all-zero chroma beside luma, and zeros kept inside the trailing run at a sub-block's first
position.  test_quant_regs_inputs.py holds, on the CPU, that the blocks reach those cases in the oracle; nothing
expected here comes from device code.  One context and one oracle result per block for the whole module."""
import numpy as np
import pytest

import quant_inputs as qi
import quant_regs_inputs as ri

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc(built):
    from wrenc_amd import gpu
    e = gpu.Encoder(64, 64, qp=ri.QP, max_split_depth=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle(built):
    from oracle import pyoracle as po
    seen = {}

    def ref(b):
        key = (b.shape[0], b.tobytes())
        if key not in seen:
            lev = po.quantize(b, ri.QP)
            seen[key] = (lev, po.level_cost(lev), po.dequantize(lev, ri.QP))
        return seen[key]
    return ref


@pytest.mark.parametrize("log2n,nc", qi.PACKS)
def test_quantize_pk(enc, oracle, log2n, nc):
    n, nch = 1 << log2n, 1 << (log2n - 1)
    luma, chroma = ri.pack_plan(log2n, nc)
    n_packs = len(luma) // nc
    assert n_packs <= 64
    levels, cost = enc.quantize_pk(qi.pack_array([b for _, b in luma], [b for _, b in chroma], nc), log2n, nc)
    for p in range(n_packs):
        at = 0
        for c in range(nc):
            name, b = luma[p * nc + c]
            ref, ref_cost, _ = oracle(b)
            assert np.array_equal(levels[p, at:at + n * n].reshape(n, n), ref), (p, c, name)
            assert int(cost[p, c, 0]) == ref_cost, (p, c, name, "cost")
            at += n * n
        for c in range(nc):
            want = 0
            for pl in range(2):
                name, b = chroma[(p * nc + c) * 2 + pl]
                ref, ref_cost, _ = oracle(b)
                assert np.array_equal(levels[p, at:at + nch * nch].reshape(nch, nch), ref), (p, c, pl, name)
                want += ref_cost
                at += nch * nch
            assert int(cost[p, c, 1]) == want, (p, c, "chroma cost")
    print("(%d, %d): %d packs compared" % (log2n, nc, n_packs))


def _check_blocks(enc, oracle, named, packed):
    arr = np.stack([b for _, b in named])
    assert len(named) <= 64
    got, cost = enc.quantize_p16(arr) if packed else enc.quantize(arr)
    deq = enc.dequantize(got)
    for i, (name, b) in enumerate(named):
        ref, ref_cost, ref_deq = oracle(b)
        assert np.array_equal(got[i], ref), (i, name)
        assert int(cost[i]) == ref_cost, (i, name, "cost")
        assert np.array_equal(deq[i], ref_deq), (i, name, "dequantised")


@pytest.mark.parametrize("log2n", (2, 3, 4, 5))
def test_quantize(enc, oracle, log2n):
    _check_blocks(enc, oracle, ri.pool(1 << log2n), False)


def test_quantize_p16(enc, oracle):
    src = ri.pool(4)
    _check_blocks(enc, oracle, src + src[::-1][1:], True)     # an odd count: a partial last group of four, every order of neighbours


@pytest.mark.parametrize("n", (4, 8, 16))
def test_quantize_nb(enc, oracle, n):
    pairs = ri.pair_plan(n)
    assert len(pairs) <= 64
    levels, cost, any_level = enc.quantize_groups(np.stack([np.stack([a, b]) for (_, a), (_, b) in pairs]))
    for g, pair in enumerate(pairs):
        want, some = 0, False
        for i, (name, b) in enumerate(pair):
            ref, ref_cost, _ = oracle(b)
            assert np.array_equal(levels[g, i], ref), (g, i, name)
            want += ref_cost
            some = some or bool(ref.any())
        assert int(cost[g]) == want, (g, "cost")
        assert bool(any_level[g]) == some, (g, "any_level")
