"""The generators of tests/quant_inputs.py against the oracle alone: the coverage conditions test_gpu_quant_bounds.py relies
on are checked here without a device (the GPU file asserts them again on what it actually sends)."""
import numpy as np
import pytest

import quant_inputs as qi
from oracle import pyoracle as po


def _refs(tagged, qp):
    return [po.quantize(b, qp) for _, b in tagged]


def test_step_formula_and_level_walk_are_the_oracles():
    """The helper's level scale and shift dequantise level 1 as the oracle does at every QP and size, its scan and state
    walk give the oracle's level cost, and reach() is what the oracle makes of +-32767."""
    lv = po.tables(32)[0]
    rng = np.random.default_rng(1)
    for n in qi.SIZES:
        assert sorted(qi.scan(n)) == [(y, x) for y in range(n) for x in range(n)]
        one = np.zeros((n, n), np.int16)
        one[1, 2] = 1
        for qp in range(64):
            want = min((qi.level_scale(qp) + (1 << (qi.shift(n) - 1))) >> qi.shift(n), 32767)
            assert int(po.dequantize(one, qp)[1, 2]) == want, (n, qp)
        for it in range(12):
            levels = (rng.integers(-6, 7, (n, n)) * (rng.random((n, n)) < [0.9, 0.3, 0.05][it % 3])).astype(np.int16)
            assert qi.level_cost_model(levels, lv) == po.level_cost(levels), (n, it)
        for qp in (0, 3, 17, 28, 32, 45, 63):
            if qi.quotient(32767, qp, n) >= qi.OVER_QUOTIENT:
                continue
            lone = np.zeros((n, n), np.int16)
            lone[n - 1, n - 1] = 32767      # the walk's first position: state 0, a = quotient / 2 or one more
            a = int(qi.trellis_levels(po.quantize(lone, qp)).max())
            assert a in (qi.reach(qp, n), qi.reach(qp, n) + 1), (n, qp, a)


def test_where_the_classes_are_required():
    """required_classes is the 16-bit range and the step formula, nothing else: the levels beyond the LDS tables' 256
    entries exist up to QP 32 (32x32), a level of 900 up to QP 22 (32x32), QP 4 (4x4), six QPs per doubling of the side; levels
    1 .. 8 everywhere but at 4x4 from QP 57 and 8x8 at QP 63, where 32767 is less than two levels."""
    assert [max(qp for qp in range(64) if qi.reach(qp, n) >= 900) for n in qi.SIZES] == [4, 10, 16, 22]
    assert [max(qp for qp in range(64) if "c" in qi.required_classes(qp, n)) for n in qi.SIZES] == [14, 20, 26, 32]
    assert all("c" in qi.required_classes(qp, 32) for qp in range(33))
    assert all({"a", "d", "e"} <= set(qi.required_classes(qp, n)) for qp in range(64) for n in qi.SIZES)
    assert [(qp, n) for qp in range(64) for n in qi.SIZES if "b_dense" not in qi.required_classes(qp, n)] == \
        [(qp, 4) for qp in range(57, 63)] + [(63, 4), (63, 8)]


@pytest.mark.parametrize("qp", range(64))
def test_every_class_occurs_at_every_qp_and_size(qp):
    """At every QP each required class occurs at every size -- in the blocks quantize
    and quantize_p16 get and in the luma and chroma blocks of every quantize_pk pack plan -- and no block makes the
    oracle raise."""
    for n in qi.SIZES:
        tagged = qi.qp_blocks(qp, n)
        assert qi.missing_classes(qp, n, tagged, _refs(tagged, qp)) == [], (qp, n)
    for log2n, nc in qi.PACKS:
        luma, chroma = qi.pack_plan(qp, log2n, nc)
        assert len(luma) % nc == 0 and len(chroma) == 2 * len(luma)
        assert qi.missing_classes(qp, 1 << log2n, luma, _refs(luma, qp)) == [], (qp, log2n, nc)
        assert qi.missing_classes(qp, 1 << (log2n - 1), chroma, _refs(chroma, qp)) == [], (qp, log2n, nc)


@pytest.mark.parametrize("qp,extra", qi.BOUND_MODELS)
def test_bound_blocks_hold_the_largest_levels(qp, extra):
    """Every block built against the stated bounds has a level of 900 or more, or -- where 16 bits do not reach that --
    the largest level +-32767 / -32768 give at that QP and size; none makes the oracle raise."""
    po.set_extra_params(extra)
    try:
        for n in qi.SIZES:
            for name, b in qi.bound_blocks(qp, n):
                a = qi.trellis_levels(po.quantize(b, qp))
                assert qi.bound_level_floor(qp, n) <= a.max() <= 1023, (qp, extra, n, name, int(a.max()))
                assert np.abs(b.astype(np.int32)).max() >= min(qi.top_coef(qp, n), qi.top_coef(qp, n, neg=True))
    finally:
        po.set_extra_params(None)
    if qp in (16, 22):
        assert qi.bound_level_floor(qp, 32) == 900
    assert qi.bound_level_floor(16, 16) == 900
    assert [qi.bound_level_floor(4, n) for n in qi.SIZES] == [900] * 4     # the low-QP model: the tables' end at every size
    assert 4 in [q for q, _ in qi.BOUND_MODELS]


@pytest.mark.parametrize("qp", qi.WRAP_QPS)
def test_dc_wrap_occurs_in_the_oracle(qp):
    for n in qi.SIZES:
        blocks = qi.dc_wrap_blocks(qp, n)
        count = sum(bool(qi.dc_wrapped(b, po.quantize(b, qp))) for b in blocks)
        assert count >= 1, (qp, n)


@pytest.mark.parametrize("n", qi.SIZES)
def test_the_level_limit_in_the_oracle(n):
    """A coefficient at the tables' last entry quantises (dq_table[1023] consulted, nothing beyond); one step more and
    the oracle raises where the reference panics."""
    qps = qi.limit_qps(n)
    assert (qps[0] + 1) % 6 != (qps[1] + 1) % 6
    for qp in qps:
        for seed in range(4):
            ref = po.quantize(qi.limit_block(qp, n, seed, over=False), qp)
            assert po.last_table_index() == 1023, (n, qp, seed)
            assert qi.trellis_levels(ref).max() in (1021, 1022), (n, qp, seed)
            with pytest.raises(OverflowError):
                po.quantize(qi.limit_block(qp, n, seed, over=True), qp)
        po.quantize(qi.harmless_block(qp, n), qp)
        # between the two, at quotient 2043, the reference's answer depends on the states its search visits: alone at
        # the walk's first position (state 0 only) it quantises, reached in a state with delta 1 it panics, at the DC
        # position it quantises in every state
        for name, b, oracle_ok, device_ok in qi.early_blocks(qp, n):
            assert int(np.abs(b.astype(np.int32)).max()) == qi.coef_below(qi.OVER_QUOTIENT - 1, qp, n)
            if oracle_ok:
                ref = po.quantize(b, qp)
                assert po.last_table_index() == 1023, (n, qp, name)
                assert qi.trellis_levels(ref).max() in (1021, 1022), (n, qp, name)
            else:
                with pytest.raises(OverflowError):
                    po.quantize(b, qp)
            assert oracle_ok or not device_ok
        dc = qi.early_blocks(qp, n)[2][1]
        assert np.count_nonzero(po.quantize(dc, qp)) > 1      # the walk does not arrive at the DC position in state 0 alone
