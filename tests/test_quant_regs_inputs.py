"""The blocks of quant_regs_inputs.py reach the cases they are built for -- read off the reference's formulas and the
oracle (its literal search, and its model of the head test), on the CPU: test_gpu_quant_regs.py then cannot pass without
exercising them."""
import numpy as np
import pytest

import quant_inputs as qi
import quant_regs_inputs as ri


@pytest.fixture(scope="module")
def po(built):
    from oracle import pyoracle
    return pyoracle


def _model(po, b):
    """The oracle model's counters for one block (its levels equal the literal search's)."""
    po.dq_sc_stats_enable(True)
    try:
        out = po.quantize_sc(b, ri.QP)
        _, st = po.dq_sc_stats_read()
    finally:
        po.dq_sc_stats_enable(False)
    assert np.array_equal(out, po.quantize(b, ri.QP))
    return st[b.shape[0].bit_length() - 1]


def _first_test(po, b):
    """What the head test at the end of the planned walk says: ("pass", start), ("fail", 0) or ("none", 0)."""
    st = _model(po, b)
    if st["head_fail"]:        # a pass ends the model's tests: a failure counted means the first one failed
        return "fail", 0
    if st["head_tests"]:
        return "pass", 16 * st["head_sb_skipped"]
    return "none", 0


@pytest.mark.parametrize("n", qi.SIZES)
def test_both_parities_at_every_position(n):
    seen = set()
    for flip in (0, 1):
        b = ri.parity_block(n, flip)
        for p, qd in enumerate(ri.quotients(b)):
            assert ri.at(b, p) != 0 and qd >= 2, (n, flip, p)
            seen.add((p, qd & 1))
    assert seen == {(p, e) for p in range(n * n) for e in (0, 1)}     # (p = n * n - 1: the DC position)


@pytest.mark.parametrize("n", qi.SIZES)
def test_the_table_edge(po, n):
    N = n * n
    for k, a3 in enumerate(ri.EDGE):
        b = ri.edge_one_block(n, a3, k)
        top = [qd // 2 + 3 for qd in ri.quotients(b)]
        assert sorted(top)[-2:] == [sorted(top)[-2], a3] and sorted(top)[-2] < 253, (n, a3)     # one lane, the others far below
        ref = po.quantize(b, ri.QP)
        assert po.last_table_index() in (a3 - 1, a3), (n, a3, po.last_table_index())            # the oracle read that entry
        assert qi.trellis_levels(ref).max() < 1021
    reached, parities = set(), set()
    for seed in range(2):
        b = ri.edge_all_block(n, seed)
        qds = ri.quotients(b)
        assert all(ri.EDGE[0] <= qd // 2 + 3 <= ri.EDGE[-1] for qd in qds), (n, seed)           # all lanes
        reached |= {qd // 2 + 3 for qd in qds}
        parities |= {(qd // 2 + 3, qd & 1) for qd in qds}
        ref = po.quantize(b, ri.QP)
        assert 256 <= po.last_table_index() <= 258, (n, seed)
        assert qi.trellis_levels(ref).max() < 1021
    assert reached == set(ri.EDGE), (n, reached)
    if N >= 64:
        assert parities == {(a3, e) for a3 in ri.EDGE for e in (0, 1)}, n


@pytest.mark.parametrize("n", (8, 16, 32))
def test_heads_pass_and_fail(po, n):
    starts = {0}
    for sbs, amp, seed in ri.HEADS[n]["pass"]:
        assert _first_test(po, ri.head_block(n, sbs, amp, seed)) == ("pass", 16 * sbs), (n, sbs)
        starts.add(16 * sbs)
    for sbs, amp, seed in ri.HEADS[n]["fail"]:
        assert _first_test(po, ri.head_block(n, sbs, amp, seed)) == ("fail", 0), (n, sbs)
    if n == 8:      # trace_rows64: 4, 4, 2 and 1 positions per lane
        assert starts == {0, 16, 32, 48}
    if n < 32:      # the sizes quantize_pk takes
        assert ri.HEADS[n]["fail"]


@pytest.mark.parametrize("log2n,nc", qi.PACKS)
def test_packs_hold_both_orders(po, log2n, nc):
    """Chains whose head test passes, chains whose test fails, and -- from two candidates up -- a pack with both; a pack with
    all-zero chroma beside non-zero luma; at most 64 packs."""
    luma, chroma = ri.pack_plan(log2n, nc)
    assert len(luma) // nc <= 64
    kinds = [_first_test(po, b)[0] for _, b in luma]
    assert "pass" in kinds and "fail" in kinds
    per_pack = [set(kinds[p * nc:(p + 1) * nc]) for p in range(len(luma) // nc)]
    if nc > 1:
        assert any({"pass", "fail"} <= s for s in per_pack)
    if log2n == 4:  # 8x8 chroma chains have heads too: both outcomes, and both in one pack
        ckinds = [_first_test(po, b)[0] for _, b in chroma]
        assert "pass" in ckinds and "fail" in ckinds
        assert any({"pass", "fail"} <= set(ckinds[p * 2 * nc:(p + 1) * 2 * nc]) for p in range(len(luma) // nc))
    zero_beside = [p for p in range(len(luma) // nc)
                   if not any(b.any() for _, b in chroma[p * 2 * nc:(p + 1) * 2 * nc]) and all(po.quantize(b, ri.QP).any() for _, b in luma[p * nc:(p + 1) * nc])]
    assert zero_beside


@pytest.mark.parametrize("n", (4, 8, 16))
def test_zero_kept_in_the_trailing_run_at_a_sub_block_start(po, n):
    """In chains that are walked from end to end (no head skipped: the largest coefficient of quotient 1 ends the proven
    region at 4x4 and 8x8; at 16x16, where it does not, the heads that fail their test), the first position of a sub-block
    (p & 15 == 15) is a zero of state 0 inside the trailing run -- quotient below 2, at or before the first significant
    position -- in some sub-blocks and not in others; at 4x4 and 8x8 so is the DC position of a walked chain.  (At 32x32 no
    block of these recipes is walked through such a position: quant_regs_inputs.HEADS.)"""
    N = n * n
    blocks = [ri.adj_block(n, True), ri.adj_block(n, False)] if n < 16 else []
    blocks += [ri.head_block(n, *h) for h in ri.HEADS[n]["fail"]]
    flags = set()
    for b in blocks:
        st = _model(po, b)
        assert st["whole_zero"] == 0 and (st["head_sb_skipped"] == 0 or st["head_fail"]), n
        qds = ri.quotients(b)
        istar = min([p for p in range(N) if qds[p] >= 2], default=N)
        for p in range(15, N, 16):
            flags.add((p == N - 1, p <= istar and qds[p] < 2))
    if n > 4:
        assert (False, True) in flags and (False, False) in flags
    if n < 16:
        assert (True, True) in flags and (True, False) in flags


@pytest.mark.parametrize("n", qi.SIZES)
def test_single_coefficients(po, n):
    N = n * n
    for first in (True, False):
        for v in (1, -1):
            b = ri.single_block(n, first, v)
            assert ri.at(b, N - 1 if first else 0) == v and np.count_nonzero(b) == 1
            assert not po.quantize(b, ri.QP).any()
        for s in (1, -1):
            ref = po.quantize(ri.single_block(n, first, s * qi.coef_below(2, ri.QP, n)), ri.QP)
            assert np.count_nonzero(ref) == 1 and ref.ravel()[np.flatnonzero(ref)[0]] * s > 0
