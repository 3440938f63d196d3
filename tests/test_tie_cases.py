"""The pictures of tie_cases.py can tell the two sides of every tie rule apart (CPU, the oracle alone).

test_gpu_ties.py holds the device to the oracle on these pictures; that says which side of a tie the device takes only
while taking the other side changes the oracle's record.  This file fails when the list loses that power.

Measured with this list (27 cases; whoever changes the list measures again, tie_cases.changed / decisive):

    records changed of 27 / log2 sizes at which the rule decides (2 = 4x4, for R5 and R6 the 4x4 chroma leaf of a split 8x8)

    rule   ZERO             ZERO_CHROMA      default model
    R1      7   2            7   2 3          5   2 3
    R2      7   2 4          6   2 3 4        5   2 3 4
    R3      3   2            0                0
    R4     27   2 3 4 5      0                0
    R5     15   2 3 4 5     10   2 3 4 5      9   2 3 4 5
    R6     27   2 3 4 5     27   2 3 4 5      0
    R7      9   3 4 5        0                0

    R7 by depth under ZERO: the 32x32 node alone at depth 1 (flat) and depth 2 (flat, stripes0); the 16x16 node in
    stripes0 at depth 3, whose 32x32 decisions do not tie; the 8x8 node in stripes0 and extremes at depth 3.

The default model is the control: R4, R6 and R7 change no record of the list under it, which is the gap that the zero
lambda closes.  R1, R2, R3 and R5 compare SADs, which carry no rate term under any model."""
import numpy as np
import pytest

import tie_cases as tc


def _measure(extra, rule):
    hit = [c for c in tc.CASES if tc.changed(c, extra, rule)]
    sizes = set()
    for c in hit:
        sizes |= tc.decisive(c, extra, rule)
    return hit, sizes


def test_the_list_is_small_and_has_every_kind_of_ctu():
    assert len(tc.CASES) == len(set(tc.CASES)) <= 30
    for (w, h, depth), cases in tc.groups().items():
        assert w >= 64 and h >= 64 and w % 32 == 0 and h % 32 == 0     # corner, top-edge, left-edge, interior CTU
        assert 0 <= depth <= 3 and len(cases) <= 10
    assert {g[2] for g in tc.groups()} == {0, 1, 2, 3}
    assert any(g[0] >= 96 for g in tc.groups())                         # two CTUs on one anti-diagonal


@pytest.mark.parametrize("rule", tc.RULES)
def test_every_rule_changes_a_record_under_zero(rule):
    hit, sizes = _measure(tc.ZERO, rule)
    assert hit and sizes, rule
    # the flipped oracle is still an encoder: its records are valid, only different (record() checks the final pass)
    want = {"R4": {2, 3, 4, 5},    # leaf sizes 4, 8, 16, 32
            "R6": {2, 3, 4, 5},    # the 4x4 chroma leaf of a split 8x8; single-tree sizes 8, 16, 32
            "R5": {2, 3, 4, 5},    # likewise
            "R7": {3, 4, 5}}.get(rule, set())
    assert want <= sizes, (rule, sizes)


def test_r4_and_r6_decide_in_every_case_under_zero():
    """The first CTU of a picture has no neighbours: planar, DC and mode 2 predict the same block, DM and CCLM too."""
    for rule in ("R4", "R6"):
        assert len(_measure(tc.ZERO, rule)[0]) == len(tc.CASES), rule


def test_r7_decides_at_each_node_size_pinned_by_the_depth():
    by = lambda kind, w, depth: [c for c in tc.CASES if (c[0], c[1], c[5]) == (kind, w, depth)][0]
    # depth 1: only the 32x32 decision exists
    assert tc.decisive(by("flat", 64, 1), tc.ZERO, "R7") == {5}
    # depth 2, stripes0: its 32x32 decision ties, and the flipped oracle stops there
    assert tc.decisive(by("stripes0", 64, 2), tc.ZERO, "R7") == {5}
    # depth 3, stripes0: CTUs whose 32x32 decision does not tie while 16x16 and 8x8 decisions below it do
    assert {3, 4} <= tc.decisive(by("stripes0", 64, 3), tc.ZERO, "R7")
    c = by("stripes0", 64, 3)
    a, b = tc.record(c, tc.ZERO), tc.record(c, tc.ZERO, "R7")
    at16 = (b["cu_log2_size"] == 4) & (a["cu_log2_size"] < 4)
    assert at16.any() and not (b["cu_log2_size"][at16] == 5).any()
    # depth 3, extremes: 8x8 against 4x4
    assert tc.decisive(by("extremes", 64, 3), tc.ZERO, "R7") == {3}


def test_r6_decides_under_zero_chroma():
    hit, sizes = _measure(tc.ZERO_CHROMA, "R6")
    assert len(hit) == len(tc.CASES) and sizes == {2, 3, 4, 5}


@pytest.mark.parametrize("rule", ["R4", "R6", "R7"])
def test_control_the_default_model_leaves_the_rule_undecided(rule):
    assert _measure(tc.DEFAULT, rule)[0] == []


def test_zero_changes_every_record():
    """What test_gpu_ties.py asserts of the device's records, here of the oracle's: the string reaches the search.
    (ZERO_CHROMA leaves some records as they are, the flat pictures' among them, although R6 decides in them.)"""
    for c in tc.CASES:
        plain, rec = tc.record(c, tc.DEFAULT), tc.record(c, tc.ZERO)
        assert any(not np.array_equal(rec[k], plain[k]) for k in tc.KEYS), tc.case_id(c)
        assert np.array_equal(rec["ctu_cost"], np.trunc(rec["ctu_cost"])), tc.case_id(c)     # a cost is (float)ssd
    changed = [c for c in tc.CASES if any(not np.array_equal(tc.record(c, tc.ZERO_CHROMA)[k], tc.record(c, tc.DEFAULT)[k])
                                          for k in tc.KEYS)]
    assert 2 * len(changed) > len(tc.CASES)       # (17 of 27: where DM won before, it still wins the tie)


def test_the_switches_are_off_by_default_and_after_record():
    from oracle import pyoracle as po
    c = tc.CASES[0]
    tc.record(c, tc.ZERO, "R4")
    y, cb, cr = tc.frame(c)
    again = po.encode_picture(y, cb, cr, c[4], c[5])
    plain = tc.record(c, tc.DEFAULT)
    assert all(np.array_equal(again[k], plain[k]) for k in tc.KEYS)
