"""The split cut's floors (wrenc_amd/csrc/dev_search.h, split_floor_cut; const_block.cpp, fill_split_floors) on the CPU.

The rule: before a child of a split is searched, the partial sum of the children searched so far plus the floor of every
child still to come, added one by one in z-order in f32, is compared with the unsplit cost; strictly greater means the
split has lost.  Held here in NumPy f32 against the exhaustive search on random trees whose children cost at least
their floors -- some exactly their floors, some with partial sums equal to the unsplit cost -- and two wrong rules (a cut
on >=, a sum of floors formed on its own and added once) are shown to take another decision somewhere.

The floors: recomputed from the tables of the host's own config with the host's formula (split_floors.floors_of_config)
and held against the oracle alone -- on traced encodes every candidate of every leaf and every node's cost is >= its
floor, at QP 18 .. 51 in every (qp + 1) % 6 class and under the rate models at the edge of what the library accepts, on
smooth, textured, noise and flat content; and the floors decide cuts the plain partial sum does not."""
import numpy as np
import pytest

import quant_inputs as qi
import split_floors as sf
from content import content

F = np.float32


# ---- the rule on random trees ------------------------------------------------------------------------------------
# A node is (unsplit cost, children): four nodes, or at level 2 five leaf costs (four 4x4 luma leaves, the chroma leaf).
def _full(node, level=0):
    u, kids = node
    s, parts = F(0.0), []
    for k in kids:
        c, p = (k, "L") if level == 2 else _full(k, level + 1)
        s = F(s + c)
        parts.append(p)
    return (u, "U") if s > u else (s, tuple(parts))


def _cut(node, fl, level=0, fired=None, strict=True, presum=False):
    """The device's rule; strict=False cuts on >=, presum=True adds one precomputed sum of the floors to come."""
    u, kids = node
    kf = fl.children(level)
    s, parts = F(0.0), []
    for i, k in enumerate(kids):
        if presum:
            rest = F(0.0)
            for f in kf[i:]:
                rest = F(rest + f)
            b = F(s + rest)
        else:
            b = s
            for f in kf[i:]:
                b = F(b + f)
        if (b > u) if strict else (b >= u):
            if fired is not None:
                fired["floor" if not s > u else "plain"] += 1
                fired["whole"] += int(i == 0)
            return u, "U"
        c, p = (k, "L") if level == 2 else _cut(k, fl, level + 1, fired, strict, presum)
        s = F(s + c)
        parts.append(p)
    return (u, "U") if s > u else (s, tuple(parts))


def _random_tree(rng, fl, level=0):
    if level == 2:
        kf = fl.children(2)
        kind = rng.integers(0, 4)
        if kind == 0:       # every leaf exactly at its floor
            kids = list(kf)
        elif kind == 1:     # some at the floor, large and small together: sums that round
            kids = [f if rng.integers(0, 2) else F(f + F(rng.choice([0.37, 3.0, 1.0e8, 16777216.0]))) for f in kf]
        else:
            kids = [F(f + F(rng.random() * rng.choice([1.0, 300.0, 5.0e4]))) for f in kf]
    else:
        kids = [_random_tree(rng, fl, level + 1) for _ in range(4)]
    s = _full((F(np.inf), kids), level)[0]      # what the split costs
    pick = rng.integers(0, 8)
    if pick == 0:
        u = s                                   # a tie: the split wins
    elif pick == 1:
        u = np.nextafter(s, F(np.inf), dtype=F)
    elif pick == 2:
        u = np.nextafter(s, F(0.0), dtype=F)
    elif pick == 3:
        u = fl.single                           # the unsplit candidate exactly at its floor
    else:
        u = F(s * F(rng.choice([0.2, 0.6, 0.9, 1.1, 1.6, 4.0])))
    return (max(F(u), fl.single), kids)


def _random_floors(rng):
    scale = F(rng.choice([0.0, 1.0, 235.2, 1.0e4, 3.0e6]))
    return sf.Floors(F(scale * F(rng.random())), F(scale * F(rng.random())), F(scale * F(2.0 * rng.random())), 3)


def test_floor_rule_decides_like_the_full_sum():
    rng = np.random.default_rng(7)
    fired = {"floor": 0, "plain": 0, "whole": 0}
    ties = at_floor = 0
    wrong = {"ge": 0, "presum": 0}
    for _ in range(600):
        fl = _random_floors(rng)
        tree = _random_tree(rng, fl)
        want = _full(tree)
        got = _cut(tree, fl, fired=fired)
        assert got[1] == want[1], "another partition"
        assert F(got[0]).tobytes() == F(want[0]).tobytes(), "another cost"
        ties += int(_full((F(np.inf), tree[1]))[0] == tree[0])
        at_floor += int(tree[0] == fl.single)
        wrong["ge"] += int(_cut(tree, fl, strict=False) != want)
        wrong["presum"] += int(_cut(tree, fl, presum=True) != want)
    assert fired["floor"] > 0 and fired["plain"] > 0 and fired["whole"] > 0, fired
    assert ties > 0 and at_floor > 0
    assert wrong["ge"] > 0, "a cut on >= took no other decision on these trees: they hold no tie"
    assert wrong["presum"] > 0, "a precomputed sum of floors took no other decision: no sum on these trees rounds"
    print("cuts %s, ties %d, wrong decisions of the two wrong rules %s" % (fired, ties, wrong))


def test_a_tie_is_a_split_and_the_floors_are_added_in_order():
    """Children exactly at their floors and a partial sum equal to the unsplit cost: the split wins and is searched to
    its end; a cut on >= loses it.  Floors that round away one by one but not as a sum: ((2^24 + 1) + 1) + 1 = 2^24 in
    f32, 2^24 + (1 + 1 + 1) is not, so a precomputed sum cuts a split that ties."""
    fl = sf.Floors(1.0, 2.0, 1.0, 3)
    node8 = (F(6.0), [F(1.0), F(1.0), F(1.0), F(1.0), F(2.0)])
    assert _full(node8, 2) == _cut(node8, fl, 2) == (F(6.0), ("L",) * 5)
    assert _cut(node8, fl, 2, strict=False) == (F(6.0), "U")
    big = F(16777216.0)
    node8 = (big, [big, F(1.0), F(1.0), F(1.0), F(1.0)])
    fl = sf.Floors(1.0, 1.0, 1.0, 3)
    assert _full(node8, 2) == _cut(node8, fl, 2) == (big, ("L",) * 5)
    assert _cut(node8, fl, 2, presum=True) == (big, "U")
    # one step over: the floors decide before the second leaf, the partial sum alone does not
    fired = {"floor": 0, "plain": 0, "whole": 0}
    fl = sf.Floors(2.0, 3.0, 4.0, 3)
    over = (F(11.0), [F(2.5), F(2.0), F(2.0), F(2.0), F(3.0)])
    assert _full(over, 2) == _cut(over, fl, 2, fired) == (F(11.0), "U")
    assert fired == {"floor": 1, "plain": 0, "whole": 0}


# ---- the floors against the oracle -------------------------------------------------------------------------------
def _frame(kind, w, h, i):
    from wrenc_amd import synth
    if kind == "smooth":
        return synth.synth_frame(w, h, i)
    if kind == "textured":
        return synth.synth_textured_frame(w, h, i)
    return content(kind, w, h, 40 + i)


def _check_floors(qp, extra, kinds, depth=3, w=64, h=64):
    """Traced oracle encodes at one rate model: every candidate and every node against the floors; returns the replay's
    counts summed over the pictures (floors rule) and the same under the plain rule."""
    from oracle import pyoracle as po
    from wrenc_amd import gpu
    cfg = gpu.default_config(w, h, qp, depth, extra_params=extra)
    fl = sf.floors_of_config(cfg)
    assert fl.leaf4 >= 0 and fl.leafc4 >= 0 and fl.single >= 0
    with_floors, plain = {}, {}
    po.set_extra_params(extra)
    try:
        for kind in kinds:
            rec, rows = sf.ordered_trace(*_frame(kind, w, h, 1), qp, depth)
            cost, low = sf.leaf_costs(rows)
            for (x, y, lg, tree), v in low.items():
                f = {sf.SINGLE: fl.single, sf.DUAL_LUMA: fl.leaf4, sf.DUAL_CHROMA: fl.leafc4}[tree]
                assert v >= f, (qp, extra, kind, (x, y, lg, tree), float(v), float(f))
            i = 0
            for cy in range(0, h, 32):
                for cx in range(0, w, 32):
                    full = {}
                    want = sf.replay(cost, cx, cy, 0, fl, stats=full, exhaustive=True)
                    assert F(want).tobytes() == F(rec["ctu_cost"][i]).tobytes(), (qp, extra, kind, cx, cy)
                    for level, v in full["nodes"]:
                        assert v >= fl.node[level], (qp, extra, kind, level, float(v), float(fl.node[level]))
                    for stats, rule in ((with_floors, fl), (plain, sf.zero_floors(depth))):
                        got = sf.replay(cost, cx, cy, 0, rule, stats=stats)
                        assert F(got).tobytes() == F(want).tobytes(), (qp, extra, kind, cx, cy)
                    i += 1
    finally:
        po.set_extra_params(None)
    return fl, with_floors, plain


KINDS = ("smooth", "textured", "noise", "flat")


@pytest.mark.parametrize("qp", [18, 22, 27, 32, 37, 41, 46, 51])
def test_costs_stay_above_the_floors(built, qp):
    """QP 18 .. 51; 18, 22, 27, 32, 37, 41 are the six (qp + 1) % 6 classes 1, 5, 4, 3, 2, 0."""
    fl, with_floors, plain = _check_floors(qp, None, KINDS)
    assert fl.leaf4 > 0 and fl.leafc4 > 0 and fl.single > 0, "the default tables prove positive floors"
    assert plain.get("floor_cuts", 0) == 0
    print("qp %d floors %.1f / %.1f / %.1f nodes %s: %s, plain %s" % (qp, fl.leaf4, fl.leafc4, fl.single,
                                                                     [float(v) for v in fl.node], with_floors, plain))


def test_qp_classes_are_all_there():
    assert {(q + 1) % 6 for q in (18, 22, 27, 32, 37, 41, 46, 51)} == set(range(6))


@pytest.mark.parametrize("qp,extra", qi.BOUND_MODELS)
def test_costs_stay_above_the_floors_at_the_edge_models(built, qp, extra):
    """The QPs and rate models of tests/test_gpu_quant_bounds.py."""
    _check_floors(qp, extra, ("textured", "noise", "flat"), w=32, h=32)


@pytest.mark.parametrize("depth", [1, 2])
def test_costs_stay_above_the_floors_at_lower_depths(built, depth):
    _check_floors(32, None, ("smooth", "textured"), depth=depth)


def test_the_floors_cut_what_the_partial_sum_does_not(built):
    """Smooth content at QP 32, the benchmark's: cuts that only the floors decide, fewer 4x4 leaves and chroma leaves
    searched than under the plain rule, and never more of anything."""
    fl, with_floors, plain = _check_floors(32, None, ("smooth",), w=128, h=64)
    assert with_floors.get("floor_cuts", 0) > 0
    assert with_floors["leaf4"] < plain["leaf4"]
    for k in ("leaf4", "leafc4", "node8", "node16"):
        assert with_floors.get(k, 0) <= plain.get(k, 0), k
    print("with floors %s\nplain %s" % (with_floors, plain))


def test_tables_that_prove_nothing_give_zero_floors(built):
    """A negative lv_table entry, a negative header-bit minimum or a negative lambda: every floor is 0.0, the plain rule."""
    from wrenc_amd import gpu
    for spoil in ("lv", "hb", "lambda"):
        cfg = gpu.default_config(64, 64, 32, 3)
        if spoil == "lv":
            cfg.lv_table[900] = -1
        elif spoil == "hb":
            cfg.header_bits_chroma[2] = -5
        else:
            cfg.lambda_rd_chroma = -1.0
        fl = sf.floors_of_config(cfg)
        assert fl.leaf4 == 0 and fl.leafc4 == 0 and fl.single == 0 and all(v == 0 for v in fl.node), spoil
