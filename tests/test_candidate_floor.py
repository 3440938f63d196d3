"""The candidate cut of the 4x4 luma leaf search (wrenc_amd/csrc/dev_search.h, kCandidateCut; const_block.cpp,
fill_split_floors) on the CPU, from the oracle alone (tests/candidate_floors.py holds the floors and the replay).

  * Every traced full candidate of every 4x4 DUAL_TREE_LUMA leaf costs at least the floor of its mode class, in f32, with
    no violation allowed: smooth, textured, noise and flat content at QP 18 .. 51 and under the rate models at the edge of
    what the library accepts.
  * The leaf search replayed under the rule returns the exhaustive leaf's mode and cost, bit for bit, ...
  * ... and put into the split cut's replay (split_floors.replay) it reaches the oracle's CTU cost.
  * Two wrong rules -- a cut on floor + eps >= best, the floor of another class -- take another decision somewhere."""
import numpy as np
import pytest

import candidate_floors as cf
import quant_inputs as qi
import split_floors as sf
from content import content

F = np.float32
KINDS = ("smooth", "textured", "noise", "flat")


def _frame(kind, w, h, i):
    from wrenc_amd import synth
    if kind == "smooth":
        return synth.synth_frame(w, h, i)
    if kind == "textured":
        return synth.synth_textured_frame(w, h, i)
    return content(kind, w, h, 40 + i)


def _check(qp, extra, kinds, w=64, h=64, depth=3):
    """Traced oracle encodes at one rate model; returns what fired, summed over the pictures."""
    from oracle import pyoracle as po
    from wrenc_amd import gpu
    cfg = gpu.default_config(w, h, qp, depth, extra_params=extra)
    fl = cf.floors_of_config(cfg)
    split_fl = sf.floors_of_config(cfg)
    assert fl.proven and (fl.cls >= 0).all()
    fired = {"sad": 0, "packB": 0, None: 0}
    po.set_extra_params(extra)
    try:
        for kind in kinds:
            rec, rows = sf.ordered_trace(*_frame(kind, w, h, 1), qp, depth)
            cost, _ = sf.leaf_costs(rows)
            leaves = cf.leaves_of(rec, rows)
            assert len(leaves) == (w // 4) * (h // 4)
            cut_cost = dict(cost)
            for (x, y), leaf in leaves.items():
                for m, v in leaf.cands:
                    f = fl.cls[cf.mpm_class_of(leaf.mpl, m)]
                    assert v >= f, (qp, extra, kind, (x, y), m, float(v), float(f))
                    if m > cf.DC:
                        assert f >= fl.ang or (m == leaf.mpl[0] and f == fl.cls[1]), (qp, extra, kind, (x, y), m)
                mode, best, what = cf.replay_leaf(leaf, fl)
                want = leaf.exhaustive()
                assert mode == want[0] and F(best).tobytes() == F(want[1]).tobytes(), (qp, extra, kind, (x, y), what)
                assert F(best).tobytes() == F(cost[(x, y, 2, sf.DUAL_LUMA)]).tobytes()
                fired[what] += 1
                cut_cost[(x, y, 2, sf.DUAL_LUMA)] = best
            i = 0
            for cy in range(0, h, 32):
                for cx in range(0, w, 32):
                    got = sf.replay(cut_cost, cx, cy, 0, split_fl)
                    assert F(got).tobytes() == F(rec["ctu_cost"][i]).tobytes(), (qp, extra, kind, cx, cy)
                    i += 1
    finally:
        po.set_extra_params(None)
    return fl, fired


@pytest.mark.parametrize("qp", [18, 22, 27, 32, 37, 41, 46, 51])
def test_candidates_stay_above_their_floors(built, qp):
    """QP 18 .. 51; 18, 22, 27, 32, 37, 41 are the six (qp + 1) % 6 classes."""
    fl, fired = _check(qp, None, KINDS)
    assert fl.cls[0] > 0 and fl.ang > fl.cls[0], "the default tables: planar is the cheapest class"
    print("qp %d floors planar %.1f mpm0 %.1f angular %.1f: %s" % (qp, fl.cls[0], fl.cls[1], fl.ang, fired))


@pytest.mark.parametrize("qp,extra", [(32, "quant_lambda_mul_trellis=86"), (37, "quant_lambda_mul_trellis=44")])
def test_candidates_stay_above_their_floors_at_the_edge_models(built, qp, extra):
    assert (qp, extra) in qi.BOUND_MODELS
    _check(qp, extra, KINDS)


def test_both_rules_fire_on_smooth_content(built):
    """160x128 at QP 32 and 37: leaves that skip the SAD search and pack B, and leaves that skip pack B alone."""
    for qp in (32, 37):
        _, fired = _check(qp, None, ("smooth",), w=160, h=128)
        assert fired["sad"] > 0 and fired["packB"] > 0 and fired[None] > 0, (qp, fired)


def test_noise_is_never_cut(built):
    _, fired = _check(32, None, ("noise",))
    assert fired["sad"] == 0 and fired["packB"] == 0


# ---- the rule itself, on leaves made by hand -------------------------------------------------------------------------
def _leaf(fl, mpl, best_a, cm, costs_b):
    """A leaf whose pack A costs [best_a, best_a + 9] and whose pack B costs costs_b (one per candidate that exists)."""
    leaf = cf.Leaf(8, 8, mpl)
    modes = [cm] + ([cm - 1] if cm >= 3 else []) + ([cm + 1] if cm + 1 <= 66 else [])
    leaf.cands = [(cf.PLANAR, F(best_a)), (cf.DC, F(best_a + F(9.0)))] + [(m, F(v)) for m, v in zip(modes, costs_b)]
    return leaf


def _real_floors():
    from wrenc_amd import gpu
    return cf.floors_of_config(gpu.default_config(64, 64, 32, 3))


def test_a_candidate_at_its_floor_is_cut_only_on_a_tie(built):
    fl = _real_floors()
    mpl = cf.mpm_list(cf.PLANAR, cf.PLANAR)         # (DC, 50, 18, 46, 54)
    cm = 30
    modes = (30, 29, 31)
    f = [fl.cls[cf.mpm_class_of(mpl, m)] for m in modes]
    j = int(np.argmin(f))
    up = np.nextafter(f[j], F(np.inf), dtype=F)
    big = F(1.0e6)
    # best one step above the smallest floor of pack B, that candidate exactly at its floor: it wins, and only an
    # exhaustive pack B finds it
    leaf = _leaf(fl, mpl, up, cm, [f[j] if i == j else big for i in range(3)])
    assert cf.replay_leaf(leaf, fl) == (modes[j], f[j], None) == leaf.exhaustive() + (None,)
    wrong = cf.replay_leaf(leaf, fl, eps=np.spacing(f[j]))
    assert wrong[0] == cf.PLANAR and wrong[2] == "packB", "a cut on floor + eps >= best loses the candidate at its floor"
    # best equal to the smallest floor of pack B and every candidate at its floor: a tie keeps pack A's winner, cut or not
    leaf = _leaf(fl, mpl, min(f), cm, f)
    assert cf.replay_leaf(leaf, fl)[:2] == leaf.exhaustive() == (cf.PLANAR, min(f))
    assert cf.replay_leaf(leaf, fl)[2] == "packB"
    # best at the smallest angular floor: nothing angular can be strictly cheaper, the SAD search is skipped
    leaf = _leaf(fl, mpl, fl.ang, cm, [big, big, big])
    assert cf.replay_leaf(leaf, fl)[2] == "sad"
    leaf = _leaf(fl, mpl, np.nextafter(fl.ang, F(np.inf), dtype=F), cm, [big, big, big])
    assert cf.replay_leaf(leaf, fl)[2] != "sad"


def test_the_floor_of_another_class_decides_otherwise(built):
    """cm = the first MPM candidate of an angular neighbourhood (class 1); classified as if the list were the default
    one it is a remainder mode with a larger floor, and a cost between the two floors is cut although it wins."""
    fl = _real_floors()
    mpl = cf.mpm_list(34, 34)
    assert mpl[0] == 34
    default = cf.mpm_list(cf.PLANAR, cf.PLANAR)
    right = fl.cls[1]
    other = min(fl.cls[cf.mpm_class_of(default, m)] for m in (34, 33, 35))
    assert other > right, "QP 32: the remainder modes 33 .. 35 of the default list are dearer than mpm_idx 0"
    best = F(other)
    win = F((right + other) / 2)
    big = F(1.0e6)
    leaf = _leaf(fl, mpl, best, 34, [win, big, big])
    assert cf.replay_leaf(leaf, fl) == (34, win, None) == leaf.exhaustive() + (None,)
    wrong = cf.replay_leaf(leaf, fl, cls_of=lambda l, m: cf.mpm_class_of(default, m))
    assert wrong[0] == cf.PLANAR and wrong[2] is not None
    # the first rule counts mpm_idx 0 where it is angular: with this list best = the remainder minimum does not skip the SAD search
    # unless mpm_idx 0 is as dear
    assert (cf.replay_leaf(_leaf(fl, mpl, fl.ang, 34, [big, big, big]), fl)[2] == "sad") == (fl.cls[1] >= fl.ang)


def test_random_leaves_decide_like_the_exhaustive_search(built):
    fl = _real_floors()
    rng = np.random.default_rng(11)
    fired = {"sad": 0, "packB": 0, None: 0}
    wrong = 0
    for _ in range(3000):
        left, above = (int(rng.choice([0, 1, 2, 18, 34, 35, 50, 66])) for _ in range(2))
        mpl = cf.mpm_list(left, above)
        cm = int(rng.choice([2, 3, 18, 34, 50, 65, 66, int(rng.integers(2, 67))]))
        modes = [cm] + ([cm - 1] if cm >= 3 else []) + ([cm + 1] if cm + 1 <= 66 else [])
        fb = [fl.cls[cf.mpm_class_of(mpl, m)] for m in modes]
        # costs at or above the floors, often exactly at them or one step away
        def at(f):
            k = rng.integers(0, 4)
            return f if k == 0 else np.nextafter(f, F(np.inf), dtype=F) if k == 1 else F(f + F(rng.random() * 300.0))
        leaf = cf.Leaf(4, 4, mpl)
        a0 = (at(fl.cls[0]), min(fb), np.nextafter(min(fb), F(np.inf), dtype=F), F(fl.cls[0] + F(rng.random() * 600.0)))[rng.integers(0, 4)]
        leaf.cands = [(cf.PLANAR, a0), (cf.DC, at(fl.cls[cf.mpm_class_of(mpl, cf.DC)]))] + [(m, at(f)) for m, f in zip(modes, fb)]
        mode, best, what = cf.replay_leaf(leaf, fl)
        assert (mode, F(best).tobytes()) == (leaf.exhaustive()[0], F(leaf.exhaustive()[1]).tobytes())
        fired[what] += 1
        wrong += int(cf.replay_leaf(leaf, fl, eps=F(0.01))[:2] != leaf.exhaustive())
    assert min(fired.values()) > 0, fired
    assert wrong > 0, "a cut on floor + eps >= best took no other decision on these leaves"


def test_tables_that_prove_nothing_switch_the_rule_off(built):
    from wrenc_amd import gpu
    for spoil in ("lv", "hb", "lambda"):
        cfg = gpu.default_config(64, 64, 32, 3)
        if spoil == "lv":
            cfg.lv_table[900] = -1
        elif spoil == "hb":
            cfg.header_bits_luma[1][0][40] = -5
        else:
            cfg.lambda_rd = -1.0
        fl = cf.floors_of_config(cfg)
        assert not fl.proven and np.isneginf(fl.cls).all() and np.isneginf(fl.ang), spoil
        leaf = _leaf(fl, cf.mpm_list(0, 0), 1.0, 30, [0.5, 2.0, 2.0])
        assert cf.replay_leaf(leaf, fl) == (30, F(0.5), None)
