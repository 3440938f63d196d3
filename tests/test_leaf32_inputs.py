"""The pictures of tests/leaf32_inputs.py hold the cases tests/test_gpu_leaf32.py is there for -- asserted from the CPU
oracle's record and trace alone, so that a case cannot silently vanish when the content or the oracle changes."""
import leaf32_inputs as li


def _ctus(built):
    """(picture kind, CTU index, facts) of every CTU of every picture, at max-split-depth 3"""
    return [(k, i, f) for k, per in zip(li.KINDS, li.leaf_facts(3)) for i, f in enumerate(per)]


def test_pictures_are_3x3_ctus(built):
    for y, cb, cr in li.frames():
        assert y.shape == (96, 96) and cb.shape == cr.shape == (48, 48)


def test_a_leaf_wins_and_loses_in_one_picture(built):
    """(a) a CTU whose 32x32 leaf is the decision at depth 3 and one in the same picture whose split wins"""
    per = li.leaf_facts(3)[li.KINDS.index("smooth_noisy")]
    assert any(f["cu32"] for f in per) and any(not f["cu32"] for f in per)


def test_b_winners_planar_dc_and_a_neighbour_of_cm(built):
    """(b) 32x32 CUs whose luma mode is planar, DC, and cm - 1 or cm + 1 (the winner is not the SAD search's mode); the
    restore path: a winner that a later candidate has overwritten in the tile, and one that is the last candidate"""
    won = [f for _, _, f in _ctus(built) if f["cu32"]]
    assert all(f["luma"] == f["winner"] for f in won)
    assert any(f["winner"] == 0 for f in won)
    assert any(f["winner"] == 1 for f in won)
    assert any(f["winner"] in (f["cm"] - 1, f["cm"] + 1) and f["winner"] > 1 for f in won)
    assert any(f["winner"] == f["cm"] for f in won)
    assert any(f["winner"] != f["order"][-1] for f in won) and any(f["winner"] == f["order"][-1] for f in won)


def test_c_cclm_and_dm_chroma(built):
    """(c) a 32x32 CU whose chroma mode is a CCLM mode and one that keeps DM"""
    won = [f for _, _, f in _ctus(built) if f["cu32"]]
    assert any(f["chroma"] >= li.LT_CCLM for f in won)
    assert any(f["chroma"] == f["luma"] for f in won)


def test_d_directional_winner_at_a_range_end(built):
    """(d) the SAD search ends at mode 2 / mode 66, the neighbour outside 2..66 is not evaluated, and a directional
    candidate wins the leaf -- at either end"""
    ctus = [f for _, _, f in _ctus(built)]
    assert any(f["cm"] == 66 and len(f["order"]) == 4 and f["winner"] >= 65 for f in ctus)
    assert any(f["cm"] == 2 and len(f["order"]) == 4 and f["winner"] in (2, 3) for f in ctus)
    assert any(f["cm"] == 66 and f["cu32"] and f["luma"] == 66 for f in ctus)


def test_every_depth_searches_the_leaf(built):
    """the records of the four depths differ (the leaf is the decision at depth 0 and only sometimes above)"""
    r0, r3 = li.refs(li.QP, 0), li.refs(li.QP, 3)
    assert all((r["cu_log2_size"] == 5).all() for r in r0)
    assert any((r["cu_log2_size"] != 5).any() for r in r3)
