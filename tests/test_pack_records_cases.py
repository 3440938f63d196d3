"""What test_gpu_pack_records.py compares, checked on the oracle's records alone (no device)."""
import pack_records_cases as pc


def test_the_records_hold_every_state_and_every_cclm_case():
    """Across the cases every CU size from 8x8 to 32x32 occurs with levels in luma but not in chroma, in chroma but not in
    luma, in both and in neither; and a CCLM chroma mode wins at each of the three sizes with the left neighbour available
    and unavailable."""
    states, cclm = pc.coverage()
    assert [(lg, s) for lg in (3, 4, 5) for s in pc.STATES if (lg, s) not in states] == []
    assert [(lg, left) for lg in (3, 4, 5) for left in (True, False) if (lg, left) not in cclm] == []


def test_the_cases():
    assert len(pc.CASES) == len(pc.KINDS) * 2 * 3 * 3
    assert {"cclm", "ramp", "stripes20", "checker"} <= set(pc.KINDS)
    assert set(pc.SIZES) == {(64, 64), (96, 64)} and pc.QPS == (22, 32, 42) and pc.DEPTHS == (1, 2, 3)
