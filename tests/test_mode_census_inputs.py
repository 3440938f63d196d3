"""The planted pictures of tests/mode_census_inputs.py are what tests/test_gpu_mode_census.py needs them to be: conditions on
the inputs, evaluated from the oracle alone (no GPU).  Every failure prints the census table."""
import os
import re

import numpy as np
import pytest

import mode_census_inputs as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4, 8, 16, 32)


@pytest.fixture(scope="module")
def total():
    return mc.total_census()


def _check(ok, total, what):
    assert ok, "%s\n%s" % (what, mc.table(total))


def test_every_luma_mode_wins_at_every_cu_size(total):
    """... at least twice: the save to the leaf's slot and the restore from it, fill_maps, the final pass and the host's
    mode syntax run with every mode number at every size."""
    for row, n in zip(total["wins"], SIZES):
        _check(row.min() >= 2, total, "%dx%d: modes %s win fewer than 2 CUs" % (n, n, np.flatnonzero(row < 2).tolist()))


def test_every_mode_is_a_sad_probe_and_a_full_candidate_at_every_size(total):
    """Kind 0 with every mode 2..66 (the step search lands on both ends of the range, where the probe beyond is refused) and
    kind 1 with every mode 0..66 (cm, cm - 1 and cm + 1 take every value)."""
    for row, n in zip(total["probes"], SIZES):
        _check(row[2:].min() >= 1, total, "%dx%d: modes %s are never a SAD probe" % (n, n, (2 + np.flatnonzero(row[2:] < 1)).tolist()))
        _check(row[:2].max() == 0, total, "%dx%d: planar or DC as a SAD probe" % (n, n))
    for row, n in zip(total["full"], SIZES):
        _check(row.min() >= 1, total, "%dx%d: modes %s are never a full candidate" % (n, n, np.flatnonzero(row < 1).tolist()))


def test_the_derived_chroma_mode_wins_with_every_luma_mode(total):
    """DM with a non-zero Cb or Cr level at the chroma of 32x32, 16x16 and single-tree 8x8 CUs with every mode; at the dual-tree
    chroma of a split 8x8 the issue's floor is 60 modes of 67, and the "dual" pictures reach all 67 (with a non-zero level
    too), which is pinned."""
    for sit in range(3):
        row = total["dm_nz"][sit]
        _check(row.min() >= 1, total, "chroma of %s: DM with a non-zero level never wins with modes %s" % (
            mc.SITUATIONS[sit], np.flatnonzero(row < 1).tolist()))
    assert np.count_nonzero(total["dm"][3]) >= 60
    _check(np.count_nonzero(total["dm"][3]) == mc.N_MODES, total, "dual-tree 8x8: DM never wins with modes %s" % (
        np.flatnonzero(total["dm"][3] < 1).tolist()))
    _check(np.count_nonzero(total["dm_nz"][3]) == mc.N_MODES, total, "dual-tree 8x8: DM with a non-zero level never wins with "
           "modes %s" % (np.flatnonzero(total["dm_nz"][3] < 1).tolist()))


def test_every_cclm_mode_wins_in_every_chroma_situation(total):
    _check(total["cclm"].min() >= 2, total, "a CCLM mode wins fewer than 2 blocks of a situation (rows %s; LT, T, L):\n%s" % (
        mc.SITUATIONS, total["cclm"]))


def test_every_arm_of_the_mpm_derivation_is_taken_at_every_size():
    """The neighbours of the decided CUs take every arm of the MPM list's derivation at 16x16, 8x8 and 4x4, a distance of
    exactly 62 (modes 2 and 64, 3 and 65, 4 and 66: where that arm begins) included; a 32x32 CU has its above neighbour
    across a CTU row, which counts as planar, so that only the last two arms exist for it."""
    arms = sum(mc.mpm_census(r) for kd in mc.ENCODES for r in mc.refs(*kd))
    text = "\n".join("%2d | %s" % (n, " ".join("%d" % v for v in row)) for n, row in zip(SIZES, arms))
    assert arms[:3].min() >= 1, "arms %s\n%s" % (mc.MPM_BRANCHES, text)
    assert arms[3, 6:].min() >= 1 and arms[3, :6].max() == 0, text


def test_the_oracle_final_pass_agrees_with_its_search():
    for kind, depth in mc.ENCODES:
        for seed, rec in zip(mc.SEEDS, mc.refs(kind, depth)):
            assert rec["final_pass_mismatches"] == 0, (kind, depth, seed)


def test_the_stream_pictures_hold_every_mode_at_the_planted_size():
    """tests/test_gpu_mode_census.py writes streams of the four pictures of a kind at the depth at which the planted size is
    the smallest CU: together they hold all 67 modes at that size."""
    for kind, (lg, w, h) in mc.KINDS.items():
        wins = sum(mc.census(r)["wins"][lg - 2] for r in mc.refs(kind, mc.depths(kind)[0]))
        assert wins.min() >= 1, (kind, np.flatnonzero(wins < 1).tolist())


def test_oracle_records_go_through_the_writer_and_the_spec_decoder(built):
    """The host's mode syntax and the independent decoder on the oracle's own records of the same pictures: the stream
    parses back to the record, and the spec decoder rebuilds the oracle's reconstruction from it (a difference here is a
    finding about the oracle or the writer, not about a kernel)."""
    from wrenc_amd import bitstream as bs
    from oracle import pyoracle as po
    for kind, (lg, w, h) in mc.KINDS.items():
        for s, (rec, qp) in enumerate(zip(mc.refs(kind, mc.depths(kind)[0]), mc.QPS)):
            stream = bs.write_parameter_sets(w, h, qp) + bs.write_picture(w, h, qp, s, rec)
            back = po.parse_picture(stream, 0)
            for k in ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr"):
                assert np.array_equal(back[k], rec[k]), (kind, s, k)
            for plane, k in zip(po.spec_decode_record(back, qp), ("rec_y", "rec_cb", "rec_cr")):
                assert np.array_equal(plane, rec[k]), (kind, s, k)


def test_the_set_is_cheap(total):
    """The GPU tests compute these references themselves: the whole set takes the oracle seconds."""
    assert mc.oracle_seconds() < 60.0


def test_the_pictures_are_small():
    """At most 72 CTUs, whole CTUs, one QP per seed."""
    assert len(mc.QPS) == len(mc.SEEDS)
    for kind, (lg, w, h) in mc.KINDS.items():
        assert w % 32 == 0 and h % 32 == 0 and (w // 32) * (h // 32) <= 72, kind
        for y, cb, cr in mc.frames(kind):
            assert y.shape == (h, w) and cb.shape == cr.shape == (h // 2, w // 2)
            assert not y.flags.writeable


def test_traces_fit_the_device_buffer():
    """The device records re-evaluations the oracle memoises, into a buffer of kTraceMax records that drops what does not
    fit: every traced encode makes at most a quarter of that in the oracle, every kind included, and pictures larger than
    160x128 are traced at depth 0 only."""
    src = open(os.path.join(ROOT, "wrenc_amd", "csrc", "dev_common.h")).read()
    m = re.search(r"constexpr unsigned kTraceMax = 1u << (\d+);", src)
    assert m and (1 << int(m.group(1))) == mc.TRACE_MAX
    worst = 0
    for kind, depth in mc.TRACED:
        lg, w, h = mc.KINDS[kind]
        assert depth == 0 or w * h <= 160 * 128, (kind, depth)
        for trace, n_raw in mc.traces(kind, depth):
            assert 0 < len(trace) <= n_raw <= mc.TRACE_MAX // 4, (kind, depth, len(trace), n_raw)
            assert mc.trace_census(trace)["kinds"] == {0, 1, 2, 3}, (kind, depth)
            worst = max(worst, n_raw)
    print("largest oracle trace: %d records of %d" % (worst, mc.TRACE_MAX))


def test_the_generator_is_deterministic():
    mc.picture.cache_clear()
    a = mc.picture("p8", 2)
    mc.picture.cache_clear()
    b = mc.picture("p8", 2)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_census_counts_a_hand_made_record():
    """census() on a 32x32 record made by hand: one 16x16 CU (mode 50, DM, a chroma level), one 16x16 with T_CCLM, one
    8x8 quadrant of 8x8 CUs, and a split 8x8 among them whose DM comes from its bottom-right 4x4 block."""
    cu = np.zeros((8, 8), np.uint8)
    lm = np.zeros((8, 8), np.uint8)
    cm = np.zeros((4, 4), np.uint8)
    cu[0:4, 0:4], lm[0:4, 0:4], cm[0:2, 0:2] = 4, 50, 50
    cu[0:4, 4:8], lm[0:4, 4:8], cm[0:2, 2:4] = 4, 18, mc.T_CCLM
    cu[4:8, 0:4], lm[4:8, 0:4], cm[2:4, 0:2] = 4, 0, 0
    cu[4:8, 4:8] = 3
    lm[4:6, 4:6], cm[2, 2] = 2, 2
    lm[4:6, 6:8], cm[2, 3] = 66, mc.L_CCLM
    lm[6:8, 4:6], cm[3, 2] = 1, 1
    cu[6:8, 6:8] = 2
    lm[6:8, 6:8] = [[10, 11], [12, 13]]
    cm[3, 3] = 13
    lev = [np.zeros((32, 32), np.int16), np.zeros((16, 16), np.int16), np.zeros((16, 16), np.int16)]
    lev[1][7, 7] = -1          # in the first 16x16 CU's Cb block
    lev[2][12, 15] = 2         # in the split 8x8's Cr block
    c = mc.census({"cu_log2_size": cu, "luma_mode": lm, "chroma_mode": cm, "lev_y": lev[0], "lev_cb": lev[1], "lev_cr": lev[2]})
    want = np.zeros((4, 67), np.int64)
    want[2, [50, 18, 0]] = 1
    want[1, [2, 66, 1]] = 1
    want[0, [10, 11, 12, 13]] = 1
    assert np.array_equal(c["wins"], want)
    dm = np.zeros((4, 67), np.int64)
    dm[1, [50, 0]] = 1
    dm[2, [2, 1]] = 1
    dm[3, 13] = 1
    assert np.array_equal(c["dm"], dm)
    nz = np.zeros((4, 67), np.int64)
    nz[1, 50] = 1
    nz[3, 13] = 1
    assert np.array_equal(c["dm_nz"], nz)
    cc = np.zeros((4, 3), np.int64)
    cc[1, 1] = 1
    cc[2, 2] = 1
    assert np.array_equal(c["cclm"], cc)
    t = mc.trace_census({(0, 0, 5, 0, 0, 34, 34): {1}, (0, 0, 5, 0, 1, 0, 0): {2}, (0, 0, 5, 0, 1, 0, 81): {3},
                         (4, 0, 2, 1, 0, 2, 2): {4}, (0, 0, 3, 2, 3, 0, 50): {5}})
    assert t["kinds"] == {0, 1, 3} and t["probes"][3, 34] == 1 and t["probes"][0, 2] == 1 and t["probes"].sum() == 2
    assert t["full"][3, 0] == 2 and t["full"].sum() == 2
