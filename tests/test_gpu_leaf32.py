"""The wave kernels search the CTU's 32x32 leaf inside one request (wrenc_amd/csrc/dev_search.h: K_LEAF32, full_search):
planar, DC, the SAD search, cm, cm - 1, cm + 1, the CCLM part, with the running best in registers, a new best saved
straight to the leaf's slot and the winner restored from there.  Every record must stay what the walk through single
requests made, so the pictures of tests/leaf32_inputs.py (3x3 CTUs: every neighbour availability; the cases are pinned
by tests/test_leaf32_inputs.py) are held, on all ten planes and bit for bit,

  * against the CPU oracle in the wave schedule at max-split-depth 0, 1, 2 and 3 (the leaf is the CTU's decision, or the
    unsplit candidate whose slot the split's restore reads);
  * in the AUTO and the TEAM schedule at depth 3 against the wave schedule's records (the team kernels keep the single
    requests);
  * in one call with two QPs against the oracle at each picture's QP."""
import numpy as np
import pytest

import leaf32_inputs as li


def _same(got, ref, what):
    for k in li.KEYS:
        if not np.array_equal(got[k], ref[k]):
            bad = np.argwhere(np.asarray(got[k]) != np.asarray(ref[k]))
            raise AssertionError("%s: %s differs at %d positions, first %s" % (what, k, len(bad), bad[0]))


def _encode(depth, schedule, qps=None):
    from wrenc_amd import gpu
    frames = li.frames()
    enc = gpu.Encoder(li.W, li.H, qp=li.QP, max_split_depth=depth, n_slots=len(frames), schedule=schedule)
    try:
        for s, f in enumerate(frames):
            enc.upload(s, *f)
            if qps is not None:
                enc.set_qp(s, qps[s])
        enc.encode(0, len(frames))
        enc.sync()
        assert enc.final_pass_mismatches() == 0
        if schedule:
            assert enc.last_schedule() == schedule
        return [enc.download(s) for s in range(len(frames))]
    finally:
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", li.DEPTHS)
def test_wave_records_equal_the_oracle(built, depth):
    got, refs = _encode(depth, 1), li.refs(li.QP, depth)
    for s, k in enumerate(li.KINDS):
        _same(got[s], refs[s], "wave, depth %d, %s" % (depth, k))


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", [0, 2])
def test_auto_and_team_records_equal_the_wave_schedule(built, schedule):
    wave, got, refs = _encode(3, 1), _encode(3, schedule), li.refs(li.QP, 3)
    for s, k in enumerate(li.KINDS):
        _same(got[s], wave[s], "schedule %d against wave, %s" % (schedule, k))
        _same(got[s], refs[s], "schedule %d against the oracle, %s" % (schedule, k))


@pytest.mark.gpu
def test_mixed_qp_call_equals_the_oracle(built):
    """two QPs in one call of the wave kernel: each picture's record is the oracle's at its own QP"""
    qps = [27, 37, 37, 27]
    got = _encode(3, 1, qps)
    for s, k in enumerate(li.KINDS):
        _same(got[s], li.refs(qps[s], 3)[s], "mixed QPs, %s at QP %d" % (k, qps[s]))
