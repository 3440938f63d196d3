"""Search parity on pictures where every intra mode wins at every CU size (tests/mode_census_inputs.py; what the pictures
hold is pinned on the CPU by tests/test_mode_census_inputs.py).

Picture-level parity compares winners, and what the search does with a winner -- the save of a new best to the leaf's slot
and the restore from it, fill_maps, the MPM lists of the later neighbours, the DM chroma prediction at the chroma block's
size, the final pass, the host's mode syntax -- runs only with the modes that win somewhere.  On these pictures each of the
67 luma modes is the decision of at least two CUs of every size, DM wins with every luma mode in every chroma situation, each
CCLM mode wins in each, every mode 2..66 is a SAD probe and every mode a full candidate at every size:

  * the record of every (picture, depth) in both schedules and in AUTO against the oracle's, bit for bit, the four pictures of
    a kind in one call at four QPs;
  * every candidate the device evaluates against the oracle's trace (f32 bits), in both schedules;
  * the stream written from the device's record against the one from its tokens, and through the parser and the spec decoder
    back to the record's modes and the device's reconstruction."""
import numpy as np
import pytest

import mode_census_inputs as mc
from test_gpu_picture import _compare
from trace_common import assert_trace_matches, gpu_trace, trace_gpu  # noqa: F401  (trace_gpu is a fixture)

pytestmark = pytest.mark.gpu

CTX_QP = 30      # of the context; every slot carries its own


def _encode(kind, depth, schedule):
    """The four pictures of a kind in one encode call, QPS[i] on slot i."""
    from wrenc_amd import gpu
    lg, w, h = mc.KINDS[kind]
    enc = gpu.Encoder(w, h, qp=CTX_QP, max_split_depth=depth, n_slots=len(mc.SEEDS), schedule=schedule)
    for s, (f, qp) in enumerate(zip(mc.frames(kind), mc.QPS)):
        enc.upload(s, *f)
        enc.set_qp(s, qp)
    enc.encode(0, len(mc.SEEDS))
    enc.sync()
    return enc


@pytest.mark.parametrize("schedule", [1, 2, 0])    # one wave per CTU / a team of four waves per CTU / AUTO
@pytest.mark.parametrize("kind,depth", mc.ENCODES)
def test_records_match_oracle(built, kind, depth, schedule):
    refs = mc.refs(kind, depth)
    enc = _encode(kind, depth, schedule)
    try:
        assert enc.final_pass_mismatches() == 0
        if schedule:
            assert enc.last_schedule() == schedule
        for s, ref in enumerate(refs):
            _compare(enc.download(s), ref, "%s seed %d qp%d d%d schedule %d" % (kind, mc.SEEDS[s], mc.QPS[s], depth, schedule))
    finally:
        enc.close()


@pytest.mark.parametrize("schedule", [1, 2])
@pytest.mark.parametrize("seed", range(len(mc.SEEDS)))
@pytest.mark.parametrize("kind,depth", mc.TRACED)
def test_every_candidate_cost_matches_oracle(trace_gpu, kind, depth, seed, schedule):
    ref = mc.refs(kind, depth)[seed]
    otrace, _ = mc.traces(kind, depth)[seed]
    got, gtrace, n = gpu_trace(trace_gpu, *mc.picture(kind, mc.SEEDS[seed]), mc.QPS[seed], depth, schedule)
    assert n < mc.TRACE_MAX, "the device's trace buffer is full: records were dropped"
    _compare(got, ref, "%s seed %d d%d schedule %d (trace build)" % (kind, mc.SEEDS[seed], depth, schedule))
    assert_trace_matches(gtrace, otrace)


@pytest.mark.parametrize("kind", list(mc.KINDS))
def test_streams_carry_every_mode(built, kind):
    """The four pictures of a kind at the depth at which the planted size is the smallest CU: the host's mode syntax with all
    67 modes at that size (tests/test_mode_census_inputs.py), each beside neighbours of every mode (every MPM position, the
    truncated-binary remainder)."""
    from wrenc_amd import bitstream as bs
    from oracle import pyoracle as po
    lg, w, h = mc.KINDS[kind]
    depth = mc.depths(kind)[0]
    enc = _encode(kind, depth, None)
    try:
        pool, pics = enc.download_tokens(0, len(mc.SEEDS))
        recs = [enc.download(s) for s in range(len(mc.SEEDS))]
    finally:
        enc.close()
    for s, (got, qp) in enumerate(zip(recs, mc.QPS)):
        _compare(got, mc.refs(kind, depth)[s], "%s seed %d" % (kind, mc.SEEDS[s]))
        pic = bs.write_picture(w, h, qp, s, got)
        assert pic == bs.write_picture_tokens(w, h, qp, s, pool, pics[s]), s
        back = po.parse_picture(bs.write_parameter_sets(w, h, qp) + pic, 0)
        for k in ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr"):
            assert np.array_equal(back[k], got[k]), (s, k)
        for plane, k in zip(po.spec_decode_record(back, qp), ("rec_y", "rec_cb", "rec_cr")):
            assert np.array_equal(plane, got[k]), (s, k)
