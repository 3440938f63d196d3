"""Whole records against the oracle's (pyoracle.encode_picture) over small pictures whose CUs hold levels in every
combination of luma and chroma and pick CCLM at every size (tests/pack_records_cases.py; test_pack_records_cases.py checks
that of the oracle's records on the CPU), in both schedules: the packed leaf searches trace only the chains that have
something to trace, and the CCLM tail of a leaf predicts from the probe's down-sampled luma."""
import numpy as np
import pytest

import pack_records_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("schedule", [1, 2])    # one wave per CTU / a team of four waves per CTU
@pytest.mark.parametrize("kind,size,qp,depth", pc.CASES)
def test_record_matches_the_oracle(built, kind, size, qp, depth, schedule):
    from wrenc_amd import gpu
    w, h = size
    ref = pc.reference(kind, size, qp, depth)
    enc = gpu.Encoder(w, h, qp=qp, max_split_depth=depth, schedule=schedule)
    try:
        got = enc.encode_picture(*pc.picture(kind, size, qp))
        assert enc.final_pass_mismatches() == 0
    finally:
        enc.close()
    for k in pc.KEYS:
        if not np.array_equal(got[k], ref[k]):
            bad = np.argwhere(got[k] != ref[k])
            raise AssertionError("%s %dx%d qp%d d%d schedule %d: %s differs at %d positions, first %s (got %s want %s)" % (
                kind, w, h, qp, depth, schedule, k, len(bad), bad[0], got[k][tuple(bad[0])], ref[k][tuple(bad[0])]))
