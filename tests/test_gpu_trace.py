"""Candidate-level parity: every evaluation the GPU search makes -- the SAD of every listed mode, the
RD cost of every full candidate, every chroma cost -- equals what the oracle's search computed for the
same block, mode and tree type, bit for bit.  Picture-level parity only sees the winners; this also
pins the candidates that lose.

Uses the diagnostic build libwrenc_gpu_trace.so (same sources, -DWRENC_TRACE: the kernel appends a
record per evaluation); the oracle records its own evaluations in the same layout."""
import numpy as np
import pytest

from trace_common import assert_trace_matches, gpu_trace, trace_gpu  # noqa: F401  (trace_gpu is a fixture)

pytestmark = pytest.mark.gpu


def _gpu_trace(gpu, y, cb, cr, qp, depth, schedule, extra_params=None):
    return gpu_trace(gpu, y, cb, cr, qp, depth, schedule, extra_params)[:2]


@pytest.mark.parametrize("kind,w,h,qp,depth", [
    ("tex", 64, 64, 32, 2), ("tex", 96, 64, 27, 3), ("cclm", 128, 64, 32, 2), ("stripes45", 64, 64, 27, 2),
    ("noise", 64, 64, 37, 3), ("tex", 64, 32, 22, 1), ("tex3", 96, 64, 32, 3), ("tex3", 128, 96, 37, 3),
    ("tex", 64, 64, 32, 0),     # max-split-depth 0: the only depth at which the team's CCLM stages leave trace records
])
@pytest.mark.parametrize("schedule", [1, 2])    # one wave per CTU / a team of four waves per CTU
def test_every_candidate_cost_matches_oracle(trace_gpu, kind, w, h, qp, depth, schedule):
    from oracle import pyoracle as po
    from wrenc_amd import synth
    if kind.startswith("tex"):
        y, cb, cr = synth.synth_textured_frame(w, h, 3 if kind == "tex3" else 9)
    else:
        from test_gpu_content import _content
        y, cb, cr = _content(kind, w, h, 77)
    got, gtrace = _gpu_trace(trace_gpu, y, cb, cr, qp, depth, schedule)
    ref, otrace = po.encode_picture_traced(y, cb, cr, qp, depth)
    assert np.array_equal(got["ctu_cost"], ref["ctu_cost"])
    assert_trace_matches(gtrace, otrace)
