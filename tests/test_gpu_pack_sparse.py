"""quantize_pk (wrenc_amd/csrc/dev_quant.h) on packs whose chains are zero, quiet or live in every combination, against the
oracle's literal DFS, compared as test_gpu_quant_bounds.py compares its packs: the levels of every block, the level cost
of every luma block and chroma pair, the dequantised chroma levels.  The packed quantiser traces only the chains that have
something to trace; a chain it leaves out must come back as zeros with level cost 0 beside chains that are traced, in
every position of the pack (tests/pack_sparse_inputs.py; test_pack_sparse_inputs.py holds the generator against the
oracle on the CPU)."""
import pytest

import pack_sparse_inputs as ps
from test_gpu_quant_bounds import _Oracle, _check_packs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("log2n,nc", ps.PACKS)
@pytest.mark.parametrize("qp", ps.QPS)
def test_sparse_packs_match_the_oracle(built, qp, log2n, nc):
    from wrenc_amd import gpu
    oracle = _Oracle(qp)
    kinds, luma, chroma = ps.plan(qp, log2n, nc)
    # what the generator claims, asserted of what is sent
    for kind, b in zip([k for lk, _ in kinds for k in lk], luma):
        assert oracle(b)[0].any() == (kind == "live"), (qp, log2n, nc, kind)
    for kind, b in zip([k for _, ck in kinds for k in ck], chroma):
        assert oracle(b)[0].any() == (kind == "live"), (qp, log2n, nc, kind)
    e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
    try:
        compared = _check_packs(e, oracle, luma, chroma, log2n, nc, (qp, log2n, nc))
    finally:
        e.close()
    print("qp %d log2n %d nc %d: %d packs, %d blocks compared" % (qp, log2n, nc, len(kinds), compared))
