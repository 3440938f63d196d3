"""The generator of tests/pack_sparse_inputs.py against the oracle alone: what test_gpu_pack_sparse.py relies on is checked
here without a device."""
import numpy as np
import pytest

import pack_sparse_inputs as ps
from oracle import pyoracle as po


@pytest.mark.parametrize("qp", ps.QPS)
def test_the_three_kinds_are_what_they_claim(qp):
    """For every pack of every shape: a zero block has no coefficient; a quiet block has coefficients and the oracle
    gives it no level; a live block gets a level.  Every luma assignment and every chroma pattern occurs."""
    for log2n, nc in ps.PACKS:
        kinds, luma, chroma = ps.plan(qp, log2n, nc)
        assert len(kinds) == 3 ** nc * (2 * nc + 2)
        assert len(luma) == nc * len(kinds) and len(chroma) == 2 * len(luma)
        assert len({lk for lk, _ in kinds}) == 3 ** nc and len({ck for _, ck in kinds}) == 2 * nc + 2
        for p, (lk, ck) in enumerate(kinds):
            blocks = list(zip(lk, luma[p * nc:(p + 1) * nc])) + list(zip(ck, chroma[p * 2 * nc:(p + 1) * 2 * nc]))
            for kind, b in blocks:
                ref = po.quantize(b, qp)
                if kind == "zero":
                    assert not b.any()
                elif kind == "quiet":
                    assert b.any() and not ref.any(), (qp, log2n, nc, p)
                else:
                    assert ref.any(), (qp, log2n, nc, p)


def test_the_chroma_patterns():
    """All quiet, one live chain in each position (for three candidates chains 4 and 5 too, the second pass of four 4x4
    blocks), all live."""
    for nc in (1, 2, 3):
        pats = ps.chroma_patterns(nc)
        assert pats[0] == ("quiet",) * (2 * nc) and pats[-1] == ("live",) * (2 * nc)
        assert [p.index("live") for p in pats[1:-1]] == list(range(2 * nc))
        assert all(p.count("live") == 1 for p in pats[1:-1])
