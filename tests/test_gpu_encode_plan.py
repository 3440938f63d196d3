"""An encode call runs the plan wrenc_gpu_test_plan gives for its arguments (wrenc_amd/csrc/encode_plan.h): what the
statistics entry points and wrenc_gpu_last_schedule report after a mixed-QP call under AUTO, with team and wave diagonals
in one call, and after a call at one QP on the same context, is what the plan says -- and the pictures are the oracle's."""
import numpy as np
import pytest

from content import content
from encode_plan_ref import span_stats

pytestmark = pytest.mark.gpu

W = H = 96                                  # 3 x 3 CTUs, 7 diagonals of 1, 1, 2, 1, 2, 1, 1 CTUs
QPS = (30, 32, 32, 35, 30, 32)
CTX_QP = 32
KINDS = ("noise", "cclm", "stripes20", "checker", "ramp", "extremes")
PLANES = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")

_FRAMES = [content(k, W, H, 70 + i) for i, k in enumerate(KINDS)]
_ORACLE = {}


def _oracle(slot, qp, depth):
    from oracle import pyoracle as po
    key = (slot, qp, depth)
    if key not in _ORACLE:
        _ORACLE[key] = po.encode_picture(*_FRAMES[slot], qp, depth)
    return _ORACLE[key]


def _check_call(enc, qps, depth, slots):
    from wrenc_amd import gpu
    n = len(qps)
    enc.encode(0, n)
    plan = gpu.encode_plan(W // 32, H // 32, qps, gpu.Encoder.SCHEDULE_AUTO, slots, depth == 3)
    want = span_stats(plan)
    assert set(L["team"] for L in plan["launches"]) == {0, 1} and plan["schedule"] == gpu.Encoder.SCHEDULE_AUTO
    assert enc.last_encode_stats()["n_launches"] == want["n_launches"] == plan["n_spans"]
    got = enc.last_encode_kernel_stats()
    for kernel in ("wave", "team"):
        assert got[kernel]["ctu_pictures"] == want[kernel]["ctu_pictures"], kernel
        assert got[kernel]["launches"] == want[kernel]["launches"], kernel
    assert got["wave"]["ctu_pictures"] + got["team"]["ctu_pictures"] == n * (W // 32) * (H // 32)
    assert enc.last_schedule() == plan["schedule"]
    for s in range(n):
        pic = enc.download(s)
        ref = _oracle(s, qps[s], depth)
        for k in PLANES:
            assert np.array_equal(pic[k], ref[k]), (s, qps[s], k)
    assert enc.final_pass_mismatches() == 0


@pytest.mark.parametrize("depth", [2, 3])
def test_encode_runs_its_plan(built, depth):
    from wrenc_amd import gpu
    n = len(QPS)
    enc = gpu.Encoder(W, H, qp=CTX_QP, max_split_depth=depth, n_slots=n, schedule=gpu.Encoder.SCHEDULE_AUTO)
    # one-CTU diagonals as teams, two-CTU ones as waves: n x 1 x 100 <= slots x pct < n x 2 x 100
    slots = (200 * n - 1) // (65 if depth == 3 else 50)
    enc.test_set_wave_slots(slots)
    enc.stats_enable()
    for s in range(n):
        enc.upload(s, *_FRAMES[s])
        enc.set_qp(s, QPS[s])
    _check_call(enc, list(QPS), depth, slots)                   # mixed: a list, three classes, team launches per class
    for s in range(n):
        enc.set_qp(s, None)
    _check_call(enc, [CTX_QP] * n, depth, slots)                # one QP: the slots in place
    enc.close()
