"""The candidate cut of the 4x4 luma leaf search on the device (wrenc_amd/csrc/dev_search.h, kCandidateCut): once pack
{planar, DC} is evaluated, the SAD search and pack {cm, cm - 1, cm + 1} are skipped where the header bits of every
candidate still to come already cost as much as the running best.  The decision is the reference's, so every record
stays what the exhaustive search makes:

  * pictures of 64x64, 96x64 and 160x128 at max-split-depth 3, each of smooth, flat, textured and noise content, four
    slots per call at QP 22 / 32 / 37 / 51 (every slot with the floors of its own QP), in the wave schedule and in AUTO
    calls that mix team (exhaustive) and wave (cut) diagonals: every plane of the record and the f32 CTU costs equal the
    oracle's, and the stream written from the record goes through the spec decoder to the device's reconstruction;
  * one case against the build of the same sources with -DWRENC_EXHAUSTIVE_CANDIDATES where that build exists
    (tools/build_exp.sh exhaustive_candidates -DWRENC_EXHAUSTIVE_CANDIDATES), and always against the trace build, which
    evaluates every candidate.

What the inputs exercise is shown on the CPU from the oracle's trace alone (tests/candidate_floors.py), among the leaves
the split cut still searches: both rules fire on smooth inputs; on flat inputs the first rule fires (a flat block's
planar candidate costs its floor, which is below every angular floor, so the second rule never gets its turn there);
neither fires on noise.  tests/test_candidate_floor.py holds the rule and the floors themselves."""
import os

import numpy as np
import pytest

import candidate_floors as cf
import split_floors as sf
from content import content

pytestmark = pytest.mark.gpu

KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr",
        "ctu_cost")
SIZES = ((64, 64), (96, 64), (160, 128))
QPS = (22, 32, 37, 51)
KINDS = ("smooth", "flat", "textured", "noise")
_refs = {}


def _frame(kind, w, h):
    from wrenc_amd import synth
    if kind == "smooth":
        return synth.synth_frame(w, h, 0)
    if kind == "textured":
        return synth.synth_textured_frame(w, h, 0)
    return content(kind, w, h, 60)


def _ref(kind, w, h, qp):
    """(oracle record, what the rule does on it), computed once per input."""
    key = (kind, w, h, qp)
    if key not in _refs:
        from wrenc_amd import gpu
        rec, rows = sf.ordered_trace(*_frame(kind, w, h), qp, 3)
        _refs[key] = (rec, cf.counts(rec, rows, w, h, gpu.default_config(w, h, qp, 3)))
    return _refs[key]


def _same(got, ref, what):
    for k in KEYS:
        if not np.array_equal(got[k], ref[k]):
            bad = np.argwhere(got[k] != ref[k])
            raise AssertionError("%s: %s differs at %d positions, first %s" % (what, k, len(bad), bad[0]))


def _run(enc, refs, what):
    enc.encode(0, len(refs))
    enc.sync()
    assert enc.final_pass_mismatches() == 0
    out = [enc.download(s) for s in range(len(refs))]
    for s, got in enumerate(out):
        _same(got, refs[s], "%s slot %d" % (what, s))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_records_equal_the_oracle(built, kind, w, h):
    from wrenc_amd import bitstream, gpu
    from oracle import pyoracle as po
    refs = [_ref(kind, w, h, qp)[0] for qp in QPS]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=3, n_slots=len(QPS), schedule=gpu.Encoder.SCHEDULE_WAVE)
    frame = _frame(kind, w, h)
    for s, qp in enumerate(QPS):
        enc.upload(s, *frame)
        enc.set_qp(s, qp)
    got = _run(enc, refs, "%s %dx%d wave" % (kind, w, h))
    assert enc.last_schedule() == 1
    enc.set_schedule(gpu.Encoder.SCHEDULE_AUTO)
    ctus = (w // 32) * (h // 32)
    enc.test_set_wave_slots(max(1, (200 * len(QPS) - 1) // 65) if ctus > 4 else 20)
    _run(enc, refs, "%s %dx%d auto" % (kind, w, h))
    enc.close()
    for s, qp in enumerate(QPS):
        stream = bitstream.write_parameter_sets(w, h, qp) + bitstream.write_picture(w, h, qp, 0, got[s])
        back = po.parse_picture(stream, 0)
        for a, k in zip(po.spec_decode_record(back, qp), ("rec_y", "rec_cb", "rec_cr")):
            assert np.array_equal(a, got[s][k]), "%s %dx%d QP %d: the spec decoder's %s differs" % (kind, w, h, qp, k)


def test_the_inputs_exercise_both_rules(built):
    """Conditions on the inputs, from the oracle alone."""
    fired = {k: {"sad": 0, "packB": 0, "searched": 0} for k in KINDS}
    for kind in KINDS:
        for w, h in SIZES:
            for qp in QPS:
                c = _ref(kind, w, h, qp)[1]
                for k in fired[kind]:
                    fired[kind][k] += c[k]
    print(fired)
    assert fired["smooth"]["sad"] > 0 and fired["smooth"]["packB"] > 0
    assert fired["flat"]["sad"] > 0
    assert fired["noise"]["searched"] > 0 and fired["noise"]["sad"] == 0 and fired["noise"]["packB"] == 0
    for kind in ("smooth", "textured"):
        assert fired[kind]["sad"] + fired[kind]["packB"] < fired[kind]["searched"], "leaves that run pack B too"


def _encode_with(gpu, path, frames, w, h, qps):
    saved = (gpu._lib, gpu.LIB_PATH)
    gpu._lib, gpu.LIB_PATH = None, path
    try:
        enc = gpu.Encoder(w, h, qp=32, max_split_depth=3, n_slots=len(frames), schedule=1)
        for s, f in enumerate(frames):
            enc.upload(s, *f)
            enc.set_qp(s, qps[s])
        enc.encode(0, len(frames))
        enc.sync()
        assert enc.final_pass_mismatches() == 0
        out = [enc.download(s) for s in range(len(frames))]
        enc.close()
        return out
    finally:
        gpu._lib, gpu.LIB_PATH = saved


def test_records_equal_the_exhaustive_builds(built):
    from wrenc_amd import gpu
    w, h = 160, 128
    frames = [_frame(k, w, h) for k in KINDS] * 2
    qps = (32, 32, 32, 32, 37, 22, 51, 37)
    product = gpu.LIB_PATH
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(product))))
    others = [os.path.join(os.path.dirname(product), "libwrenc_gpu_trace.so")]
    assert os.path.exists(others[0]), "run __graft_entry__.build() first"
    exhaustive = os.path.join(root, "xbuild", "exhaustive_candidates.so")
    if os.path.exists(exhaustive):
        others.append(exhaustive)
    cut = _encode_with(gpu, product, frames, w, h, qps)
    for path in others:
        full = _encode_with(gpu, path, frames, w, h, qps)
        for s in range(len(frames)):
            _same(cut[s], full[s], "%s picture %d" % (os.path.basename(path), s))
