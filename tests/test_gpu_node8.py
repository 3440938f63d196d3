"""The wave schedule at max-split-depth 3 decides an 8x8 node inside one request, and the four 8x8 children of a 16x16
node in one (wrenc_amd/csrc/dev_search.h: node8_search, K_SPLIT16): the unsplit 8x8 candidate waits in registers while
its split is searched and is put back when the split loses; a split cut before its first leaf restores nothing; the
16x16 split is cut between siblings inside the request.  Every record must stay what the walk through single requests
made, so the same batch is held

  * against the CPU oracle on all ten planes, whole and with padding waves in the last workgroup;
  * against the team schedule, whose kernels keep the single requests, and against the exhaustive build
    (libwrenc_gpu_trace.so), which never cuts: a node restored after some leaves ran, a node skipped whole and a 16x16
    split cut between siblings all have to end as the full search does;
  * against itself with the pictures rotated through the slots: a kept block must not survive a CTU or a picture.

The shapes put a node at the picture corner, in pictures one CTU wide and one CTU tall, and at every in-CTU position.
Before anything runs on the device, the oracle's records alone must show that every (shape, QP) batch holds each
outcome a node can have (test_batches_hold_every_outcome)."""
import functools
import os

import numpy as np
import pytest

KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr",
        "ctu_cost")
SHAPES = [(64, 64), (32, 96), (96, 32)]
QPS = [22, 27, 32, 37]
DEPTH = 3
MIN_OF_EACH = 4


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    from content import content
    from wrenc_amd import synth
    return tuple([synth.synth_frame(w, h, 0)] + [synth.synth_textured_frame(w, h, i) for i in range(3)] +
                 [content(k, w, h, 41) for k in ("stripes45", "extremes", "flat", "cclm")])


@functools.lru_cache(maxsize=None)
def _refs(w, h, qp):
    """The oracle's records of the batch: computed once, shared by every test, never written to."""
    from oracle import pyoracle as po
    refs = tuple(po.encode_picture(*f, qp, DEPTH) for f in _frames(w, h))
    for r in refs:
        for k in KEYS:
            r[k].setflags(write=False)
    return refs


def _outcomes(refs):
    lg = np.concatenate([r["cu_log2_size"].ravel() for r in refs])
    n = {"cu32": int((lg == 5).sum()) // 64, "cu16": int((lg == 4).sum()) // 16, "split8": int((lg == 2).sum()) // 4,
         "cu8_dm": 0, "cu8_cclm": 0}
    for r in refs:
        is8 = r["cu_log2_size"][::2, ::2] == 3        # one entry per 8x8 block, as chroma_mode has
        n["cu8_dm"] += int((is8 & (r["chroma_mode"] < 81)).sum())
        n["cu8_cclm"] += int((is8 & (r["chroma_mode"] >= 81)).sum())
    return n


def _same(got, ref, what):
    for k in KEYS:
        if not np.array_equal(got[k], ref[k]):
            bad = np.argwhere(np.asarray(got[k]) != np.asarray(ref[k]))
            raise AssertionError("%s: %s differs at %d positions, first %s" % (what, k, len(bad), bad[0]))


def _encode(gpu, frames, w, h, qp, schedule, path=None):
    """The records of `frames`, slot by slot, from the product library or from the one at `path`."""
    saved = (gpu._lib, gpu.LIB_PATH)
    if path is not None:
        gpu._lib, gpu.LIB_PATH = None, path
    try:
        enc = gpu.Encoder(w, h, qp=qp, max_split_depth=DEPTH, n_slots=len(frames), schedule=schedule)
        try:
            for s, f in enumerate(frames):
                enc.upload(s, *f)
            enc.encode(0, len(frames))
            enc.sync()
            assert enc.last_schedule() == schedule and enc.final_pass_mismatches() == 0
            return [enc.download(s) for s in range(len(frames))]
        finally:
            enc.close()
    finally:
        gpu._lib, gpu.LIB_PATH = saved


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("qp", QPS)
def test_batches_hold_every_outcome(built, w, h, qp):
    """From the oracle's records alone: 32x32 CUs, 16x16 CUs (a 16x16 split that lost), 8x8 CUs with DM and with CCLM
    chroma (the restore must bring the CCLM pair back) and split 8x8 nodes, at least four of each in every batch."""
    n = _outcomes(_refs(w, h, qp))
    assert min(n.values()) >= MIN_OF_EACH, n


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("qp", QPS)
def test_records_equal_the_oracle(built, w, h, qp):
    """Wave schedule: all eight pictures, then the first five alone (padding waves in the last workgroup)."""
    from wrenc_amd import gpu
    frames, refs = _frames(w, h), _refs(w, h, qp)
    for n in (len(frames), 5):
        got = _encode(gpu, frames[:n], w, h, qp, 1)
        for s in range(n):
            _same(got[s], refs[s], "%dx%d qp%d, %d pictures, slot %d" % (w, h, qp, n, s))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("qp", QPS)
def test_records_equal_the_team_schedule_and_the_exhaustive_build(built, w, h, qp):
    from wrenc_amd import gpu
    frames = _frames(w, h)
    exhaustive = os.path.join(os.path.dirname(gpu.LIB_PATH), "libwrenc_gpu_trace.so")
    assert os.path.exists(exhaustive), "run __graft_entry__.build() first"
    wave = _encode(gpu, frames, w, h, qp, 1)
    team = _encode(gpu, frames, w, h, qp, 2)
    full = _encode(gpu, frames, w, h, qp, 1, exhaustive)
    for s in range(len(frames)):
        _same(wave[s], team[s], "%dx%d qp%d wave against team, slot %d" % (w, h, qp, s))
        _same(wave[s], full[s], "%dx%d qp%d wave against the exhaustive build, slot %d" % (w, h, qp, s))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("qp", QPS)
def test_slots_reused(built, w, h, qp):
    """One context: the batch, then the pictures rotated by three slots.  Nothing kept from the previous CTU or picture
    of a slot may show."""
    from wrenc_amd import gpu
    frames, refs = _frames(w, h), _refs(w, h, qp)
    n = len(frames)
    enc = gpu.Encoder(w, h, qp=qp, max_split_depth=DEPTH, n_slots=n, schedule=1)
    try:
        for rot in (0, 3):
            for s in range(n):
                enc.upload(s, *frames[(s + rot) % n])
            enc.encode(0, n)
            enc.sync()
            assert enc.last_schedule() == 1 and enc.final_pass_mismatches() == 0
            for s in range(n):
                _same(enc.download(s), refs[(s + rot) % n], "%dx%d qp%d rotated by %d, slot %d" % (w, h, qp, rot, s))
    finally:
        enc.close()
