"""The device buffers a context makes or remakes after wrenc_gpu_create (wrenc_amd/csrc/host_mem.h owns them): the per-call
scratch of every read-back, grown by a larger call and kept by a smaller one; the scaler's and the converter's staging
planes, set, set again and dropped; the per-QP constant blocks and the picture lists of mixed-QP calls; and contexts made,
used and destroyed in a row.  Small pictures: what is checked is that every value is the one the references in tests/
give whatever was allocated before, not the kernels' coverage.  (No allocation is made to fail here: the failure paths are
tools/sanitize/host_mem.cpp's.)"""
import numpy as np
import pytest

import complexity_ref
import metrics_ref
import picture_hash_ref
import ratecurve_ref

pytestmark = pytest.mark.gpu

W, H, QP, DEPTH, SLOTS = 64, 64, 32, 2, 3
KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")
ENOMEM = -3


def _frames():
    from wrenc_amd import synth
    return [synth.synth_textured_frame(W, H, s) for s in range(SLOTS)]


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


def _one_three_one(read, check, same):
    """read(n) -> n entries; the entries of one picture, of three (the scratch grows) and of one again: slot 0's the same
    every time, all of them what check(slot, entry) asks."""
    first, grown, again = read(1), read(SLOTS), read(1)
    assert len(first) == len(again) == 1 and len(grown) == SLOTS
    for s in range(SLOTS):
        check(s, grown[s])
    check(0, first[0])
    assert same(first[0], grown[0]) and same(first[0], again[0])


def test_scratch_made_after_create(built):
    from oracle import pyoracle
    from wrenc_amd import bitstream as bs, gpu
    frames = _frames()
    enc = gpu.Encoder(W, H, qp=QP, max_split_depth=DEPTH, n_slots=SLOTS)
    for s, f in enumerate(frames):
        enc.upload(s, *f)
    # (the passes over the originals run before the search as well as after it)
    cplx = [complexity_ref.complexity(*f) for f in frames]
    _one_three_one(lambda n: enc.download_complexity(0, n), lambda s, e: complexity_ref.check(e, *frames[s], ref=cplx[s]),
                   lambda a, b: a["satd"] == b["satd"] and np.array_equal(a["ctu_satd"], b["ctu_satd"]))
    enc.encode(0, SLOTS)
    recs = [enc.download(s) for s in range(SLOTS)]
    _same(recs[0], pyoracle.encode_picture(*frames[0], QP, DEPTH), "slot 0 against the oracle")
    planes = [(r["rec_y"], r["rec_cb"], r["rec_cr"]) for r in recs]

    def check_metrics(s, e):
        metrics_ref.check_raw(e["_raw"], frames[s], planes[s])
        metrics_ref.check_entry(e, frames[s], planes[s])
    _one_three_one(lambda n: enc.download_metrics(0, n), check_metrics, lambda a, b: a["_raw"]["bytes"] == b["_raw"]["bytes"])

    for tname, t in picture_hash_ref.TYPES:
        def check_hash(s, e):
            assert e.values(tname) == picture_hash_ref.picture_values(t, planes[s]), (tname, s)
        _one_three_one(lambda n: enc.download_hashes(0, n, tname), check_hash, lambda a, b: bytes(a) == bytes(b))

    def check_compact(s, e):
        mask, payload, maps = e
        for got, k in zip(enc.expand_levels(mask, payload), ("lev_y", "lev_cb", "lev_cr")):
            assert np.array_equal(got, recs[s][k]), (s, k)
        for k in ("cu_log2_size", "luma_mode", "chroma_mode"):
            assert np.array_equal(maps[k], recs[s][k]), (s, k)
    _one_three_one(lambda n: enc.download_compact(0, n), check_compact,
                   lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))

    def tokens(n, pool_words):
        pool, pics = enc.download_tokens(0, n, pool_words=pool_words)
        return [bs.write_picture_tokens(W, H, QP, s, pool, pics[s]) for s in range(n)]

    def check_tokens(s, e):
        assert e == bs.write_picture(W, H, QP, s, recs[s]), s
    big = SLOTS * W * H * 8
    _one_three_one(lambda n: tokens(n, big), check_tokens, lambda a, b: a == b)
    with pytest.raises(gpu.WrencGpuError) as e:      # a pool too small for the pictures: reported, as tests/test_gpu_tokens.py expects
        enc.download_tokens(0, SLOTS, pool_words=gpu.TOKEN_PAGE * 2)
    assert e.value.code == ENOMEM
    for s, stream in enumerate(tokens(SLOTS, big)):  # ... and a large one works afterwards
        check_tokens(s, stream)

    _one_three_one(lambda n: enc.download_complexity(0, n), lambda s, e: complexity_ref.check(e, *frames[s], ref=cplx[s]),
                   lambda a, b: a["satd"] == b["satd"] and np.array_equal(a["ctu_satd"], b["ctu_satd"]))
    hists = [ratecurve_ref.rate_hist(*f) for f in frames]

    def check_hist(s, e):
        assert np.array_equal(e, hists[s]), s
    _one_three_one(lambda n: list(enc.download_rate_hist(0, n)), check_hist, np.array_equal)

    # two per-slot QPs in one mixed call, then three: a call's picture list belongs to its entry of the ring of calls in
    # flight (8), so each size is asked for often enough that every entry is made by the first and grown by the second
    want = {q: [pyoracle.encode_picture(*frames[s], q, DEPTH) for s in range(SLOTS)] for q in (27, 37)}
    want[QP] = recs
    for qps in ((27, 37), (27, 37, None)):
        for s, q in enumerate(qps):
            enc.set_qp(s, q)
        for _ in range(8):
            enc.encode(0, len(qps))
        for s, q in enumerate(qps):
            _same(enc.download(s), want[QP if q is None else q][s], ("mixed call", qps, s))
    assert enc.final_pass_mismatches() == 0
    assert enc.test_scratch_overflows() == 0
    enc.close()


def test_staging_planes_set_and_dropped(built):
    """A source size twice and back to none, a source format and back: the context is a plain one again."""
    from wrenc_amd import gpu
    frame = _frames()[0]
    plain = gpu.Encoder(W, H, qp=QP, max_split_depth=DEPTH)
    want = plain.encode_picture(*frame)
    plain.close()
    enc = gpu.Encoder(W, H, qp=QP, max_split_depth=DEPTH)
    enc.set_source_size(48, 32)
    enc.set_source_size(128, 96)
    enc.set_source_size(W, H)
    enc.set_source_format("nv12")
    enc.set_source_format("yuv420p")
    assert enc.source_size() == (W, H) and enc.source_format() == 0
    _same(enc.encode_picture(*frame), want, "after the settings")
    assert enc.final_pass_mismatches() == 0
    enc.close()


def test_contexts_in_a_row(built):
    """Create, use (staging planes, a search, a mixed-QP call, read-backs with scratch of their own), destroy: ten times."""
    from wrenc_amd import bitstream as bs, gpu
    frames = _frames()
    first = None

    def stream(pool, pics):      # (which page a CTU's tokens got differs from run to run: the bytes written from them do not)
        return bs.write_picture_tokens(W, H, QP, 0, pool, pics[0])
    for _ in range(10):
        enc = gpu.Encoder(W, H, qp=QP, max_split_depth=DEPTH, n_slots=SLOTS, source=(128, 96), source_format="nv12")
        enc.set_source_format("yuv420p")
        enc.set_source_size(W, H)
        for s, f in enumerate(frames):
            enc.upload(s, *f)
        enc.set_qp(1, 27)
        enc.encode(0, SLOTS)
        got = (enc.download(0), enc.download_metrics(0, SLOTS)[0]["_raw"]["bytes"], bytes(enc.download_hashes(0, SLOTS, "md5")[0]),
               enc.download_compact(0, SLOTS)[0][1], stream(*enc.download_tokens(0, SLOTS)), enc.download_complexity(0, SLOTS)[0]["satd"],
               enc.download_rate_hist(0, SLOTS)[0])
        assert enc.final_pass_mismatches() == 0
        enc.close()
        first = first or got
        _same(got[0], first[0], "record")
        assert got[1] == first[1] and got[2] == first[2] and got[4] == first[4] and got[5] == first[5]
        assert np.array_equal(got[3], first[3]) and np.array_equal(got[6], first[6])
