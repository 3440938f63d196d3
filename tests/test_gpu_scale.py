"""Scaling on the device (include/wrenc_gpu.h: wrenc_gpu_set_source_size; the kernel is wrenc_amd/csrc/dev_scale.h): the
upload of source-size planes leaves the slot holding the picture scale_ref makes of them, edge-padded to the coded size, bit
for bit; and everything behind it -- search, final pass, complexity, metrics -- is that of a plain context given that
picture."""
import numpy as np
import pytest

import complexity_ref
import metrics_ref
import scale_ref
from window_stream import pad_planes, strided

pytestmark = pytest.mark.gpu

KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")
EINVAL, ESTATE = -1, -5


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _encoder(source, visible, coded, **kw):
    from wrenc_amd import gpu
    return gpu.Encoder(coded[0], coded[1], qp=32, visible=visible if visible != coded else None, source=source, **kw)


_wanted = {}


def _want(source, visible, coded, name, invert=False):
    """The slot contents expected of picture `name` (computed once per size and picture)."""
    key = (source, visible, coded, name, invert)
    if key not in _wanted:
        pic = scale_ref.picture(name, *source)
        if invert:
            pic = tuple(255 - p for p in pic)
        _wanted[key] = (pic, pad_planes(scale_ref.scale_planes(pic, *visible), *coded))
    return _wanted[key]


@pytest.mark.parametrize("source,visible,coded", scale_ref.SIZES, ids=scale_ref.SIZE_IDS)
def test_slots_hold_the_scaled_picture(built, source, visible, coded):
    """Both slots of a two-slot context, back to back, with different pictures out of planes with extra stride (the one set of
    staging planes serves both); then an inverted picture into slot 0: after each step the slot is the reference's picture
    and the other slot is untouched."""
    enc = _encoder(source, visible, coded, max_split_depth=3, n_slots=2)
    assert enc.source_size() == source and enc.visible_size() == visible
    names = list(scale_ref.PICTURES)
    for a, b in zip(names, names[1:] + names[:1]):
        pa, wa = _want(source, visible, coded, a)
        pb, wb = _want(source, visible, coded, b)
        enc.upload_strided(0, *strided(pa))
        enc.upload_strided(1, *strided(pb, extra=(8, 40, 40)))
        assert _same(enc.download_originals(0), wa), (a, "slot 0")
        assert _same(enc.download_originals(1), wb), (b, "slot 1")
        pi, wi = _want(source, visible, coded, a, invert=True)
        enc.upload(0, *pi)
        assert _same(enc.download_originals(0), wi), (a, "inverted")
        assert _same(enc.download_originals(1), wb), (b, "slot 1 after slot 0's upload")
    enc.close()


@pytest.mark.parametrize("source,visible,coded", [scale_ref.SIZES[3], scale_ref.SIZES[2]], ids=["shrink-pad", "enlarge"])
def test_encode_is_that_of_the_scaled_picture(built, source, visible, coded):
    """Depth 3, QP 32: the whole record is bit for bit that of a plain context of the coded size given the numpy-scaled,
    numpy-padded planes."""
    from wrenc_amd import gpu
    pic, want_org = _want(source, visible, coded, "textured")
    enc = _encoder(source, visible, coded, max_split_depth=3, n_slots=2)
    enc.upload_strided(1, *strided(pic))
    enc.encode(1, 1)
    got = enc.download(1)
    assert enc.final_pass_mismatches() == 0
    enc.close()
    plain = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=3)
    want = plain.encode_picture(*want_org)
    assert plain.final_pass_mismatches() == 0
    plain.close()
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert any(np.any(want[k] != 0) for k in ("lev_y", "lev_cb", "lev_cr"))


def test_complexity_and_metrics_see_the_scaled_picture(built):
    source, visible, coded = scale_ref.SIZES[3]
    pic, want_org = _want(source, visible, coded, "textured")
    enc = _encoder(source, visible, coded, max_split_depth=2)
    enc.upload(0, *pic)
    complexity_ref.check(enc.download_complexity(0, 1)[0], *want_org)       # over the coded picture, margin included
    enc.encode(0, 1)
    rec = enc.download(0, keys=("rec_y", "rec_cb", "rec_cr"))
    got = enc.download_metrics(0, 1)[0]
    enc.close()
    scaled = scale_ref.scale_planes(pic, *visible)                          # metrics: the visible rectangle
    crop = tuple(np.ascontiguousarray(rec[k][:p.shape[0], :p.shape[1]]) for k, p in zip(("rec_y", "rec_cb", "rec_cr"), scaled))
    metrics_ref.check_raw(got["_raw"], scaled, crop)
    metrics_ref.check_entry(got, scaled, crop)


def test_source_size_rules(built):
    from wrenc_amd import gpu
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2)
    assert enc.source_size() == (64, 64)

    def refused(w, h, code):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.set_source_size(w, h)
        assert e.value.code == code, (w, h)
        assert enc.source_size() == (enc.src_width, enc.src_height)

    for w, h in ((65, 64), (64, 63), (14, 64), (64, 14), (258, 64), (64, 258)):
        refused(w, h, EINVAL)
    enc.set_source_size(256, 16)                 # 4:1 down and 4:1 up are the limits
    assert enc.source_size() == (256, 16)
    with pytest.raises(gpu.WrencGpuError) as e:  # the visible size comes first
        enc.set_visible_size(64, 64)
    assert e.value.code == ESTATE
    enc.set_source_size(64, 64)                  # the visible size itself: plain again
    assert enc.source_size() == (64, 64)
    enc.set_visible_size(34, 62)
    assert enc.source_size() == (34, 62)
    refused(138, 62, EINVAL)                     # the ratio is taken against the visible size
    enc.set_source_size(70, 50)
    pic = scale_ref.picture("textured", 70, 50)
    for stride_y, stride_c in ((64, 35), (70, 34)):   # a stride below the source width, at or above the visible width
        with pytest.raises(gpu.WrencGpuError) as e:
            enc._check(enc.lib.wrenc_gpu_upload(enc.ctx, 0, gpu._p(pic[0]), gpu._p(pic[1]), gpu._p(pic[2]), stride_y, stride_c))
        assert e.value.code == EINVAL
    enc.upload(0, *pic)
    refused(64, 64, ESTATE)                      # a slot has been uploaded into
    refused(34, 62, ESTATE)
    assert enc.source_size() == (70, 50)
    enc.close()


def test_the_visible_size_restores_plain_uploads(built):
    from wrenc_amd import gpu
    pic = scale_ref.picture("textured", 64, 64)
    fresh = gpu.Encoder(64, 64, qp=32, max_split_depth=3)
    want = fresh.encode_picture(*pic)
    fresh.close()
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=3, source=(128, 96))
    enc.set_source_size(64, 64)
    got = enc.encode_picture(*pic)               # planes of 64x64 again
    assert _same(enc.download_originals(0), pic)
    enc.close()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k


def test_one_picture_at_size(built):
    """3840x2160 -> 1920x1080 in 1920x1088, no encode: grid sizes and index arithmetic that only show at size."""
    source, visible, coded = (3840, 2160), (1920, 1080), (1920, 1088)
    pic = scale_ref.picture("textured", *source)
    enc = _encoder(source, visible, coded, max_split_depth=2)
    enc.upload(0, *pic)
    got = enc.download_originals(0)
    enc.close()
    want = pad_planes(scale_ref.scale_planes(pic, *visible), *coded)
    for p in range(3):
        bad = np.argwhere(got[p] != want[p])
        assert bad.size == 0, (p, len(bad), bad[:4].tolist())
