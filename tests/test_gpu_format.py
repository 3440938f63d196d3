"""Source formats on the device (include/wrenc_gpu.h: wrenc_gpu_set_source_format, wrenc_gpu_upload_planes; the kernel is
wrenc_amd/csrc/dev_format.h): the upload of a format's raw planes leaves the slot holding the picture format_ref.convert
makes of them, edge-padded to the coded size, bit for bit; with a source size, the scaled converted picture; and everything
behind it -- search, final pass, complexity, metrics -- is that of a plain context given that picture."""
import ctypes as C

import numpy as np
import pytest

import complexity_ref
import format_ref
import metrics_ref
import scale_ref
from window_stream import pad_planes, strided

pytestmark = pytest.mark.gpu

KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")
EINVAL, ESTATE = -1, -5
# source = visible (coded): whole CTUs; chroma 17 x 15 in one CTU row; chroma 35 x 25 over several CTUs; four CTUs
SIZES = [((32, 32), (32, 32)), ((34, 30), (64, 32)), ((70, 50), (96, 64)), ((64, 64), (64, 64))]
CASES = [(f, v, c) for f in format_ref.FORMATS for v, c in SIZES]
CASE_IDS = ["%s-%dx%d" % ((format_ref.NAMES[f],) + v) for f, v, _ in CASES]


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _encoder(fmt, visible, coded, source=None, **kw):
    from wrenc_amd import gpu
    return gpu.Encoder(coded[0], coded[1], qp=32, visible=visible if visible != coded else None, source=source, source_format=fmt, **kw)


_made = {}


def _pic(fmt, size, name, inverted=False):
    """(raw planes, their conversion) of picture `name`, computed once per format, size and picture."""
    key = (fmt, size, name, inverted)
    if key not in _made:
        raw = format_ref.picture(name, fmt, *size, inverted=inverted)
        _made[key] = (raw, format_ref.convert(fmt, raw))
    return _made[key]


@pytest.mark.parametrize("fmt,visible,coded", CASES, ids=CASE_IDS)
def test_slots_hold_the_converted_picture(built, fmt, visible, coded):
    """Both slots of a two-slot context, back to back without a sync between them, with different pictures out of planes with
    extra stride (the one set of raw staging planes serves both); then an inverted picture into slot 0: after each step the
    slot is the reference's picture, margin included, and the other slot is untouched."""
    enc = _encoder(fmt, visible, coded, max_split_depth=3, n_slots=2)
    assert enc.source_format() == fmt and enc.source_size() == visible
    names = list(format_ref.PICTURES)
    for a, b in zip(names, names[1:] + names[:1]):
        ra, ca = _pic(fmt, visible, a)
        rb, cb = _pic(fmt, visible, b)
        wa, wb = pad_planes(ca, *coded), pad_planes(cb, *coded)
        enc.upload_planes(0, format_ref.strided(ra, (24, 8, 8)))
        enc.upload_planes(1, format_ref.strided(rb, (8, 40, 40)))
        assert _same(enc.download_originals(0), wa), (a, "slot 0")
        assert _same(enc.download_originals(1), wb), (b, "slot 1")
        ri, ci = _pic(fmt, visible, a, inverted=True)
        enc.upload_planes(0, ri)
        assert _same(enc.download_originals(0), pad_planes(ci, *coded)), (a, "inverted")
        assert _same(enc.download_originals(1), wb), (b, "slot 1 after slot 0's upload")
    enc.close()


@pytest.mark.parametrize("fmt", [format_ref.YUV422P10LE, format_ref.NV12], ids=["yuv422p10le", "nv12"])
def test_format_and_scaling_together(built, fmt):
    """70x50 -> 34x30 in 64x32: the slot is the converted picture, scaled, padded.  The format is set first here, the sizes
    after it: the raw staging planes follow."""
    from wrenc_amd import gpu
    source, visible, coded = (70, 50), (34, 30), (64, 32)
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=3, n_slots=2, source_format=fmt)
    enc.set_visible_size(*visible)
    enc.set_source_size(*source)
    assert enc.source_format() == fmt and enc.source_size() == source
    for slot, name in ((1, "textured"), (0, "all10"), (1, "noise")):
        raw, conv = _pic(fmt, source, name)
        enc.upload_planes(slot, format_ref.strided(raw, (6, 10, 10)))
        want = pad_planes(scale_ref.scale_planes(conv, *visible), *coded)
        assert _same(enc.download_originals(slot), want), name
    enc.close()


def test_encode_is_that_of_the_converted_picture(built):
    """p010le, 64x64, depth 3, QP 32: the whole record is bit for bit that of a plain context given the numpy-converted planes."""
    from wrenc_amd import gpu
    fmt, size = format_ref.P010LE, (64, 64)
    raw, conv = _pic(fmt, size, "textured")
    enc = _encoder(fmt, size, size, max_split_depth=3, n_slots=2)
    enc.upload_planes(1, raw)
    enc.encode(1, 1)
    got = enc.download(1)
    assert enc.final_pass_mismatches() == 0
    enc.close()
    plain = gpu.Encoder(64, 64, qp=32, max_split_depth=3)
    want = plain.encode_picture(*conv)
    assert plain.final_pass_mismatches() == 0
    plain.close()
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert any(np.any(want[k] != 0) for k in ("lev_y", "lev_cb", "lev_cr"))


def test_complexity_and_metrics_see_the_converted_picture(built):
    fmt, visible, coded = format_ref.YUV422P10LE, (70, 50), (96, 64)
    raw, conv = _pic(fmt, visible, "textured")
    enc = _encoder(fmt, visible, coded, max_split_depth=2)
    enc.upload_planes(0, raw)
    complexity_ref.check(enc.download_complexity(0, 1)[0], *pad_planes(conv, *coded))   # over the coded picture, margin included
    enc.encode(0, 1)
    rec = enc.download(0, keys=("rec_y", "rec_cb", "rec_cr"))
    got = enc.download_metrics(0, 1)[0]
    enc.close()
    crop = tuple(np.ascontiguousarray(rec[k][:p.shape[0], :p.shape[1]]) for k, p in zip(("rec_y", "rec_cb", "rec_cr"), conv))
    metrics_ref.check_raw(got["_raw"], conv, crop)                                      # metrics: the visible rectangle
    metrics_ref.check_entry(got, conv, crop)


def test_format_0_is_the_plain_upload(built):
    """upload_planes on a context without a format, and on one put back to format 0, leaves what upload leaves."""
    from wrenc_amd import gpu
    visible, coded = (34, 30), (64, 32)
    pic = scale_ref.picture("textured", *visible)
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible)
    assert enc.source_format() == 0
    enc.upload(0, *pic)
    enc.upload_planes(1, strided(pic))
    want = enc.download_originals(0)
    assert _same(want, pad_planes(pic, *coded)) and _same(enc.download_originals(1), want)
    enc.close()
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible, source_format="p010le")
    enc.set_source_format("yuv420p")
    assert enc.source_format() == 0
    enc.upload_planes(1, pic)
    enc.upload(0, *pic)                                  # plain again: upload is served
    assert _same(enc.download_originals(1), want) and _same(enc.download_originals(0), want)
    enc.close()


def _upload_raw(enc, slot, ptrs, strides):
    """wrenc_gpu_upload_planes with addresses and strides of the caller's choosing; the return code."""
    enc.lib.wrenc_gpu_upload_planes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return enc.lib.wrenc_gpu_upload_planes(enc.ctx, slot, (C.c_void_p * 3)(*ptrs), (C.c_size_t * 3)(*strides))


def test_format_rules(built):
    from wrenc_amd import gpu
    size = (64, 64)
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2)

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert enc.lib.wrenc_gpu_last_error(enc.ctx)     # a message is left

    for bad in (-1, 6, 99):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.set_source_format(bad)
        assert e.value.code == EINVAL and enc.source_format() == 0
    with pytest.raises(gpu.WrencGpuError):
        enc.set_source_format("bogus")

    # a 16-bit three-plane format
    fmt = format_ref.YUV420P10LE
    enc.set_source_format(fmt)
    raw, conv = _pic(fmt, size, "textured")
    ptr = [p.ctypes.data for p in raw]
    row = [p.strides[0] for p in raw]
    for p in range(3):
        refused(_upload_raw(enc, 0, ptr[:p] + [None] + ptr[p + 1:], row), EINVAL, ("null plane", p))
        refused(_upload_raw(enc, 0, ptr, row[:p] + [row[p] - 2] + row[p + 1:]), EINVAL, ("short stride", p))
        refused(_upload_raw(enc, 0, ptr, row[:p] + [row[p] + 1] + row[p + 1:]), EINVAL, ("odd stride", p))
        refused(_upload_raw(enc, 0, ptr[:p] + [ptr[p] + 1] + ptr[p + 1:], [r + 2 for r in row]), EINVAL, ("odd pointer", p))
    refused(_upload_raw(enc, 1, ptr, row), EINVAL, "slot out of range")
    refused(_upload_raw(enc, -1, ptr, row), EINVAL, "slot out of range")
    # the uint8_t* entries cannot say what is meant
    refused(enc.lib.wrenc_gpu_upload(enc.ctx, 0, gpu._p(conv[0]), gpu._p(conv[1]), gpu._p(conv[2]), 64, 32), ESTATE, "upload")
    with pytest.raises(gpu.WrencGpuError) as e:
        enc.encode_picture(*conv)
    assert e.value.code == ESTATE
    # none of this was an upload: the format may still change, and the context works
    enc.set_source_format(format_ref.NV12)
    fmt = format_ref.NV12
    raw, conv = _pic(fmt, size, "textured")
    ptr = [p.ctypes.data for p in raw] + [None]
    row = [p.strides[0] for p in raw] + [0]
    refused(_upload_raw(enc, 0, [None, ptr[1], None], row), EINVAL, "null luma")
    refused(_upload_raw(enc, 0, [ptr[0], None, None], row), EINVAL, "null CbCr")
    refused(_upload_raw(enc, 0, ptr, [63, 64, 0]), EINVAL, "short luma stride")
    refused(_upload_raw(enc, 0, ptr, [64, 62, 0]), EINVAL, "short CbCr stride: w / 2 pairs are w bytes")
    odd = np.zeros(64 * 65 + 1, np.uint8)                 # an 8-bit format takes odd addresses and strides
    view = np.lib.stride_tricks.as_strided(odd[1:], (64, 64), (65, 1))
    view[:] = raw[0]
    assert view.ctypes.data % 2 == 1
    assert _upload_raw(enc, 0, [view.ctypes.data, ptr[1], None], [65, 64, 0]) == 0       # plane[2] and its stride are not read
    assert _same(enc.download_originals(0), conv)
    # a slot has been uploaded into
    for f in (0, format_ref.P010LE, format_ref.NV12):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.set_source_format(f)
        assert e.value.code == ESTATE and enc.source_format() == format_ref.NV12
    enc.upload_planes(0, _pic(fmt, size, "noise")[0])
    assert _same(enc.download_originals(0), _pic(fmt, size, "noise")[1])
    enc.close()


def test_one_picture_at_size(built):
    """yuv422p10le at 3840x2160 in 3840x2176 and p010le at 1920x1080 in 1920x1088, no encode: grid sizes and index arithmetic
    that only show at size."""
    for fmt, visible, coded, name in ((format_ref.YUV422P10LE, (3840, 2160), (3840, 2176), "textured"),
                                      (format_ref.P010LE, (1920, 1080), (1920, 1088), "noise")):
        raw = format_ref.picture(name, fmt, *visible)
        enc = _encoder(fmt, visible, coded, max_split_depth=2)
        enc.upload_planes(0, raw)
        got = enc.download_originals(0)
        enc.close()
        want = pad_planes(format_ref.convert(fmt, raw), *coded)
        for p in range(3):
            bad = np.argwhere(got[p] != want[p])
            assert bad.size == 0, (format_ref.NAMES[fmt], p, len(bad), bad[:4].tolist())
