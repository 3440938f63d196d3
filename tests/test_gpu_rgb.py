"""RGB sources on the device (include/wrenc_gpu.h: wrenc_gpu_set_source_rgb; the kernel is wrenc_amd/csrc/dev_rgb.h): the
upload of a layout's raw planes leaves the slot holding the picture rgb_ref.convert makes of them, edge-padded to the coded
size, bit for bit; with a source size, the scaled converted picture; and the encode behind it is that of a plain context
given that picture."""
import ctypes as C

import numpy as np
import pytest

import rgb_ref
import scale_ref
from window_stream import pad_planes

pytestmark = pytest.mark.gpu

KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")
EINVAL, ESTATE = -1, -5
# source = visible (coded): whole CTUs; a row tail inside a lane's group and chroma 17 x 15; chroma 35 x 25 over several CTUs
SIZES = [((32, 32), (32, 32)), ((34, 30), (64, 32)), ((70, 50), (96, 64))]
SOURCES = [(lay, rgb_ref.BT709, rgb_ref.TV) for lay in rgb_ref.LAYOUTS] + [(rgb_ref.RGB24, m, r) for m, r in rgb_ref.COMBOS[1:]]
CASES = [(s, v, c) for s in SOURCES for v, c in SIZES]
CASE_IDS = ["%s-%s-%s-%dx%d" % ((rgb_ref.NAMES[s[0]], rgb_ref.MATRICES[s[1]], rgb_ref.RANGES[s[2]]) + v) for s, v, _ in CASES]


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _encoder(source, visible, coded, **kw):
    from wrenc_amd import gpu
    return gpu.Encoder(coded[0], coded[1], qp=32, visible=visible if visible != coded else None, source_rgb=source, **kw)


_made = {}


def _pic(source, size, name, inverted=False):
    """(raw planes, their conversion) of picture `name`, computed once per source, size and picture."""
    key = (source, size, name, inverted)
    if key not in _made:
        raw = rgb_ref.picture(name, source[0], *size, inverted=inverted)
        _made[key] = (raw, rgb_ref.convert(*source, raw))
    return _made[key]


def _planes(raw):
    return raw if len(raw) > 1 else raw[0]


@pytest.mark.parametrize("source,visible,coded", CASES, ids=CASE_IDS)
def test_slots_hold_the_converted_picture(built, source, visible, coded):
    """Both slots of a two-slot context, back to back without a sync between them, with different pictures out of planes with
    extra stride (the one set of raw staging planes serves both); then an inverted picture into slot 0: after each step the
    slot is the reference's picture, margin included, and the other slot is untouched."""
    enc = _encoder(source, visible, coded, max_split_depth=3, n_slots=2)
    assert enc.source_rgb() == source and enc.source_format() == 0 and enc.source_size() == visible
    names = list(rgb_ref.PICTURES)
    for a, b in zip(names, names[1:] + names[:1]):
        ra, ca = _pic(source, visible, a)
        rb, cb = _pic(source, visible, b)
        wa, wb = pad_planes(ca, *coded), pad_planes(cb, *coded)
        enc.upload_rgb(0, _planes(rgb_ref.strided(ra, (24, 8, 8))))
        enc.upload_rgb(1, _planes(rgb_ref.strided(rb, (7, 40, 40))))
        assert _same(enc.download_originals(0), wa), (a, "slot 0")
        assert _same(enc.download_originals(1), wb), (b, "slot 1")
        ri, ci = _pic(source, visible, a, inverted=True)
        enc.upload_rgb(0, _planes(ri))
        assert _same(enc.download_originals(0), pad_planes(ci, *coded)), (a, "inverted")
        assert _same(enc.download_originals(1), wb), (b, "slot 1 after slot 0's upload")
    enc.close()


@pytest.mark.parametrize("lay", [rgb_ref.BGR24, rgb_ref.GBRP], ids=["bgr24", "gbrp"])
def test_rgb_and_scaling_together(built, lay):
    """70x50 -> 34x30 in 64x32: the slot is the converted picture, scaled, padded.  The RGB source is set first here, the
    sizes after it: the raw staging planes follow."""
    from wrenc_amd import gpu
    source, size, visible, coded = (lay, rgb_ref.BT601, rgb_ref.PC), (70, 50), (34, 30), (64, 32)
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=3, n_slots=2, source_rgb=("%s" % rgb_ref.NAMES[lay], "bt601", "pc"))
    enc.set_visible_size(*visible)
    enc.set_source_size(*size)
    assert enc.source_rgb() == source and enc.source_size() == size
    for slot, name in ((1, "textured"), (0, "corners"), (1, "noise")):
        raw, conv = _pic(source, size, name)
        enc.upload_rgb(slot, _planes(rgb_ref.strided(raw, (6, 10, 10))))
        want = pad_planes(scale_ref.scale_planes(conv, *visible), *coded)
        assert _same(enc.download_originals(slot), want), name
    enc.close()


def test_encode_is_that_of_the_converted_picture(built):
    """rgb24, 64x64, depth 3, QP 32: the whole record is bit for bit that of a plain context given the numpy-converted planes."""
    from wrenc_amd import gpu
    source, size = (rgb_ref.RGB24, rgb_ref.BT709, rgb_ref.TV), (64, 64)
    raw, conv = _pic(source, size, "textured")
    enc = _encoder(source, size, size, max_split_depth=3, n_slots=2)
    enc.upload_rgb(1, raw[0])
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


def _upload_raw(enc, slot, ptrs, strides):
    """wrenc_gpu_upload_planes with addresses and strides of the caller's choosing; the return code."""
    return enc.lib.wrenc_gpu_upload_planes(enc.ctx, slot, (C.c_void_p * 3)(*ptrs), (C.c_size_t * 3)(*strides))


def test_rgb_rules(built):
    from wrenc_amd import gpu
    size = (64, 64)
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2)

    def refused(rc, code, what):
        assert rc == code, (what, rc)
        assert enc.lib.wrenc_gpu_last_error(enc.ctx)     # a message is left

    def raises(code, fn, *args):
        with pytest.raises(gpu.WrencGpuError) as e:
            fn(*args)
        assert e.value.code == code, (args, e.value.code)

    assert enc.source_rgb() == (-1, 0, 0)
    for bad in ((5, 0, 0), (-2, 0, 0), (99, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2), (0, 0, -1)):
        raises(EINVAL, enc.set_source_rgb, *bad)
        assert enc.source_rgb() == (-1, 0, 0)
    raises(EINVAL, enc.set_source_rgb, "bogus")
    raises(EINVAL, enc.set_source_rgb, "rgb24", "bt2020")
    raises(EINVAL, enc.set_source_rgb, "rgb24", "bt709", "full")

    # exclusive with a non-zero source format, in both orders
    enc.set_source_format("nv12")
    raises(ESTATE, enc.set_source_rgb, "rgb24")
    raises(ESTATE, enc.set_source_rgb, -1)
    assert enc.source_format() == 1 and enc.source_rgb() == (-1, 0, 0)
    enc.set_source_format(0)
    enc.set_source_rgb("gbrp", "bt601", "pc")
    assert enc.source_rgb() == (rgb_ref.GBRP, rgb_ref.BT601, rgb_ref.PC) and enc.source_format() == 0
    raises(ESTATE, enc.set_source_format, "p010le")
    enc.set_source_format(0)                             # a no-op that succeeds: the RGB source stays
    assert enc.source_rgb() == (rgb_ref.GBRP, rgb_ref.BT601, rgb_ref.PC) and enc.source_format() == 0

    # gbrp reads three planes
    source = (rgb_ref.GBRP, rgb_ref.BT601, rgb_ref.PC)
    raw, conv = _pic(source, size, "textured")
    ptr = [p.ctypes.data for p in raw]
    row = [p.strides[0] for p in raw]
    for p in range(3):
        refused(_upload_raw(enc, 0, ptr[:p] + [None] + ptr[p + 1:], row), EINVAL, ("null plane", p))
        refused(_upload_raw(enc, 0, ptr, row[:p] + [row[p] - 1] + row[p + 1:]), EINVAL, ("short stride", p))
    refused(_upload_raw(enc, 1, ptr, row), EINVAL, "slot out of range")
    refused(_upload_raw(enc, -1, ptr, row), EINVAL, "slot out of range")
    # the uint8_t* entries cannot say what is meant
    refused(enc.lib.wrenc_gpu_upload(enc.ctx, 0, gpu._p(conv[0]), gpu._p(conv[1]), gpu._p(conv[2]), 64, 32), ESTATE, "upload")
    raises(ESTATE, enc.encode_picture, *conv)
    # none of this was an upload: the source may still change, through -1 or directly, and the context works
    enc.set_source_rgb(-1)
    assert enc.source_rgb() == (-1, 0, 0)
    enc.set_source_format("nv12")
    enc.set_source_format(0)
    enc.set_source_rgb("gbrp", "bt601", "pc")
    enc.set_source_rgb("bgr0", "bt709", "tv")
    source = (rgb_ref.BGR0, rgb_ref.BT709, rgb_ref.TV)
    assert enc.source_rgb() == source
    raw, conv = _pic(source, size, "textured")
    d = raw[0].ctypes.data
    refused(_upload_raw(enc, 0, [None, d, d], [256, 256, 256]), EINVAL, "null plane")
    refused(_upload_raw(enc, 0, [d, None, None], [255, 0, 0]), EINVAL, "short stride: 4 w bytes a row")
    assert _upload_raw(enc, 0, [d, None, None], [256, 0, 0]) == 0        # plane[1], plane[2] and their strides are not read
    assert _same(enc.download_originals(0), conv)
    # a slot has been uploaded into
    for args in (("rgb24",), (-1,), ("bgr0", "bt709", "tv")):
        raises(ESTATE, enc.set_source_rgb, *args)
        assert enc.source_rgb() == source
    raises(ESTATE, enc.set_source_format, 0)
    raw, conv = _pic(source, size, "noise")
    enc.upload_rgb(0, raw[0])
    assert _same(enc.download_originals(0), conv)
    enc.close()
    # a context put back to no RGB source takes plain pictures again
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2, source_rgb="rgb24")
    assert enc.source_rgb() == (0, 0, 0)
    enc.set_source_rgb(None)
    enc.upload(0, *conv)
    assert _same(enc.download_originals(0), conv)
    enc.close()
