"""The three source kernels past their first workgroup and their first tile (wrenc_amd/csrc/dev_format.h, dev_rgb.h,
dev_scale.h): every format and every RGB layout at a picture 1030 wide -- three workgroups along a luma row, two along a
chroma row, a row tail in the last lane of each -- and at one 1022 wide, whose tail is the last lane of the grid; and the
scaler over several tiles per row at 4 : 1, at the widest column span, at 1 : 4 and at mixed ratios, bit for bit against
format_ref, rgb_ref and scale_ref.  The sizes are those of
tests/source_geometry.py; test_source_geometry.py shows on the host that they reach what they are named for."""
import numpy as np
import pytest

import format_ref
import rgb_ref
import scale_ref
import source_geometry as sg
from test_gpu_format import KEYS
from window_stream import pad_planes, strided

pytestmark = pytest.mark.gpu

_, WIDE, WIDE_CODED = sg.CASES["wide"]
FORMAT_CASES = [(c, f) for c in sg.UNSCALED for f in format_ref.FORMATS]
FORMAT_IDS = ["%s-%s" % (c, format_ref.NAMES[f]) for c, f in FORMAT_CASES]
RGB_SOURCES = [(lay, rgb_ref.BT709, rgb_ref.TV) for lay in rgb_ref.LAYOUTS] + [(rgb_ref.RGB24, m, r) for m, r in rgb_ref.COMBOS[1:]]
RGB_CASES = [(c, s) for c in sg.UNSCALED for s in RGB_SOURCES]
RGB_IDS = ["%s-%s-%s-%s" % (c, rgb_ref.NAMES[s[0]], rgb_ref.MATRICES[s[1]], rgb_ref.RANGES[s[2]]) for c, s in RGB_CASES]


def _differences(got, want):
    """'' when the three planes are equal, else where they first differ."""
    out = []
    for p, (g, w) in enumerate(zip(got, want)):
        if g.shape != w.shape:
            out.append("plane %d: shape %s for %s" % (p, g.shape, w.shape))
            continue
        bad = np.argwhere(g != w)
        if bad.size:
            out.append("plane %d: %d differ, first (row, column) %s" % (p, len(bad), bad[:4].tolist()))
    return "; ".join(out)


def _margin_is_the_edge_sample(planes, visible):
    """Right of the visible rectangle, in its rows, every byte is the row's last visible sample: where a store that took
    no notice of the row's end would have left its own."""
    for p, s in zip(planes, (0, 1, 1)):
        w, h = visible[0] >> s, visible[1] >> s
        assert p.shape[1] > w and np.array_equal(p[:h, w:], np.repeat(p[:h, w - 1:w], p.shape[1] - w, axis=1))


_made = {}


def _format_pic(fmt, size, name, inverted=False):
    """(raw planes, their conversion): once per format, size and picture, read-only."""
    key = ("format", fmt, size, name, inverted)
    if key not in _made:
        raw = format_ref.picture(name, fmt, *size, inverted=inverted)
        _made[key] = (raw, format_ref.convert(fmt, raw))
    return _made[key]


def _rgb_pic(source, size, name, inverted=False):
    key = ("rgb", source, size, name, inverted)
    if key not in _made:
        raw = rgb_ref.picture(name, source[0], *size, inverted=inverted)
        _made[key] = (raw, rgb_ref.convert(*source, raw))
    return _made[key]


def _scale_pic(case, name, inverted=False):
    """(source planes, the slot expected of them)."""
    key = ("scale", case, name, inverted)
    if key not in _made:
        source, visible, coded = sg.CASES[case]
        pic = scale_ref.picture(name, *source)
        if inverted:
            pic = tuple(255 - p for p in pic)
        _made[key] = (pic, pad_planes(scale_ref.scale_planes(pic, *visible), *coded))
    return _made[key]


def _rgb_planes(raw):
    return raw if len(raw) > 1 else raw[0]


def _walk_slots(enc, names, upload, pictures, visible=None):
    """Slot 0 out of strided planes and slot 1 out of planes with another stride, back to back; then an inverted picture into
    slot 0: after each step both slots are exact, margin included.  pictures(name, inverted) -> (planes, the slot expected);
    upload(slot, planes, which stride)."""
    for a, b in zip(names, names[1:] + names[:1]):
        pa, wa = pictures(a, False)
        pb, wb = pictures(b, False)
        upload(0, pa, 0)
        upload(1, pb, 1)
        got0, got1 = enc.download_originals(0), enc.download_originals(1)
        assert not _differences(got0, wa), (a, "slot 0", _differences(got0, wa))
        assert not _differences(got1, wb), (b, "slot 1", _differences(got1, wb))
        if visible is not None:
            _margin_is_the_edge_sample(got0, visible)
            _margin_is_the_edge_sample(got1, visible)
        pi, wi = pictures(a, True)
        upload(0, pi, None)
        got0, got1 = enc.download_originals(0), enc.download_originals(1)
        assert not _differences(got0, wi), (a, "inverted", _differences(got0, wi))
        assert not _differences(got1, wb), (b, "slot 1 after slot 0's upload", _differences(got1, wb))
        if visible is not None:
            _margin_is_the_edge_sample(got0, visible)


@pytest.mark.parametrize("case,fmt", FORMAT_CASES, ids=FORMAT_IDS)
def test_formats_past_the_first_workgroup(built, case, fmt):
    """1030x18 in 1056x32 (three workgroups along a luma row) and 1022x18 in 1024x32 (the last lane of the grid live): all10
    (10-bit saturation, every value), noise (words above 1023, junk low bits) and ones (the clamp before the shift over a
    full row)."""
    from wrenc_amd import gpu
    _, visible, coded = sg.CASES[case]
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible, source_format=fmt)
    assert enc.source_format() == fmt and enc.source_size() == visible

    def pictures(name, inverted):
        raw, conv = _format_pic(fmt, visible, name, inverted)
        return raw, pad_planes(conv, *coded)

    def upload(slot, raw, stride):
        enc.upload_planes(slot, raw if stride is None else format_ref.strided(raw, ((24, 8, 8), (8, 40, 40))[stride]))

    _walk_slots(enc, ["all10", "noise", "ones"], upload, pictures, visible)
    enc.close()


@pytest.mark.parametrize("case,source", RGB_CASES, ids=RGB_IDS)
def test_rgb_past_the_first_workgroup(built, case, source):
    """The same two sizes: noise and corners (pc: pure blue and red reach 256 before the chroma clamp); gbrp out of three
    planes of three strides."""
    from wrenc_amd import gpu
    _, visible, coded = sg.CASES[case]
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible, source_rgb=source)
    assert enc.source_rgb() == source and enc.source_size() == visible

    def pictures(name, inverted):
        raw, conv = _rgb_pic(source, visible, name, inverted)
        return raw, pad_planes(conv, *coded)

    def upload(slot, raw, stride):
        enc.upload_rgb(slot, _rgb_planes(raw if stride is None else rgb_ref.strided(raw, ((24, 8, 16), (7, 40, 5))[stride])))

    _walk_slots(enc, ["noise", "corners"], upload, pictures, visible)
    enc.close()


@pytest.mark.parametrize("case", sg.SCALED)
def test_scaler_over_several_tiles_a_row(built, case):
    """checker1 (the overshoot clips at both ends in every tile), noise and ones."""
    from wrenc_amd import gpu
    source, visible, coded = sg.CASES[case]
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible if visible != coded else None, source=source)
    assert enc.source_size() == source and enc.visible_size() == visible

    def upload(slot, pic, stride):
        if stride is None:
            enc.upload(slot, *pic)
        else:
            enc.upload_strided(slot, *strided(pic, extra=((24, 8, 8), (8, 40, 40))[stride]))

    _walk_slots(enc, ["checker1", "noise", "ones"], upload, lambda name, inverted: _scale_pic(case, name, inverted))
    enc.close()


CHAINS = [("format", format_ref.P010LE, "s_mixed", "all10"), ("format", format_ref.YUV422P, "s_span", "noise"),
          ("rgb", (rgb_ref.GBRP, rgb_ref.BT601, rgb_ref.PC), "s4to1", "corners"), ("rgb", (rgb_ref.BGR0, rgb_ref.BT709, rgb_ref.TV), "s1to4", "noise")]


@pytest.mark.parametrize("kind,what,case,name", CHAINS, ids=["p010le-s_mixed", "yuv422p-s_span", "gbrp-s4to1", "bgr0-s1to4"])
def test_convert_scale_and_pad_in_one_chain(built, kind, what, case, name):
    """One upload each: the converter writes the scaler's staging planes at their own pitch, the scaler the slot, the pad
    its margin."""
    from wrenc_amd import gpu
    source, visible, coded = sg.CASES[case]
    kw = {"source_format": what} if kind == "format" else {"source_rgb": what}
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible if visible != coded else None, source=source, **kw)
    assert enc.source_size() == source and enc.visible_size() == visible
    if kind == "format":
        raw, conv = _format_pic(what, source, name)
        enc.upload_planes(1, format_ref.strided(raw, (6, 10, 10)))
    else:
        raw, conv = _rgb_pic(what, source, name)
        enc.upload_rgb(1, _rgb_planes(rgb_ref.strided(raw, (6, 10, 3))))
    want = pad_planes(scale_ref.scale_planes(conv, *visible), *coded)
    got = enc.download_originals(1)
    enc.close()
    assert not _differences(got, want), _differences(got, want)


def test_encode_behind_a_wide_converted_source(built):
    """nv12, 1030x18 in 1056x32 (33 CTU columns, one row), depth 2, QP 32: the whole record is that of a plain context of the
    coded size given the numpy-converted, numpy-padded planes -- the tiling of the picture for the search included."""
    from wrenc_amd import gpu
    raw, conv = _format_pic(format_ref.NV12, WIDE, "textured")
    want_org = pad_planes(conv, *WIDE_CODED)
    enc = gpu.Encoder(WIDE_CODED[0], WIDE_CODED[1], qp=32, max_split_depth=2, n_slots=2, visible=WIDE, source_format=format_ref.NV12)
    enc.upload_planes(1, raw)
    enc.encode(1, 1)
    got = enc.download(1)
    assert enc.final_pass_mismatches() == 0
    enc.close()
    plain = gpu.Encoder(WIDE_CODED[0], WIDE_CODED[1], qp=32, max_split_depth=2)
    want = plain.encode_picture(*want_org)
    assert plain.final_pass_mismatches() == 0
    plain.close()
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert any(np.any(want[k] != 0) for k in ("lev_y", "lev_cb", "lev_cr"))
