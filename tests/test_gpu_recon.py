"""Reconstruction out on the device (include/wrenc_gpu.h: wrenc_gpu_download_recon, wrenc_gpu_download_recon_device;
wrenc_amd/csrc/dev_recon.h; wrenc_amd/torch_source.py: download_tensor) against include/wrenc_recon.h as tests/recon_ref.py
restates it, byte for byte: planes no search emits put into slots by wrenc_gpu_test_load_recon, with a margin unlike the
visible edge; the device entry's ordering against the consumer stream; a real encode; and the tensor round trip."""
import numpy as np
import pytest

import recon_ref as rr
import rgb_ref
import source_geometry as sg

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("torch sees no GPU", allow_module_level=True)

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
# name -> (visible, coded): three workgroups along a row with a tail of six pixels in the last lane and nine row pairs; the
# tail in the last lane of the grid; an unpadded context
SIZES = {"wide": sg.CASES["wide"][1:], "wide_last": sg.CASES["wide_last"][1:], "plain64": ((64, 64), (64, 64))}
FORMATS = [(f, rr.BT709, rr.TV) for f in range(7)] + [(rr.RGB24, m, r) for m, r in ((rr.BT709, rr.PC), (rr.BT601, rr.TV), (rr.BT601, rr.PC))]

_made = {}


def _content(name):
    """Per case, made once and left unchanged: two visible pictures (noise, corners) and their coded-size planes."""
    if name not in _made:
        (w, h), (cw, ch) = SIZES[name]
        vis = (rr.noise(w, h, 21), rr.corners(w, h))
        _made[name] = [(v, rr.with_margin(v, cw, ch)) for v in vis]
    return _made[name]


def _encoder(name, **kw):
    from wrenc_amd import gpu
    (w, h), (cw, ch) = SIZES[name]
    return gpu.Encoder(cw, ch, qp=32, max_split_depth=2, n_slots=2, visible=None if (w, h) == (cw, ch) else (w, h), **kw)


def _sentinel_planes(fmt, w, h, extra=9, value=0xA5):
    wide = [np.full((rows, row_bytes + extra), value, np.uint8) for rows, row_bytes in rr.layout(fmt, w, h)]
    return [a[:, :a.shape[1] - extra] for a in wide], wide


def _assert_planes(got, want, what):
    assert len(got) == len(want), what
    for p, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, p, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, p, len(bad), bad[:4].tolist())


def test_the_margin_is_unlike_the_edge():
    for name in ("wide", "wide_last"):
        (w, h), _ = SIZES[name]
        for vis, coded in _content(name):
            for v, c in zip(vis, coded):
                vh, vw = v.shape
                assert np.all(np.abs(c[:vh, vw].astype(int) - v[:, -1].astype(int)) > 100)
                assert np.all(np.abs(c[vh, :vw].astype(int) - v[-1, :].astype(int)) > 100)


@pytest.mark.parametrize("name", list(SIZES))
def test_loaded_planes_in_every_format(built, name):
    """Both slots of a two-slot context, every output format and, for rgb24, every matrix and range: the host entry's bytes are
    the reference's of the VISIBLE planes, and the bytes between the destination's rows keep their sentinel."""
    (w, h), _ = SIZES[name]
    enc = _encoder(name)
    pics = _content(name)
    for slot, (vis, coded) in enumerate(pics):
        enc.test_load_recon(slot, *coded)
    for fmt, matrix, rng in FORMATS:
        for slot, (vis, coded) in enumerate(pics):
            views, wide = _sentinel_planes(fmt, w, h)
            got = enc.download_recon(slot, fmt, matrix, rng, out=views)
            _assert_planes(got, rr.convert(fmt, matrix, rng, *vis), (name, rr.NAMES[fmt], matrix, rng, slot))
            for big, v in zip(wide, views):
                assert np.all(big[:, v.shape[1]:] == 0xA5)
    # fresh arrays, names, the default format; and the slots are unchanged: the same bytes again
    vis = pics[1][0]
    _assert_planes(enc.download_recon(1), rr.convert(rr.YUV420P, 0, 0, *vis), "default")
    _assert_planes(enc.download_recon(1, "bgra", "bt601", "pc"), rr.convert(rr.BGR0, rr.BT601, rr.PC, *vis), "bgra")
    _assert_planes(enc.download_recon(0, "gbrp"), rr.convert(rr.GBRP, rr.BT709, rr.TV, *pics[0][0]), "again")
    enc.close()


def _tensor_view(shape, pad_rows=2, pad_cols=5, value=0x5A):
    """A view of `shape` (2-D or (H, W, C)) inside a larger CUDA tensor filled with a sentinel: (view, the larger tensor)."""
    big = torch.full([shape[0] + 2 * pad_rows, shape[1] + 2 * pad_cols] + list(shape[2:]), value, dtype=torch.uint8, device="cuda")
    return big[pad_rows:pad_rows + shape[0], pad_cols:pad_cols + shape[1]], big


def test_device_entry_into_tensors_and_views(built):
    """download_tensor into fresh tensors and into views of larger tensors: the host entry's bytes, and the sentinel outside
    the views unchanged."""
    from wrenc_amd import torch_source
    name = "wide"
    (w, h), _ = SIZES[name]
    enc = _encoder(name)
    vis, coded = _content(name)[0]
    enc.test_load_recon(1, *coded)
    for fmt, matrix, rng in ((rr.RGB24, "bt709", "tv"), (rr.BGR0, "bt601", "pc"), (rr.GBRP, "bt709", "pc"), (rr.YUV420P, "bt709", "tv"),
                             (rr.NV12, "bt709", "tv")):
        host = enc.download_recon(1, fmt, matrix, rng)
        _assert_planes(host, rr.convert(fmt, rr.BT601 if matrix == "bt601" else rr.BT709, rr.PC if rng == "pc" else rr.TV, *vis), rr.NAMES[fmt])
        fresh = torch_source.download_tensor(enc, 1, rr.NAMES[fmt], matrix, rng)
        if fmt in (rr.RGB24, rr.BGR0):
            c = 3 if fmt == rr.RGB24 else 4
            assert tuple(fresh.shape) == (h, w, c)
            view, big = _tensor_view((h, w, c))
            back = torch_source.download_tensor(enc, 1, fmt, matrix, rng, out=view)
            assert back is view
            got_fresh, got_view = [fresh.cpu().numpy().reshape(h, w * c)], [view.cpu().numpy().reshape(h, w * c)]
            outside = big.clone()
            outside[2:2 + h, 5:5 + w] = 0x5A
        elif fmt == rr.GBRP:
            assert tuple(fresh.shape) == (3, h, w)
            big = torch.full((3, h + 4, w + 9), 0x5A, dtype=torch.uint8, device="cuda")
            view = big[:, 2:2 + h, 4:4 + w]
            torch_source.download_tensor(enc, 1, fmt, matrix, rng, out=view)
            got_fresh, got_view = ([t[c].cpu().numpy() for c in (1, 2, 0)] for t in (fresh, view))      # R, G, B -> planes G, B, R
            outside = big.clone()
            outside[:, 2:2 + h, 4:4 + w] = 0x5A
        else:
            assert isinstance(fresh, tuple) and [tuple(t.shape) for t in fresh] == rr.layout(fmt, w, h)
            pairs = [_tensor_view(s) for s in rr.layout(fmt, w, h)]
            torch_source.download_tensor(enc, 1, fmt, out=tuple(v for v, _ in pairs))
            got_fresh, got_view = [t.cpu().numpy() for t in fresh], [v.cpu().numpy() for v, _ in pairs]
            blanked = [b.clone() for _, b in pairs]
            for o, s in zip(blanked, rr.layout(fmt, w, h)):
                o[2:2 + s[0], 5:5 + s[1]] = 0x5A
            outside = torch.cat([o.flatten() for o in blanked])
        _assert_planes(got_fresh, host, ("fresh", rr.NAMES[fmt]))
        _assert_planes(got_view, host, ("view", rr.NAMES[fmt]))
        assert int((outside != 0x5A).sum()) == 0, rr.NAMES[fmt]
    assert float(torch_source.to_float(torch.tensor([0, 51, 255], dtype=torch.uint8))[1]) == pytest.approx(0.2)
    with pytest.raises(ValueError):
        torch_source.download_tensor(enc, 1, "rgb24", out=torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        torch_source.download_tensor(enc, 1, "rgb24", out=torch.zeros(h, w, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        torch_source.download_tensor(enc, 1, "rgb24", out=torch.zeros(h, 2 * w, 3, dtype=torch.uint8, device="cuda")[:, ::2])
    enc.close()


@pytest.mark.parametrize("side", [True, False], ids=["side-stream", "default-stream"])
def test_device_entry_is_ordered_against_the_consumer_stream(built, side):
    """Work in front, a fill of the destination, the call, a clone: all on one stream, nothing synchronises in between.  The
    fill queued BEFORE the call does not survive it, and the clone queued right behind it holds the picture."""
    from wrenc_amd import torch_source
    name = "wide_last"
    (w, h), _ = SIZES[name]
    enc = _encoder(name)
    vis, coded = _content(name)[1]
    enc.test_load_recon(0, *coded)
    want = rr.convert(rr.RGB24, rr.BT709, rr.TV, *vis)[0]
    stream = torch.cuda.Stream() if side else torch.cuda.default_stream()
    dst = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(6):
            a = (a @ a).clamp_(-1, 1)          # the call is queued long before the fill runs
        dst.fill_(7)
        torch_source.download_tensor(enc, 0, "rgb24", out=dst, stream=stream.cuda_stream if side else None)
        held = dst.clone()
    torch.cuda.synchronize()
    enc.close()
    for t, what in ((held, "clone"), (dst, "destination")):
        got = t.cpu().numpy().reshape(h, 3 * w)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def test_refusals_and_states(built):
    from wrenc_amd import gpu
    name = "plain64"
    enc = _encoder(name)
    vis, coded = _content(name)[0]
    t = torch.zeros((64, 192), dtype=torch.uint8, device="cuda")

    def refused(code, call, *args, **kw):
        with pytest.raises(gpu.WrencGpuError) as e:
            call(*args, **kw)
        assert e.value.code == code, (args, e.value.code)

    refused(ESTATE, enc.download_recon, 0, "rgb24")                                      # an empty slot
    enc.upload(0, *vis)
    refused(ESTATE, enc.download_recon, 0, "rgb24")                                      # uploaded, not encoded
    refused(ESTATE, enc.download_recon_device, 0, "rgb24", [t.data_ptr()], [192])
    enc.test_load_recon(0, *coded)
    host = np.zeros((64, 192), np.uint8)
    refused(EINVAL, enc.download_recon_device, 0, "rgb24", [host.ctypes.data], [192])    # a numpy (host) pointer
    pinned = torch.from_numpy(host).pin_memory()
    refused(EINVAL, enc.download_recon_device, 0, "rgb24", [pinned.data_ptr()], [192])   # page-locked host memory is host memory
    refused(EINVAL, enc.download_recon_device, 0, "rgb24", [torch.zeros(4).data_ptr()], [192])   # a CPU tensor
    refused(EINVAL, enc.download_recon_device, 0, "rgb24", [t.data_ptr()], [191])        # a stride below the row
    refused(EINVAL, enc.download_recon_device, 0, "rgb24", [None], [192])
    refused(EINVAL, enc.download_recon_device, 0, "gbrp", [t.data_ptr(), t.data_ptr(), None], [64, 64, 64])
    refused(EINVAL, enc.download_recon_device, 2, "rgb24", [t.data_ptr()], [192])        # the context has two slots
    refused(EINVAL, enc.download_recon_device, 0, 7, [t.data_ptr()], [192])              # an unknown id
    refused(EINVAL, enc.download_recon_device, 0, "rgb24", [t.data_ptr()], [192], matrix=2)
    refused(EINVAL, enc.download_recon, -1, "rgb24")
    refused(EINVAL, enc.download_recon, 0, 0, 0, 2)
    import ctypes as C
    ptr, stride = (C.c_void_p * 3)(host.ctypes.data), (C.c_size_t * 3)(192)
    assert enc.lib.wrenc_gpu_download_recon(enc.ctx, 0, None, ptr, stride) == EINVAL     # a null format
    # none of this changed the slot: the YUV outputs read neither matrix nor range, and the context works
    _assert_planes(enc.download_recon(0, "nv12", 9, 9), rr.convert(rr.NV12, 0, 0, *vis), "nv12")
    enc.download_recon_device(0, "rgb24", [t.data_ptr()], [192])
    torch.cuda.synchronize()
    _assert_planes([t.cpu().numpy()], rr.convert(rr.RGB24, 0, 0, *vis), "device")
    enc.upload(0, *vis)                                                                  # a fresh upload into an encoded slot
    refused(ESTATE, enc.download_recon, 0, "rgb24")
    refused(ESTATE, enc.download_recon_device, 0, "rgb24", [t.data_ptr()], [192])
    enc.close()


def test_a_real_encode(built):
    """Coded 64x64, visible 50x40, QP 32, depth 2: yuv420p is the crop of download's planes, nv12 and gbrp the reference's of
    that crop, and the compact record is the same whether or not download_recon was called."""
    from wrenc_amd import gpu
    w, h = 50, 40
    y, cb, cr = rr.noise(w, h, 77)
    y = (y // 4 + np.indices((h, w))[1] * 3).astype(np.uint8)          # texture on a ramp: something to code
    records = []
    for with_recon in (False, True):
        enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2, visible=(w, h))
        enc.upload(0, y, cb, cr)
        enc.encode(0, 1)
        if with_recon:
            rec = enc.download(0, keys=("rec_y", "rec_cb", "rec_cr"))
            crop = rr.crop((rec["rec_y"], rec["rec_cb"], rec["rec_cr"]), w, h)
            _assert_planes(enc.download_recon(0, "yuv420p"), [np.ascontiguousarray(p) for p in crop], "yuv420p")
            _assert_planes(enc.download_recon(0, "nv12"), rr.convert(rr.NV12, 0, 0, *crop), "nv12")
            _assert_planes(enc.download_recon(0, "gbrp"), rr.convert(rr.GBRP, rr.BT709, rr.TV, *crop), "gbrp")
        records.append(enc.download_compact(0, 1)[0])
        assert enc.final_pass_mismatches() == 0
        enc.close()
    (m0, p0, maps0), (m1, p1, maps1) = records
    assert np.array_equal(m0, m1) and np.array_equal(p0, p1) and len(p0) > 0
    for a, b in zip(maps0.values() if isinstance(maps0, dict) else maps0, maps1.values() if isinstance(maps1, dict) else maps1):
        assert np.array_equal(a, b)


def test_round_trip_of_a_tensor(built):
    """upload_tensor of an rgb24 tensor, encode, download_tensor("rgb24"): the reference's conversion of the downloaded planes."""
    from wrenc_amd import gpu, torch_source
    w, h = 64, 64
    rgb = rgb_ref.rgb_picture("textured", w, h)
    enc = gpu.Encoder(w, h, qp=27, max_split_depth=2, source_rgb=("rgb24", "bt709", "tv"))
    src = torch.from_numpy(rgb).cuda()
    torch_source.upload_tensor(enc, 0, src)
    enc.encode(0, 1)
    back = torch_source.download_tensor(enc, 0, "rgb24")
    torch.cuda.synchronize()
    rec = enc.download(0, keys=("rec_y", "rec_cb", "rec_cr"))
    assert enc.final_pass_mismatches() == 0
    enc.close()
    got = back.cpu().numpy()
    assert got.shape == (h, w, 3)
    _assert_planes([got.reshape(h, 3 * w)], rr.convert(rr.RGB24, rr.BT709, rr.TV, rec["rec_y"], rec["rec_cb"], rec["rec_cr"]), "round trip")
    mse = float(np.mean((got.astype(np.float64) - rgb.astype(np.float64)) ** 2))
    print("round trip rgb24 64x64 QP 27: PSNR %.2f dB" % (10 * np.log10(255.0 ** 2 / mse) if mse else float("inf")))
