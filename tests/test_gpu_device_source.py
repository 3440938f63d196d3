"""Pictures that are already in device memory (include/wrenc_gpu.h: wrenc_gpu_upload_planes_device; wrenc_amd/torch_source.py):
a slot filled from torch tensors holds what the host entry leaves there, for every source kind; the upload is ordered
against the tensor's stream on both sides without a host wait; and host pointers, short strides and tensors that do not fit
are refused."""
import numpy as np
import pytest

import format_ref
import rgb_ref
import scale_ref
from window_stream import pad_planes

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("torch sees no GPU", allow_module_level=True)

pytestmark = pytest.mark.gpu

KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")
EINVAL = -1
RGB = (rgb_ref.RGB24, rgb_ref.BT709, rgb_ref.TV)


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _view(plane, pad_rows=3, pad_cols=5):
    """The numpy plane (2-D, or (H, W, C)) as a view into a larger CUDA tensor filled with another value: its row stride is
    not the packed one, and it starts inside the tensor."""
    t = torch.from_numpy(np.ascontiguousarray(plane).view(np.int16) if plane.dtype == np.uint16 else np.ascontiguousarray(plane))
    shape = list(t.shape)
    big = torch.full([shape[0] + 2 * pad_rows, shape[1] + 2 * pad_cols] + shape[2:], 0x5A, dtype=t.dtype, device="cuda")
    v = big[pad_rows:pad_rows + shape[0], pad_cols:pad_cols + shape[1]]
    v.copy_(t.cuda())
    assert v.stride(0) != t.stride(0) and v.data_ptr() != big.data_ptr()
    return v


def _both(make, host_upload, tensors):
    """The originals of slot 1 of two fresh contexts: one filled by the host entry, one by upload_tensor."""
    from wrenc_amd import torch_source
    out = []
    for device in (False, True):
        enc = make()
        if device:
            torch_source.upload_tensor(enc, 1, tensors)
        else:
            host_upload(enc)
        out.append(enc.download_originals(1))
        enc.close()
    return out


def test_format_0(built):
    from wrenc_amd import gpu
    visible, coded = (34, 30), (64, 32)
    pic = scale_ref.picture("textured", *visible)
    host, dev = _both(lambda: gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible),
                      lambda enc: enc.upload(1, *pic), tuple(_view(p) for p in pic))
    assert _same(host, pad_planes(pic, *coded)) and _same(dev, host)


def test_format_0_with_a_source_size(built):
    from wrenc_amd import gpu
    source, visible, coded = (70, 50), (34, 30), (64, 32)
    pic = scale_ref.picture("textured", *source)
    host, dev = _both(lambda: gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible, source=source),
                      lambda enc: enc.upload(1, *pic), tuple(_view(p) for p in pic))
    assert _same(host, pad_planes(scale_ref.scale_planes(pic, *visible), *coded)) and _same(dev, host)


def test_p010le(built):
    from wrenc_amd import gpu
    fmt, visible, coded = format_ref.P010LE, (70, 50), (96, 64)
    raw = format_ref.picture("textured", fmt, *visible)
    host, dev = _both(lambda: gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible, source_format=fmt),
                      lambda enc: enc.upload_planes(1, raw), tuple(_view(p) for p in raw))
    assert _same(host, pad_planes(format_ref.convert(fmt, raw), *coded)) and _same(dev, host)


@pytest.mark.parametrize("lay", [rgb_ref.RGB24, rgb_ref.GBRP], ids=["rgb24", "gbrp"])
def test_rgb(built, lay):
    from wrenc_amd import gpu
    source, visible, coded = (lay, rgb_ref.BT709, rgb_ref.TV), (70, 50), (96, 64)
    rgb = rgb_ref.rgb_picture("textured", *visible)
    raw = rgb_ref.pack(lay, rgb)
    if lay == rgb_ref.GBRP:
        # a model's CHW image, (3, H, W) in R, G, B order, inside a larger one: the samples of a row packed, the rows not
        big = torch.full((3, visible[1] + 4, visible[0] + 9), 0x5A, dtype=torch.uint8, device="cuda")
        t = big[:, 2:2 + visible[1], 4:4 + visible[0]]
        t.copy_(torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1))).cuda())
        assert t.shape == (3, visible[1], visible[0]) and t.stride(2) == 1 and t.stride(1) == visible[0] + 9
    else:
        t = _view(rgb)
    host, dev = _both(lambda: gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible, source_rgb=source),
                      lambda enc: enc.upload_rgb(1, raw if len(raw) > 1 else raw[0]), t)
    assert _same(host, pad_planes(rgb_ref.convert(*source, raw), *coded)) and _same(dev, host)


_big = []     # the ordering tests' picture and its conversion, made once


def _ordering(stream):
    """Work in front, the picture written by copy_(), the upload, the picture zeroed: all on one stream, nothing synchronises
    in between.  The slot must hold the conversion of `src`."""
    from wrenc_amd import gpu, torch_source
    size = (1920, 1088)
    if not _big:
        rgb = rgb_ref.rgb_picture("noise", *size)
        _big.extend([rgb, rgb_ref.convert(*RGB, rgb_ref.pack(rgb_ref.RGB24, rgb))])
    rgb, want = _big
    enc = gpu.Encoder(size[0], size[1], qp=32, max_split_depth=2, source_rgb=RGB)
    src = torch.from_numpy(rgb).cuda()
    t = torch.zeros_like(src)
    a = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.default_stream()):
        for _ in range(6):
            a = (a @ a).clamp_(-1, 1)         # a few milliseconds each: the upload is queued long before `t` is written
        t.copy_(src)
        torch_source.upload_tensor(enc, 0, t, stream=stream.cuda_stream if stream is not None else None)
        t.zero_()
    got = enc.download_originals(0)
    enc.close()
    torch.cuda.synchronize()
    assert int(t.max()) == 0
    for p in range(3):
        bad = np.argwhere(got[p] != want[p])
        assert bad.size == 0, (p, len(bad), bad[:4].tolist())


def test_ordering_on_a_side_stream(built):
    _ordering(torch.cuda.Stream())


def test_ordering_on_the_default_stream(built):
    _ordering(None)


def test_encode_after_a_device_upload(built):
    """64x64, depth 3: the record of a picture that came from a tensor is that of the same picture from host memory."""
    from wrenc_amd import gpu, torch_source
    rgb = rgb_ref.rgb_picture("textured", 64, 64)
    records = []
    for device in (False, True):
        enc = gpu.Encoder(64, 64, qp=32, max_split_depth=3, source_rgb=RGB)
        if device:
            torch_source.upload_tensor(enc, 0, torch.from_numpy(rgb).cuda())
        else:
            enc.upload_rgb(0, rgb.reshape(64, 192))
        enc.encode(0, 1)
        records.append(enc.download(0))
        assert enc.final_pass_mismatches() == 0
        enc.close()
    for k in KEYS:
        assert np.array_equal(records[0][k], records[1][k]), k
    assert any(np.any(records[0][k] != 0) for k in ("lev_y", "lev_cb", "lev_cr"))


def test_refusals(built):
    from wrenc_amd import gpu, torch_source
    rgb = rgb_ref.rgb_picture("textured", 64, 64)
    conv = rgb_ref.convert(*RGB, rgb_ref.pack(rgb_ref.RGB24, rgb))
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2, source_rgb=RGB)
    t = torch.from_numpy(rgb).cuda()

    def refused(code, *args):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.upload_device(*args)
        assert e.value.code == code, (args, e.value.code)

    host = np.ascontiguousarray(rgb.reshape(64, 192))
    refused(EINVAL, 0, [host.ctypes.data], [192])                       # a numpy (host) pointer
    pinned = torch.from_numpy(host).pin_memory()
    refused(EINVAL, 0, [pinned.data_ptr()], [192])                       # page-locked host memory is host memory
    refused(EINVAL, 0, [t.data_ptr()], [191])                            # a short stride
    refused(EINVAL, 0, [None], [192])
    refused(EINVAL, 1, [t.data_ptr()], [192])                            # the context has one slot
    for bad in (torch.from_numpy(rgb),                                   # a CPU tensor
                t[:, :, :2], t[:32], t.permute(2, 0, 1),                 # shapes that are not (64, 64, 3)
                torch.zeros(64, 64, 4, dtype=torch.uint8, device="cuda"),
                t.float(), torch.zeros(64, 128, 3, dtype=torch.uint8, device="cuda")[:, ::2],   # samples of a row not packed
                (t, t, t)):
        with pytest.raises(ValueError):
            torch_source.upload_tensor(enc, 0, bad)
    # none of this was an upload, and the context works
    enc.set_source_rgb("rgb24", "bt709", "tv")
    torch_source.upload_tensor(enc, 0, t)
    assert _same(enc.download_originals(0), conv)
    enc.close()
    # a YUV context takes a tuple of planes, of its own sample size
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2)
    y = torch.zeros(64, 64, dtype=torch.uint8, device="cuda")
    c = torch.zeros(32, 32, dtype=torch.uint8, device="cuda")
    for bad in (y, (y, c), (y, c, c.short()), (y, c, c[:16]), (y, c, c.cpu())):
        with pytest.raises(ValueError):
            torch_source.upload_tensor(enc, 0, bad)
    with pytest.raises(gpu.WrencGpuError) as e:                          # yuv420p: the chroma planes share one stride
        torch_source.upload_tensor(enc, 0, (y, c, torch.zeros(32, 48, dtype=torch.uint8, device="cuda")[:, :32]))
    assert e.value.code == EINVAL
    torch_source.upload_tensor(enc, 0, (y, c, c))
    assert _same(enc.download_originals(0), tuple(np.zeros(s, np.uint8) for s in ((64, 64), (32, 32), (32, 32))))
    enc.close()
