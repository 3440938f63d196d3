"""Pictures that are torch tensors on the GPU, into an encoder and the reconstruction back out of it without a trip over the bus
(wrenc_gpu_upload_planes_device, wrenc_gpu_download_recon_device).

torch is imported here and nowhere else in the package: wrenc_amd.gpu stays a ctypes binding of the C ABI.

    enc = gpu.Encoder(3840, 2176, visible=(3840, 2160), source_rgb=("rgb24", "bt709", "tv"), n_slots=2)
    frame = to_uint8(model(x))              # (H, W, 3), uint8, on the encoder's device
    upload_tensor(enc, 0, frame)            # queued behind the work that made `frame`, on torch's current stream
    frame.zero_()                           # ... and this behind the upload's copies: nothing synchronises

The library COPIES the planes (device to device) and orders the copies against `stream` on both sides, so the tensor may be
overwritten or freed on that stream right after the call (include/wrenc_gpu.h).  Work on other streams is the caller's to
order, as always with torch.
"""
import torch

from . import gpu

_PACKED = {0: 3, 1: 3, 2: 4, 3: 4}      # layout id (include/wrenc_rgb.h) -> channels of the (H, W, C) tensor
_GBRP = 4


def to_uint8(t):
    """A float tensor in [0, 1] -> uint8 by (t.clamp(0, 1) * 255 + 0.5).to(torch.uint8).  This is torch's floating-point
    arithmetic: it lies outside the bit-exact definition of include/wrenc_rgb.h, which starts at the bytes."""
    return (t.clamp(0, 1) * 255 + 0.5).to(torch.uint8)


def _plane(t, rows, row_bytes, device, what):
    """(address, row stride in bytes) of a 2-D or (H, W, C) uint8 view whose rows are `row_bytes` contiguous bytes."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s is not a tensor" % what)
    if t.dtype not in (torch.uint8, torch.int16, torch.uint16) or not t.is_cuda:
        raise ValueError("%s must be an integer tensor on the GPU, not %s on %s" % (what, t.dtype, t.device))
    if t.device.index != device:
        raise ValueError("%s is on %s, the encoder on device %d" % (what, t.device, device))
    size = t.element_size()
    inner = 1
    for d in range(t.dim() - 1, 0, -1):          # every axis but the rows is packed
        if t.shape[d] != 1 and t.stride(d) != inner:
            raise ValueError("%s: the samples of a row must be contiguous (strides %s)" % (what, tuple(t.stride())))
        inner *= t.shape[d]
    if t.shape[0] != rows or inner * size != row_bytes:
        raise ValueError("%s has shape %s: the encoder's source takes %d rows of %d bytes" % (what, tuple(t.shape), rows, row_bytes))
    if t.stride(0) * size < row_bytes:
        raise ValueError("%s: rows overlap (strides %s)" % (what, tuple(t.stride())))
    return t.data_ptr(), t.stride(0) * size


def upload_tensor(enc, slot, t, stream=None):
    """Upload tensor(s) on the encoder's device into slot `slot`, by the encoder's source kind at its source size:
        rgb24 / bgr24   one (H, W, 3) uint8 tensor
        rgb0 / bgr0     one (H, W, 4) uint8 tensor
        gbrp            one (3, H, W) uint8 tensor in R, G, B order -- a model's CHW image; the planes go to the library
                        in the layout's order G, B, R: t[1], t[2], t[0]
        a YUV format    a tuple of its plane tensors (rows x samples; uint8, or int16 / uint16 for the 16-bit formats)
    Row strides come from the tensors, so views into larger tensors work; the samples of a row must be packed.
    stream: a hipStream_t as an integer; None takes torch.cuda.current_stream(t.device).cuda_stream.
    ValueError for a tensor that does not fit (shape, strides, dtype, a CPU tensor, another device); gpu.WrencGpuError for
    what the library refuses."""
    layout, _, _ = enc.source_rgb()
    w, h = enc.source_size()
    device = enc.cfg.device
    first = t[0] if isinstance(t, (tuple, list)) else t
    if layout >= 0:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError("an RGB source takes one uint8 tensor")
        if layout == _GBRP:
            if t.dim() != 3 or tuple(t.shape) != (3, h, w):
                raise ValueError("gbrp takes a (3, %d, %d) tensor in R, G, B order, not %s" % (h, w, tuple(t.shape)))
            planes = [_plane(t[c], h, w, device, "plane %d" % c) for c in (1, 2, 0)]
        else:
            c = _PACKED[layout]
            if t.dim() != 3 or tuple(t.shape) != (h, w, c):
                raise ValueError("%s takes a (%d, %d, %d) tensor, not %s" % (gpu.rgb_name(layout), h, w, c, tuple(t.shape)))
            planes = [_plane(t, h, w * c, device, "the picture")]
    else:
        if not isinstance(t, (tuple, list)):
            raise ValueError("a YUV source takes a tuple of plane tensors")
        lay = gpu.format_layout(enc.source_format(), w, h)
        if len(t) != lay["n_planes"]:
            raise ValueError("%s has %d planes, not %d" % (gpu.format_name(enc.source_format()), lay["n_planes"], len(t)))
        for p in t:
            if isinstance(p, torch.Tensor) and p.element_size() != lay["bytes_per_sample"]:
                raise ValueError("%s takes samples of %d bytes, not %s" % (gpu.format_name(enc.source_format()), lay["bytes_per_sample"], p.dtype))
        planes = [_plane(p, lay["rows"][i], lay["row_bytes"][i], device, "plane %d" % i) for i, p in enumerate(t)]
    if stream is None:
        stream = torch.cuda.current_stream(first.device).cuda_stream
    enc.upload_device(slot, [p for p, _ in planes], [s for _, s in planes], stream)


def to_float(t):
    """A uint8 tensor -> float in [0, 1] by t.float() / 255: the inverse of to_uint8 up to torch's floating-point arithmetic."""
    return t.float() / 255


def download_tensor(enc, slot, fmt, matrix="bt709", rng="tv", out=None, stream=None):
    """The reconstruction of encoded slot `slot` as tensor(s) on the encoder's device, at its visible size, without a trip
    over the bus (wrenc_gpu_download_recon_device; include/wrenc_recon.h defines the picture).  The shapes mirror
    upload_tensor:
        rgb24 / bgr24   one (H, W, 3) uint8 tensor
        rgb0 / bgr0     one (H, W, 4) uint8 tensor (the fourth byte is 255)
        gbrp            one (3, H, W) uint8 tensor in R, G, B order -- a model's CHW image
        yuv420p / nv12  a tuple of plane tensors (rows x bytes)
    out: the tensor(s) to fill instead of fresh ones -- views into larger tensors work, the samples of a row must be packed;
    nothing outside the views is written.  stream: a hipStream_t as an integer; None takes torch.cuda.current_stream of the
    encoder's device.  The copies run behind what that stream has queued so far and what it queues next runs behind them:
    nothing synchronises.  ValueError for an `out` that does not fit; gpu.WrencGpuError for what the library refuses."""
    fid = gpu.recon_from_name(fmt) if isinstance(fmt, str) else int(fmt)
    w, h = enc.visible_size()
    device = enc.cfg.device
    dev = torch.device("cuda", device)
    lay = gpu.recon_layout(fid, w, h)
    if fid in _PACKED:
        c = _PACKED[fid]
        if out is None:
            out = torch.empty((h, w, c), dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 3 or tuple(out.shape) != (h, w, c):
            raise ValueError("%s fills a (%d, %d, %d) uint8 tensor" % (gpu.recon_name(fid), h, w, c))
        planes = [_plane(out, h, w * c, device, "the picture")]
    elif fid == _GBRP:
        if out is None:
            out = torch.empty((3, h, w), dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 3 or tuple(out.shape) != (3, h, w):
            raise ValueError("gbrp fills a (3, %d, %d) uint8 tensor in R, G, B order" % (h, w))
        planes = [_plane(out[c], h, w, device, "plane %d" % c) for c in (1, 2, 0)]
    else:
        shapes = [(lay["rows"][p], lay["row_bytes"][p]) for p in range(lay["n_planes"])]
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.uint8, device=dev) for s in shapes)
        elif not isinstance(out, (tuple, list)) or len(out) != len(shapes) or any(not isinstance(p, torch.Tensor) or p.dtype != torch.uint8 for p in out):
            raise ValueError("%s fills a tuple of %d uint8 plane tensors" % (gpu.recon_name(fid), len(shapes)))
        planes = [_plane(p, s[0], s[1], device, "plane %d" % i) for i, (p, s) in enumerate(zip(out, shapes))]
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    enc.download_recon_device(slot, fid, [p for p, _ in planes], [s for _, s in planes], stream, matrix=matrix, rng=rng)
    return out
