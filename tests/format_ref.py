"""Reference side of the source-format tests: the formats and the conversion of include/wrenc_format.h restated in numpy,
and the pictures the tests share.  A picture is first a set of SAMPLE arrays (y, cb, cr) in the format's own depth (0..255
or 0..1023) and chroma height (4:2:2: as many chroma rows as luma rows); pack() lays them out as the format's raw planes,
with junk in every bit the definition ignores or saturates; convert() is the definition."""
import numpy as np

import scale_ref

NAMES = ("yuv420p", "nv12", "yuv420p10le", "p010le", "yuv422p", "yuv422p10le")   # the name of format id i
YUV420P, NV12, YUV420P10LE, P010LE, YUV422P, YUV422P10LE = range(6)
FORMATS = (1, 2, 3, 4, 5)                        # what the device converts (0 is the plain upload)
PICTURES = ("all10", "textured", "noise", "zeros", "ones")


def is16(fmt):
    return fmt in (YUV420P10LE, P010LE, YUV422P10LE)


def pairs(fmt):
    return fmt in (NV12, P010LE)


def is422(fmt):
    return fmt in (YUV422P, YUV422P10LE)


def top(fmt):
    """The largest sample value."""
    return 1023 if is16(fmt) else 255


def layout(fmt, w, h):
    """wrenc_gpu_format_layout restated: the dict gpu.format_layout returns."""
    assert 0 <= fmt < 6 and w >= 16 and h >= 16 and w % 2 == 0 and h % 2 == 0
    bps = 2 if is16(fmt) else 1
    crows = h if is422(fmt) else h // 2
    row_bytes = [w * bps, w * bps] if pairs(fmt) else [w * bps, w // 2 * bps, w // 2 * bps]
    rows = [h] + [crows] * (len(row_bytes) - 1)
    offset = [sum(r * n for r, n in zip(row_bytes[:p], rows[:p])) for p in range(len(rows))]
    return {"n_planes": len(rows), "bytes_per_sample": bps, "row_bytes": row_bytes, "rows": rows, "offset": offset,
            "frame_bytes": sum(r * n for r, n in zip(row_bytes, rows))}


# ---- the definition ----

def _s10(fmt, v):
    v = v.astype(np.int64)
    return v >> 6 if fmt == P010LE else np.minimum(v, 1023)


def _sample(fmt, v):
    """A plane at full chroma resolution: words (or bytes) -> int64 0..255."""
    return np.minimum((_s10(fmt, v) + 2) >> 2, 255) if is16(fmt) else v.astype(np.int64)


def _halve(fmt, c):
    """A 4:2:2 chroma plane -> 4:2:0: row j from rows 2j and 2j + 1."""
    a, b = c[0::2], c[1::2]
    if is16(fmt):
        return np.minimum((_s10(fmt, a) + _s10(fmt, b) + 4) >> 3, 255)
    return (a.astype(np.int64) + b.astype(np.int64) + 1) >> 1


def convert(fmt, planes_raw):
    """The raw planes of one picture (as pack() makes them) -> (y, cb, cr) as uint8, 4:2:0."""
    planes_raw = [np.asarray(p) for p in planes_raw]
    assert all(p.dtype == (np.uint16 if is16(fmt) else np.uint8) for p in planes_raw)
    if fmt == YUV420P:
        out = planes_raw
    elif pairs(fmt):
        y, c = planes_raw
        out = (_sample(fmt, y), _sample(fmt, c[:, 0::2]), _sample(fmt, c[:, 1::2]))
    elif is422(fmt):
        out = (_sample(fmt, planes_raw[0]), _halve(fmt, planes_raw[1]), _halve(fmt, planes_raw[2]))
    else:
        out = tuple(_sample(fmt, p) for p in planes_raw)
    assert all(0 <= int(p.min()) and int(p.max()) <= 255 for p in out)
    return tuple(np.ascontiguousarray(p, dtype=np.uint8) for p in out)


# ---- raw planes ----

def pack(fmt, y, cb, cr, junk_rng):
    """Sample arrays in the format's depth -> its raw planes (a list of 2 or 3 arrays, uint8 or little-endian uint16 in
    native order).  Bits the definition does not read are random: the low six of every p010le word; and of the low-bit
    16-bit formats about one word in sixteen is replaced by one above 1023, which the definition saturates."""
    planes = [np.asarray(p).astype(np.int64) for p in (y, cb, cr)]
    assert all(0 <= int(p.min()) and int(p.max()) <= top(fmt) for p in planes)
    if pairs(fmt):
        c = np.empty((planes[1].shape[0], 2 * planes[1].shape[1]), np.int64)
        c[:, 0::2], c[:, 1::2] = planes[1], planes[2]
        planes = [planes[0], c]
    if not is16(fmt):
        return [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
    out = []
    for p in planes:
        if fmt == P010LE:
            p = (p << 6) | junk_rng.integers(0, 64, p.shape)
        else:
            p = np.where(junk_rng.integers(0, 16, p.shape) == 0, junk_rng.integers(1024, 65536, p.shape), p)
        out.append(np.ascontiguousarray(p, dtype=np.uint16))
    return out


def raw_bytes(planes_raw):
    """The planes as they lie in a raw file: tightly packed, 16-bit words little-endian."""
    return b"".join(np.ascontiguousarray(p).astype(p.dtype.newbyteorder("<")).tobytes() for p in planes_raw)


def strided(planes_raw, extra_bytes):
    """Views of the planes inside wider arrays filled with another value: rows extra_bytes[p] further apart than they are
    long (an even number for a 16-bit format)."""
    out = []
    for p, e in zip(planes_raw, extra_bytes):
        assert e % p.itemsize == 0
        wide = np.full((p.shape[0], p.shape[1] + e // p.itemsize), 0xA5A5 & (0xFFFF if p.itemsize == 2 else 0xFF), p.dtype)
        wide[:, :p.shape[1]] = p
        out.append(wide[:, :p.shape[1]])
    return out


# ---- pictures ----

def _cycle(fmt, n, start=0):
    """n values that walk through the whole sample range, 0 first and the largest value fourth: a plane of at least
    top + 1 samples holds every value."""
    m = top(fmt) + 1
    step = {256: 85, 1024: 341}[m]            # 3 * step = top, gcd(step, m) = 1
    return (np.arange(start, start + n, dtype=np.int64) * step) % m


def samples(name, fmt, w, h, seed=11):
    """(y, cb, cr) sample arrays of picture `name` for a w x h frame of format fmt, in its depth and chroma height."""
    t, ch, cw = top(fmt), (h if is422(fmt) else h // 2), w // 2
    if name in ("zeros", "ones"):
        v = 0 if name == "zeros" else t
        return np.full((h, w), v, np.int64), np.full((ch, cw), v, np.int64), np.full((ch, cw), v, np.int64)
    if name == "all10":
        y = _cycle(fmt, w * h).reshape(h, w)
        if not is422(fmt):
            cb = _cycle(fmt, ch * cw).reshape(ch, cw)
            return y, cb, t - cb
        # vertical pair k = (a, b): a walks the range, b = a or a + 1: both parities of a + b, (0, 0) at k = 0, (top, top) at k = 3
        k = np.arange(ch // 2 * cw, dtype=np.int64).reshape(ch // 2, cw)
        a = _cycle(fmt, k.size).reshape(k.shape)
        b = np.minimum(a + (k % 3 == 1), t)
        cb = np.empty((ch, cw), np.int64)
        cb[0::2], cb[1::2] = a, b
        cr = np.empty((ch, cw), np.int64)
        cr[0::2], cr[1::2] = t - a, t - b
        return y, cb, cr
    assert name in ("textured", "noise")
    if is422(fmt):
        tall = scale_ref.picture(name, w, 2 * h)
        pic = (tall[0][:h], tall[1], tall[2])
    else:
        pic = scale_ref.picture(name, w, h)
    pic = tuple(p.astype(np.int64) for p in pic)
    if is16(fmt):
        rng = np.random.default_rng(seed)
        pic = tuple((p << 2) | rng.integers(0, 4, p.shape) for p in pic)
    return pic


def invert(fmt, pic):
    return tuple(top(fmt) - p for p in pic)


def picture(name, fmt, w, h, inverted=False, seed=11):
    """The raw planes of picture `name`."""
    pic = samples(name, fmt, w, h, seed)
    if inverted:
        pic = invert(fmt, pic)
    return pack(fmt, *pic, np.random.default_rng(seed + 1000))
