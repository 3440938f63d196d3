"""Synthetic picture content shared by the parity tests: one kind per tool of the search (see
test_gpu_content.py), and what a record says about the tool a kind is there for."""
import numpy as np

# intraPredAngle of the modes 50 .. 66 (and, mirrored, 18 .. 2; negated, 50 .. 34 and 18 .. 34) in H.266
_ANGLES = (0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32)
STRIPES_SHARE = 0.45     # the oracle gives 0.50 (stripes70) .. 0.85 over test_gpu_content.CASES
CCLM_SHARE = 0.70        # the oracle gives 0.75 .. 0.96


def stripe_modes(deg):
    """The angular mode(s) along which `stripesDEG` content is constant: the picture is a function of x cos a + y sin a, so
    it is constant along (-sin a, cos a) -- (-tan a, 1) for a vertical mode of intraPredAngle 32 tan a, (1, -cot a) for a
    horizontal one.  45 degrees is both mode 2 and mode 66."""
    a = (deg + 90.0) % 180.0 - 90.0                     # -90 .. 90
    if abs(a) <= 45.0:
        t = 32.0 * np.tan(a * np.pi / 180.0)
        k = int(np.argmin([abs(abs(t) - v) for v in _ANGLES]))
        modes = {50 + k if t >= 0 else 50 - k}
    else:
        t = 32.0 / np.tan(a * np.pi / 180.0)
        k = int(np.argmin([abs(abs(t) - v) for v in _ANGLES]))
        modes = {18 - k if t >= 0 else 18 + k}
    if modes & {2, 66}:
        modes = {2, 66}
    return modes


def _cu_tops(rec):
    cu = rec["cu_log2_size"]
    yy, xx = np.mgrid[0:cu.shape[0], 0:cu.shape[1]]
    n4 = 1 << (cu.astype(np.int64) - 2)
    return (yy % n4 == 0) & (xx % n4 == 0)


def stripes_share(deg, rec):
    """The share of the record's CUs whose luma mode lies within +-3 of the stripes' direction."""
    modes = rec["luma_mode"][_cu_tops(rec)].astype(np.int64)
    near = np.zeros(modes.shape, bool)
    for m in stripe_modes(deg):
        near |= (np.abs(modes - m) <= 3) & (modes >= 2)
    return float(near.mean())


def cclm_share(rec):
    """The share of the record's chroma blocks (one per CU of 8x8 and above, one per split 8x8) coded with a CCLM mode."""
    cu8 = np.maximum(rec["cu_log2_size"][::2, ::2].astype(np.int64), 3)
    yy, xx = np.mgrid[0:cu8.shape[0], 0:cu8.shape[1]]
    n8 = 1 << (cu8 - 3)
    tops = (yy % n8 == 0) & (xx % n8 == 0)
    return float((rec["chroma_mode"][tops] >= 81).mean())


def content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "flat":
        y = np.full((h, w), 93)
        cb, cr = np.full((h // 2, w // 2), 140), np.full((h // 2, w // 2), 77)
    elif kind == "ramp":
        y = (xx * 2 + yy * 3) % 256
        cb, cr = (xx[::2, ::2] + 60) % 256, (yy[::2, ::2] * 2 + 30) % 256
    elif kind.startswith("stripes"):
        ang = float(kind[7:]) * np.pi / 180.0
        ph = xx * np.cos(ang) + yy * np.sin(ang)
        y = 128 + 90 * np.sign(np.sin(ph * 0.55))
        cb = 128 + 40 * np.sign(np.sin(ph[::2, ::2] * 0.55 + 1.0))
        cr = 128 - 50 * np.sign(np.sin(ph[::2, ::2] * 0.35))
    elif kind == "checker":
        y = 40 + 170 * (((xx // 3) + (yy // 5)) & 1)
        cb = 100 + 60 * (((xx[::2, ::2] // 4) + (yy[::2, ::2] // 2)) & 1)
        cr = 200 - cb // 2
    elif kind == "noise":
        y = rng.integers(0, 256, (h, w))
        cb, cr = rng.integers(0, 256, (h // 2, w // 2)), rng.integers(0, 256, (h // 2, w // 2))
    elif kind == "cclm":     # chroma is an affine function of the (sub-sampled) luma plus a little noise
        y = (128 + 70 * np.sin(xx * 0.21) * np.cos(yy * 0.13) + rng.integers(-6, 7, (h, w))).clip(0, 255)
        ys = y.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
        cb = (0.6 * ys + 40 + rng.integers(-2, 3, ys.shape)).clip(0, 255)
        cr = (220 - 0.7 * ys + rng.integers(-2, 3, ys.shape)).clip(0, 255)
    elif kind == "extremes":  # black / white blocks: clamps in prediction and reconstruction
        y = 255 * (((xx // 16) + (yy // 8)) & 1)
        cb, cr = 255 * ((xx[::2, ::2] // 8) & 1), 255 * ((yy[::2, ::2] // 4) & 1)
    else:
        raise ValueError(kind)
    return (np.ascontiguousarray(y, dtype=np.uint8), np.ascontiguousarray(cb, dtype=np.uint8),
            np.ascontiguousarray(cr, dtype=np.uint8))
