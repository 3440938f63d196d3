"""Reference side of the RGB-source tests: the layouts and the conversion of include/wrenc_rgb.h restated in numpy, and the
pictures the tests share.  A picture is first an (h, w, 3) uint8 array in R, G, B order; pack() lays it out as a layout's raw
planes (junk in the X byte of rgb0 / bgr0, which the definition ignores); convert() is the definition."""
import numpy as np

NAMES = ("rgb24", "bgr24", "rgb0", "bgr0", "gbrp")            # the name of layout id i
RGB24, BGR24, RGB0, BGR0, GBRP = range(5)
LAYOUTS = tuple(range(5))
ALIASES = {"rgba": RGB0, "bgra": BGR0}
MATRICES = ("bt709", "bt601")
RANGES = ("tv", "pc")
BT709, BT601 = 0, 1
TV, PC = 0, 1
COMBOS = [(m, r) for m in (BT709, BT601) for r in (TV, PC)]
K = {BT709: (0.2126, 0.0722), BT601: (0.299, 0.114)}          # Kr, Kb
PICTURES = ("noise", "corners", "gradient")

# yr yg yb | br bg bb | rr rg rb | yoff, as the header's table words them
TABLE = {
    (BT709, TV): [2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660, 16],
    (BT709, PC): [3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751, 0],
    (BT601, TV): [4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170, 16],
    (BT601, PC): [4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332, 0],
}
# (Y, Cb, Cr) of flat pictures
ANCHORS = {
    (BT709, TV): {"black": (16, 128, 128), "white": (235, 128, 128), "red": (63, 102, 240), "green": (173, 42, 26), "blue": (32, 240, 118)},
    (BT709, PC): {"black": (0, 128, 128), "white": (255, 128, 128), "red": (54, 99, 255), "green": (182, 30, 12), "blue": (18, 255, 116)},
    (BT601, TV): {"black": (16, 128, 128), "white": (235, 128, 128), "red": (81, 90, 240), "green": (145, 54, 34), "blue": (41, 240, 110)},
    (BT601, PC): {"black": (0, 128, 128), "white": (255, 128, 128), "red": (76, 85, 255), "green": (150, 44, 21), "blue": (29, 255, 107)},
}
COLOURS = {"black": (0, 0, 0), "white": (255, 255, 255), "red": (255, 0, 0), "green": (0, 255, 0), "blue": (0, 0, 255)}


def scales(rng):
    """(sy, sc): what luma and chroma are scaled by."""
    return (219 / 255, 224 / 255) if rng == TV else (1.0, 1.0)


def derive(matrix, rng):
    """The ten numbers from Kr, Kb and the range, by the header's derivation."""
    kr, kb = K[matrix]
    sy, sc = scales(rng)

    def rnd(x):
        return int(np.floor(x + 0.5))

    yr, yb = rnd(kr * sy * 2 ** 14), rnd(kb * sy * 2 ** 14)
    yg = rnd(sy * 2 ** 14) - yr - yb
    half = rnd(sc * 2 ** 13)
    br = rnd(-kr / (2 * (1 - kb)) * sc * 2 ** 14)
    rb = rnd(-kb / (2 * (1 - kr)) * sc * 2 ** 14)
    return [yr, yg, yb, br, -half - br, half, half, -half - rb, rb, 16 if rng == TV else 0]


def pixel_bytes(layout):
    return 1 if layout == GBRP else 4 if layout in (RGB0, BGR0) else 3


def layout(lay, w, h):
    """wrenc_gpu_rgb_layout restated: the dict gpu.rgb_layout returns."""
    assert 0 <= lay < 5 and w >= 16 and h >= 16 and w % 2 == 0 and h % 2 == 0
    n = 3 if lay == GBRP else 1
    row = w * pixel_bytes(lay)
    return {"n_planes": n, "bytes_per_sample": 1, "row_bytes": [row] * n, "rows": [h] * n, "offset": [p * row * h for p in range(n)],
            "frame_bytes": n * row * h}


# ---- the definition ----

def unpack(lay, planes):
    """Raw planes -> (R, G, B) as int64 arrays of h x w."""
    planes = [np.asarray(p) for p in planes]
    assert all(p.dtype == np.uint8 and p.ndim == 2 for p in planes)
    if lay == GBRP:
        g, b, r = (p.astype(np.int64) for p in planes)
        return r, g, b
    n = pixel_bytes(lay)
    p = planes[0].astype(np.int64)
    c = [p[:, k::n] for k in range(3)]
    return (c[2], c[1], c[0]) if lay in (BGR24, BGR0) else (c[0], c[1], c[2])


def luma(k, r, g, b):
    return np.clip((k[0] * r + k[1] * g + k[2] * b + (k[9] << 14) + (1 << 13)) >> 14, 0, 255)


def chroma(k3, sr, sg, sb):
    return np.clip((k3[0] * sr + k3[1] * sg + k3[2] * sb + (128 << 16) + (1 << 15)) >> 16, 0, 255)


def convert(lay, matrix, rng, planes):
    """The raw planes of one picture -> (y, cb, cr) as uint8, 4:2:0."""
    k = TABLE[(matrix, rng)]
    r, g, b = unpack(lay, planes)
    s = [c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] for c in (r, g, b)]
    acc = [k[0] * r + k[1] * g + k[2] * b + (k[9] << 14) + (1 << 13), k[3] * s[0] + k[4] * s[1] + k[5] * s[2] + (128 << 16) + (1 << 15),
           k[6] * s[0] + k[7] * s[1] + k[8] * s[2] + (128 << 16) + (1 << 15)]
    assert all(0 <= int(a.min()) and int(a.max()) < 2 ** 31 for a in acc)      # 32-bit, never negative
    out = (luma(k, r, g, b), chroma(k[3:6], *s), chroma(k[6:9], *s))
    return tuple(np.ascontiguousarray(p, dtype=np.uint8) for p in out)


# ---- raw planes ----

def pack(lay, rgb, junk_rng=None):
    """(h, w, 3) R, G, B -> the layout's raw planes, a list of 1 or 3 uint8 arrays; the X byte is random."""
    rgb = np.asarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    if lay == GBRP:
        return [np.ascontiguousarray(rgb[:, :, c]) for c in (1, 2, 0)]
    order = (2, 1, 0) if lay in (BGR24, BGR0) else (0, 1, 2)
    n = pixel_bytes(lay)
    out = np.empty((h, w, n), np.uint8)
    for k, c in enumerate(order):
        out[:, :, k] = rgb[:, :, c]
    if n == 4:
        out[:, :, 3] = (junk_rng or np.random.default_rng(77)).integers(0, 256, (h, w))
    return [out.reshape(h, w * n)]


def raw_bytes(planes):
    """The planes as they lie in a raw file."""
    return b"".join(np.ascontiguousarray(p).tobytes() for p in planes)


def strided(planes, extra_bytes):
    """Views of the planes inside wider arrays filled with another value."""
    out = []
    for p, e in zip(planes, extra_bytes):
        wide = np.full((p.shape[0], p.shape[1] + e), 0xA5, np.uint8)
        wide[:, :p.shape[1]] = p
        out.append(wide[:, :p.shape[1]])
    return out


# ---- pictures ----

def rgb_picture(name, w, h, seed=23, inverted=False):
    """(h, w, 3) uint8, R, G, B."""
    if name in COLOURS:
        pic = np.empty((h, w, 3), np.uint8)
        pic[:] = COLOURS[name]
    elif name == "noise":
        pic = np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    elif name == "corners":
        # every sample is 0 or 255.  Per channel the four positions of a 2x2 block take one of four patterns -- none, the
        # bottom right pixel, the left column, all: sums 0, 255, 510, 1020 -- and block n takes the patterns that the three
        # base-4 digits of n % 64 name: the 4^3 combinations, all of them in a 16x16 picture, with both extremes of every
        # chroma accumulator (pc, all blue and no red or green: 256 before the clip)
        pat = np.array([[0, 0, 0, 0], [0, 0, 0, 255], [255, 0, 255, 0], [255, 255, 255, 255]], np.uint8)   # [pattern][dy * 2 + dx]
        pic = np.empty((h, w, 3), np.uint8)
        by, bx = np.mgrid[0:h // 2, 0:w // 2]
        n = (by * (w // 2) + bx) % 64
        for c in range(3):
            which = (n >> (2 * c)) & 3
            for dy in range(2):
                for dx in range(2):
                    pic[dy::2, dx::2, c] = pat[which, dy * 2 + dx]
    else:
        assert name in ("gradient", "textured")
        yy, xx = np.mgrid[0:h, 0:w]
        pic = np.stack([(xx * 255) // (w - 1), (yy * 255) // (h - 1), ((xx + yy) * 255) // (w + h - 2)], axis=2)
        if name == "textured":                    # something to code: waves and mild noise on the ramps
            wave = (24 * np.sin(xx / 3.0) * np.cos(yy / 5.0)).astype(np.int64)
            pic = np.clip(pic + wave[:, :, None] + np.random.default_rng(seed).integers(-10, 11, (h, w, 3)), 0, 255)
        pic = pic.astype(np.uint8)
    return (255 - pic) if inverted else pic


def picture(name, lay, w, h, seed=23, inverted=False):
    """The raw planes of picture `name` in layout `lay`."""
    return pack(lay, rgb_picture(name, w, h, seed, inverted), np.random.default_rng(seed + 1000))
