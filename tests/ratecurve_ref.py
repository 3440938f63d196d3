"""Reference side of the rate-histogram tests: include/wrenc_ratecurve.h restated in numpy (the prediction of a block from
its neighbours' originals, the Hadamard transform of the residual, the log-magnitude bins), the curve include/wrenc_rate.h
draws from a histogram, and the pictures the tests share."""
import numpy as np

from complexity_ref import H8

BINS, TOP_BIN, MAX_MAGNITUDE = 64, 56, 16320


def bin_of(m):
    """The bin of a magnitude: 0 for 0, else 1 + 4 floor(log2 m) + the two bits below the leading one (missing bits 0)."""
    m = int(m)
    if m == 0:
        return 0
    e = m.bit_length() - 1
    return 1 + 4 * e + (((m << 2) >> e) & 3)


_BIN = np.array([bin_of(m) for m in range(MAX_MAGNITUDE + 1)], np.int64)


def bin_floor(b):
    """The smallest magnitude of bin b."""
    if b == 0:
        return 0
    e, f = (b - 1) >> 2, (b - 1) & 3
    return ((4 + f) << e) >> 2


def predict(plane, bx, by):
    """(name, 8x8 int64 prediction) of block (bx, by): DC, V, H in this order, a later one only with a strictly smaller SAD."""
    p = plane.astype(np.int64)
    s = p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
    top = p[8 * by - 1, 8 * bx:8 * bx + 8] if by > 0 else None
    left = p[8 * by:8 * by + 8, 8 * bx - 1] if bx > 0 else None
    if top is not None and left is not None:
        dc = (int(top.sum()) + int(left.sum()) + 8) >> 4
    elif top is not None:
        dc = (int(top.sum()) + 4) >> 3
    elif left is not None:
        dc = (int(left.sum()) + 4) >> 3
    else:
        dc = 128
    cands = [("DC", np.full((8, 8), dc, np.int64))]
    if top is not None:
        cands.append(("V", np.tile(top[None, :], (8, 1))))
    if left is not None:
        cands.append(("H", np.tile(left[:, None], (1, 8))))
    best = cands[0]
    for c in cands[1:]:
        if np.abs(s - c[1]).sum() < np.abs(s - best[1]).sum():
            best = c
    return best


def block_coefficients(plane, bx, by):
    s = plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].astype(np.int64)
    return H8 @ (s - predict(plane, bx, by)[1]) @ H8


def _plane_pred(p):
    """The winning prediction of every block of a plane at once (the rules of predict(), vectorised)."""
    h, w = p.shape
    nby, nbx = h // 8, w // 8
    blk = p.reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3)                       # [by, bx, y, x]
    top = np.zeros((nby, nbx, 8), np.int64)
    top[1:] = p[7::8][:nby - 1].reshape(nby - 1, nbx, 8)
    left = np.zeros((nby, nbx, 8), np.int64)
    left[:, 1:] = p[:, 7::8][:, :nbx - 1].reshape(nby, 8, nbx - 1).transpose(0, 2, 1)
    has_t = np.zeros((nby, nbx), bool)
    has_t[1:] = True
    has_l = np.zeros((nby, nbx), bool)
    has_l[:, 1:] = True
    st, sl = top.sum(-1), left.sum(-1)
    dc = np.where(has_t & has_l, (st + sl + 8) >> 4, np.where(has_t, (st + 4) >> 3, np.where(has_l, (sl + 4) >> 3, 128)))
    pdc = np.broadcast_to(dc[:, :, None, None], blk.shape)
    pv = np.broadcast_to(top[:, :, None, :], blk.shape)
    ph = np.broadcast_to(left[:, :, :, None], blk.shape)
    big = np.int64(1) << 40
    sad_dc = np.abs(blk - pdc).sum((2, 3))
    sad_v = np.where(has_t, np.abs(blk - pv).sum((2, 3)), big)
    sad_h = np.where(has_l, np.abs(blk - ph).sum((2, 3)), big)
    use_v = sad_v < sad_dc
    least = np.where(use_v, sad_v, sad_dc)
    use_h = sad_h < least
    pred = np.where(use_h[:, :, None, None], ph, np.where(use_v[:, :, None, None], pv, pdc))
    return blk, pred


def plane_hist(plane):
    """(64,) uint64: the plane's coefficients per bin."""
    blk, pred = _plane_pred(plane.astype(np.int64))
    coef = H8 @ (blk - pred) @ H8
    return np.bincount(_BIN[np.abs(coef).ravel()], minlength=BINS).astype(np.uint64)


def rate_hist(y, cb, cr):
    """(3, 64) uint64: wrenc_rate_hist of a picture."""
    return np.stack([plane_hist(p) for p in (y, cb, cr)])


def padded(planes, w, h):
    """A vis picture in the top-left corner of a w x h one, its last column and row repeated (wrenc_gpu_set_visible_size)."""
    out = []
    for p, (hh, ww) in zip(planes, ((h, w), (h // 2, w // 2), (h // 2, w // 2))):
        out.append(np.pad(p, ((0, hh - p.shape[0]), (0, ww - p.shape[1])), mode="edge"))
    return tuple(out)


def flat(w, h, v=93):
    return tuple(np.full(s, v, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def checker8(w, h):
    """0 / 255 squares of 8x8: every block but the first is flat 255 next to flat 0 or the reverse, so every candidate
    ties at SAD 64 x 255, DC wins and the residual's DC coefficient is 64 x 255 = 16,320."""
    def plane(hh, ww, inv):
        yy, xx = np.mgrid[0:hh, 0:ww]
        return (255 * ((((xx >> 3) + (yy >> 3)) & 1) ^ inv)).astype(np.uint8)
    return plane(h, w, 0), plane(h // 2, w // 2, 0), plane(h // 2, w // 2, 1)


# The curve (include/wrenc_rate.h): bits of a coefficient of bin b at QP q, and a picture's P(q)

def bin_rep(b):
    """wrenc_rate_bin_rep: the magnitude a bin stands for: the middle of its range [floor(b), floor(next occupied bin))."""
    if b == 0:
        return 0.0
    lo = bin_floor(b)
    nxt = b + 1
    while nxt <= TOP_BIN and bin_floor(nxt) <= lo:
        nxt += 1
    hi = bin_floor(nxt) if nxt <= TOP_BIN else MAX_MAGNITUDE + 1
    return 0.5 * (lo + hi - 1)


DEAD, TAIL, BITS0, BITS1, CHROMA_WEIGHT = 0.7, 0.125, 2.3, 0.87, 0.5


def level_bits(l):
    l = np.asarray(l, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(l < DEAD, TAIL * l / DEAD, BITS0 + BITS1 * np.log2(np.maximum(l, 1e-300) / DEAD))


def curve(hist):
    """wrenc_rate_curve: P(q), q = 0 .. 63, of a (3, 64) histogram."""
    hist = np.asarray(hist, np.float64)
    n = hist[0] + CHROMA_WEIGHT * (hist[1] + hist[2])
    rep = np.array([bin_rep(b) for b in range(BINS)])
    q = np.arange(64)
    level = rep[None, :] / (8.0 * 2.0 ** ((q[:, None] - 4) / 6.0))
    return (n[None, 1:] * level_bits(level[:, 1:])).sum(axis=1)
