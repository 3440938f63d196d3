"""Inputs of tests/test_gpu_leaf32.py: 96x96 pictures (3x3 CTUs: the first row and column, an interior CTU, the last
column without an above-right neighbour) whose 32x32 leaf searches take every path of the wave kernels' K_LEAF32 request
(wrenc_amd/csrc/dev_search.h, full_search), and what the oracle's record and trace say about each CTU's 32x32 leaf, so
that tests/test_leaf32_inputs.py can hold every picture to the case it is here for."""
import functools

import numpy as np

W = H = 96
QP = 32
DEPTHS = (0, 1, 2, 3)
KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr",
        "ctu_cost")
LT_CCLM = 81


def _stripes(xx, yy, deg, period):
    ang = deg * np.pi / 180.0
    ph = xx * np.cos(ang) + yy * np.sin(ang)
    return np.sign(np.sin(ph * (2 * np.pi / period)))


def picture(kind, seed=7):
    """One 96x96 4:2:0 picture.  Every kind mixes CTU-sized regions, so that one picture holds several outcomes."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = yy[::2, ::2], xx[::2, ::2]
    ctu = (yy // 32) * 3 + (xx // 32)          # CTU index of every luma sample
    cctu = (cy // 32) * 3 + (cx // 32)
    if kind == "smooth_noisy":
        # smooth ramps (the 32x32 leaf wins its split) beside noise (it loses), flat CTUs between noisy ones (DC beats
        # planar where the references are noise)
        y = 60 + xx * 0.6 + yy * 0.9
        cb, cr = 120 + cx * 0.3, 90 + cy * 0.4
        noisy = np.isin(ctu, (1, 3, 5, 7))
        y = np.where(noisy, rng.integers(0, 256, (H, W)), y)
        flat = np.isin(ctu, (4,))
        y = np.where(flat, 131, y)
        cnoisy = np.isin(cctu, (1, 3, 5, 7))
        cb = np.where(cnoisy, rng.integers(0, 256, cb.shape), cb)
        cr = np.where(cnoisy, rng.integers(0, 256, cr.shape), cr)
    elif kind == "cclm":
        # chroma an affine function of the sub-sampled luma in some CTUs (CCLM wins), independent of it in others (DM)
        y = (128 + 70 * np.sin(xx * 0.11) * np.cos(yy * 0.07) + rng.integers(-3, 4, (H, W))).clip(0, 255)
        ys = y.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
        cb = (0.6 * ys + 40 + rng.integers(-1, 2, ys.shape)).clip(0, 255)
        cr = (220 - 0.7 * ys + rng.integers(-1, 2, ys.shape)).clip(0, 255)
        plain = np.isin(cctu, (0, 4, 8))
        cb = np.where(plain, 140, cb)
        cr = np.where(plain, 77, cr)
    elif kind.startswith("edges"):
        # soft edges at an angle per CTU: directional winners, the full candidates cm - 1 / cm + 1 against cm
        base = float(kind[5:])
        y = np.zeros((H, W))
        for i in range(9):
            y = np.where(ctu == i, 128 + 60 * _stripes(xx, yy, base + 9.0 * i, 61.0), y)
        y = y + rng.integers(-2, 3, (H, W))
        cb, cr = 128 + 0.2 * (y[::2, ::2] - 128), np.full(cx.shape, 100)
    elif kind == "diagonal":
        # constant along x + y: the SAD search ends at mode 66 or mode 2, whose outer neighbour does not exist
        y = 128 + 80 * np.sin((xx + yy) * (2 * np.pi / 47.0))
        cb = 128 + 30 * np.sin((cx + cy) * (2 * np.pi / 23.5))
        cr = 128 - 30 * np.sin((cx + cy) * (2 * np.pi / 23.5))
    else:
        raise ValueError(kind)
    return tuple(np.ascontiguousarray(np.clip(np.rint(p), 0, 255), dtype=np.uint8) for p in (y, cb, cr))


KINDS = ("smooth_noisy", "cclm", "edges20", "diagonal")


@functools.lru_cache(maxsize=None)
def frames():
    return tuple(picture(k) for k in KINDS)


@functools.lru_cache(maxsize=None)
def refs(qp, depth):
    """The oracle's records of the pictures at (qp, depth): computed once, shared, never written to."""
    from oracle import pyoracle as po
    out = tuple(po.encode_picture(*f, qp, depth) for f in frames())
    for r in out:
        for k in KEYS:
            r[k].setflags(write=False)
    return out


def _f32(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


@functools.lru_cache(maxsize=None)
def leaf_facts(depth=3):
    """Per picture, per CTU (raster order): what the oracle's trace and record say about the CTU's 32x32 leaf search --
    cm (the SAD search's mode), the candidates in the reference's order with their costs, the winner (first minimum),
    whether the 32x32 CU is the CTU's decision, and its chroma mode there."""
    from oracle import pyoracle as po
    out = []
    for f in frames():
        rec, trace = po.encode_picture_traced(*f, QP, depth)
        per = []
        for cty in range(3):
            for ctx in range(3):
                x0, y0 = 32 * ctx, 32 * cty
                cands = {}
                for (x, y, lg, tree, kind, ml, mc), vals in trace.items():
                    # (kind 1: a full candidate; the final evaluation with a CCLM chroma mode has mc != ml)
                    if (x, y, lg, kind) == (x0, y0, 5, 1) and ml == mc:
                        assert len(vals) == 1, (x, y, ml, vals)
                        cands[ml] = _f32(next(iter(vals)))
                dirs = sorted(m for m in cands if m > 1)
                cm = dirs[1] if len(dirs) == 3 else (2 if dirs == [2, 3] else 66)
                assert dirs in ([cm - 1, cm, cm + 1], [2, 3], [65, 66]), dirs
                # (a neighbour outside 2..66 is not evaluated)
                order = [0, 1, cm] + [m for m in (cm - 1, cm + 1) if 2 <= m <= 66]
                assert sorted(order) == sorted(cands), (order, sorted(cands))
                win = order[0]
                for m in order[1:]:
                    if cands[m] < cands[win]:
                        win = m
                is32 = bool(rec["cu_log2_size"][y0 // 4, x0 // 4] == 5)
                per.append({"cm": cm, "order": order, "cost": cands, "winner": win, "cu32": is32,
                            "chroma": int(rec["chroma_mode"][y0 // 8, x0 // 8]),
                            "luma": int(rec["luma_mode"][y0 // 4, x0 // 4])})
        out.append(per)
    return out
