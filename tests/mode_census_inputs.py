"""Inputs of tests/test_gpu_mode_census.py: pictures on which every one of the 67 luma intra modes is the search's decision
at every CU size, and what the oracle's record and trace say about them (tests/test_mode_census_inputs.py pins that).

A picture is built block by block in coding order (CTUs in raster order, the n x n blocks of a CTU in z-order): each block
is the ORACLE'S OWN PREDICTION of a planted mode from the part of the picture built so far, plus a small innovation (a linear
ramp and a little noise), so that the planted mode leaves the cheapest residual.  The block's last row and column, the
references of the blocks after it, get strong noise: with smooth references every mode predicts the same block and the
plant decides nothing.  The modes come from a seeded permutation of 0..66 that is reshuffled every 67 blocks, so every mode
stands beside neighbours of every mode (MPM lists, the truncated-binary remainder).  Chroma is planted the same way from the
chroma prediction of the same mode (DM wins), in the 4x4 pictures as an affine function of the luma (CCLM wins), and in the
"dual" pictures from the mode of the bottom-right 4x4 block of each 8x8 area, where the search takes the DM mode of a split
8x8 from.

Nothing here reads anything but the oracle (oracle/libwrenc_oracle.so)."""
import functools
import time

import numpy as np

KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr",
        "ctu_cost")
N_MODES = 67
LT_CCLM, T_CCLM, L_CCLM = 81, 82, 83
TRACE_MAX = 1 << 19                 # kTraceMax of wrenc_amd/csrc (records of the device's trace buffer)

# kind -> (planted log2 size, width, height); "dual" plants 4x4 luma blocks and the chroma of their 8x8 area
KINDS = {"p32": (5, 288, 256), "p16": (4, 160, 128), "p8": (3, 96, 96), "p4": (2, 64, 64), "dual": (2, 96, 96)}
SEEDS = (1, 2, 3, 4)
QPS = (27, 27, 32, 22)              # of the four seeds of a kind: one encode call holds all four (a mixed-QP plan)


def depths(kind):
    """The max-split-depths a kind is encoded at: the one at which the planted size is the smallest CU, and 3."""
    d = 5 - KINDS[kind][0]
    return (d,) if d == 3 else (d, 3)


# every (kind, depth) of the set
ENCODES = tuple((k, d) for k in KINDS for d in depths(k))
# ... and those whose every candidate is compared too: the 288x256 pictures only at depth 0 (the device records the
# re-evaluations the oracle memoises, and its buffer holds TRACE_MAX records)
TRACED = tuple((k, d) for (k, d) in ENCODES if not (k == "p32" and d != 0))


def _zorder(n_side):
    out = []
    for i in range(n_side * n_side):
        x = y = 0
        for b in range(5):
            x |= ((i >> (2 * b)) & 1) << b
            y |= ((i >> (2 * b + 1)) & 1) << b
        out.append((x, y))
    return out


def _innovation(rng, n, amp, noise, edge):
    """A linear ramp of amplitude up to +-amp, +-noise everywhere, +-edge more on the last row and column."""
    t = (np.arange(n) - (n - 1) / 2.0) / max(n - 1, 1)           # -0.5 .. 0.5
    a, b = rng.uniform(-amp, amp, 2)
    inn = a * t[None, :] + b * t[:, None] + rng.integers(-noise, noise + 1, (n, n))
    inn[-1, :] += rng.integers(-edge, edge + 1, n)
    inn[:-1, -1] += rng.integers(-edge, edge + 1, n - 1)
    return inn


def _put(plane, x, y, block):
    n = block.shape[0]
    plane[y:y + n, x:x + n] = np.clip(np.rint(block), 0, 255).astype(np.uint8)


class _Modes:
    """A seeded permutation of 0..66, reshuffled every 67 draws."""

    def __init__(self, rng):
        self.rng, self.left = rng, []

    def next(self):
        if not self.left:
            self.left = self.rng.permutation(N_MODES).tolist()
        return self.left.pop()


@functools.lru_cache(maxsize=None)
def picture(kind, seed):
    """(y, cb, cr) of one planted picture, read-only."""
    from oracle import pyoracle as po
    lg, w, h = KINDS[kind]
    n = 1 << lg
    rng = np.random.default_rng(1000 * lg + seed + (500 if kind == "dual" else 0))
    modes = _Modes(rng)
    y = np.full((h, w), 128, np.uint8)
    cb = np.full((h // 2, w // 2), 128, np.uint8)
    cr = np.full((h // 2, w // 2), 128, np.uint8)
    if kind == "dual":
        order8, order4 = _zorder(4), _zorder(2)
        for y0 in range(0, h, 32):
            for x0 in range(0, w, 32):
                for bx, by in order8:
                    x8, y8 = x0 + 8 * bx, y0 + 8 * by
                    for sx, sy in order4:
                        mode = modes.next()
                        x4, y4 = x8 + 4 * sx, y8 + 4 * sy
                        pred = po.predict_blocks(y, cb, cr, [(x4, y4, 2, 1, 0, mode)])[0]
                        _put(y, x4, y4, pred + _innovation(rng, 4, 40, 2, 40))
                    # the chroma of the 8x8 area from the mode of its bottom-right 4x4 block (the last one planted)
                    for c, plane in ((1, cb), (2, cr)):
                        pred = po.predict_blocks(y, cb, cr, [(x8, y8, 3, 2, c, mode)])[0]
                        _put(plane, x8 // 2, y8 // 2, pred + _innovation(rng, 4, 30, 1, 30))
    else:
        order = _zorder(32 // n)
        # the blocks after the picture's last whole permutation get the prediction of a CCLM mode as their chroma (from
        # the block's own luma, just planted): LT_CCLM, T_CCLM, L_CCLM in turn
        whole = (w // n) * (h // n) // N_MODES * N_MODES
        at = 0
        for y0 in range(0, h, 32):
            for x0 in range(0, w, 32):
                for bx, by in order:
                    mode = modes.next()
                    x, yb = x0 + n * bx, y0 + n * by
                    pred = po.predict_blocks(y, cb, cr, [(x, yb, lg, 1 if lg == 2 else 0, 0, mode)])[0]
                    _put(y, x, yb, pred + _innovation(rng, n, 40, 2, 40))
                    if lg >= 3:
                        cmode = mode if at < whole else LT_CCLM + (at - whole + seed) % 3
                        for c, plane in ((1, cb), (2, cr)):
                            pred = po.predict_blocks(y, cb, cr, [(x, yb, lg, 0, c, cmode)])[0]
                            _put(plane, x // 2, yb // 2, pred + _innovation(rng, n // 2, 30, 1, 30))
                    at += 1
        if lg == 2:
            # chroma an affine function of the sub-sampled luma (the "cclm" recipe of tests/content.py)
            ys = y.astype(np.float64).reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
            cb = np.clip(np.rint(0.6 * ys + 40 + rng.integers(-3, 4, ys.shape)), 0, 255).astype(np.uint8)
            cr = np.clip(np.rint(220 - 0.7 * ys + rng.integers(-3, 4, ys.shape)), 0, 255).astype(np.uint8)
    out = tuple(np.ascontiguousarray(p) for p in (y, cb, cr))
    for p in out:
        p.setflags(write=False)
    return out


def frames(kind):
    return tuple(picture(kind, s) for s in SEEDS)


@functools.lru_cache(maxsize=None)
def _encoded(kind, depth):
    """Per seed (record, trace or None, raw trace records, seconds of oracle time): computed once, shared, never written
    to.  Combinations of TRACED are encoded with the trace on, so that one oracle run serves both tests."""
    from oracle import pyoracle as po
    out = []
    for f, qp in zip(frames(kind), QPS):
        t0 = time.perf_counter()
        if (kind, depth) in TRACED:
            rec, trace = po.encode_picture_traced(*f, qp, depth)
            n_raw = rec["trace_records"]                        # re-evaluations included
        else:
            rec, trace, n_raw = po.encode_picture(*f, qp, depth), None, 0
        dt = time.perf_counter() - t0
        for k in KEYS:
            rec[k].setflags(write=False)
        out.append((rec, trace, n_raw, dt))
    return tuple(out)


def refs(kind, depth):
    """The oracle's records of the four pictures of `kind` at `depth` (QPS[i] for seed i)."""
    return tuple(e[0] for e in _encoded(kind, depth))


def traces(kind, depth):
    """The oracle's trace dictionaries of the same encodes ((kind, depth) in TRACED) and their raw record counts."""
    assert (kind, depth) in TRACED
    return tuple((e[1], e[2]) for e in _encoded(kind, depth))


def oracle_seconds():
    return sum(e[3] for kd in ENCODES for e in _encoded(*kd))


SITUATIONS = ("32", "16", "8 single", "8 dual")     # the four chroma situations: CU size, and the tree of an 8x8


def census(record):
    """What one record decides.  "wins": (4, 67) CUs of log2 size 2..5 (row lg - 2) per luma mode; "dm", "dm_nz": (4, 67)
    chroma blocks per SITUATION coded with the derived mode, per luma mode they derive it from (all / those with a non-zero
    Cb or Cr level); "cclm": (4, 3) chroma blocks per situation coded LT_CCLM, T_CCLM, L_CCLM."""
    cu, lm, cm = record["cu_log2_size"], record["luma_mode"], record["chroma_mode"]
    h4, w4 = cu.shape
    yy, xx = np.mgrid[0:h4, 0:w4]
    wins = np.zeros((4, N_MODES), np.int64)
    for lg in range(2, 6):
        n4 = 1 << (lg - 2)
        top = (cu == lg) & (yy % n4 == 0) & (xx % n4 == 0)
        wins[lg - 2] = np.bincount(lm[top], minlength=N_MODES)[:N_MODES]
    # per 8x8 luma area: any non-zero chroma level, the CU size there, the luma mode DM derives from
    nz = ((record["lev_cb"] != 0) | (record["lev_cr"] != 0)).reshape(h4 // 2, 4, w4 // 2, 4).any(axis=(1, 3))
    cu8 = cu[::2, ::2]
    dm = np.zeros((4, N_MODES), np.int64)
    dm_nz = np.zeros((4, N_MODES), np.int64)
    cclm = np.zeros((4, 3), np.int64)
    for sit, lg in enumerate((5, 4, 3, 2)):
        n8 = 1 << max(lg - 3, 0)
        for by, bx in np.argwhere((cu8 == lg) & (yy[::2, ::2] % (2 * n8) == 0) & (xx[::2, ::2] % (2 * n8) == 0)):
            mode = int(cm[by, bx])
            derived = int(lm[2 * by, 2 * bx] if lg >= 3 else lm[2 * by + 1, 2 * bx + 1])
            if mode >= LT_CCLM:
                cclm[sit, mode - LT_CCLM] += 1
            elif mode == derived:
                dm[sit, derived] += 1
                dm_nz[sit, derived] += bool(nz[by:by + n8, bx:bx + n8].any())
            else:
                raise AssertionError("chroma mode %d at 8x8 area (%d, %d) is neither CCLM nor the derived %d" % (mode, bx, by, derived))
    return {"wins": wins, "dm": dm, "dm_nz": dm_nz, "cclm": cclm}


MPM_BRANCHES = ("both the same angular", "angular 1 apart", "angular 2 apart", "angular 62 apart", "angular 63 or 64 apart",
                "angular, another distance", "one angular", "none angular")


def mpm_branch(left, above):
    """The arm of the MPM derivation (H.266 8.4.2) that the neighbours' modes take, an index into MPM_BRANCHES; the arm of
    distances of 62 and more is counted apart at its boundary."""
    if left == above:
        return 0 if left > 1 else 7
    mn, mx = min(left, above), max(left, above)
    if mx <= 1:
        return 7
    if mn <= 1:
        return 6
    d = mx - mn
    return 1 if d == 1 else 2 if d == 2 else 3 if d == 62 else 4 if d > 62 else 5


def mpm_census(record):
    """(4, 8) CUs of log2 size 2..5 per arm of the MPM derivation, from the decided modes of the CU's left neighbour (at its
    bottom row) and above neighbour (at its last column; planar across a CTU row and outside the picture)."""
    cu, lm = record["cu_log2_size"], record["luma_mode"]
    out = np.zeros((4, len(MPM_BRANCHES)), np.int64)
    for y4, x4 in np.argwhere(cu > 0):
        lg = int(cu[y4, x4])
        n4 = 1 << (lg - 2)
        if y4 % n4 or x4 % n4:
            continue
        left = int(lm[y4 + n4 - 1, x4 - 1]) if x4 > 0 else 0
        above = int(lm[y4 - 1, x4 + n4 - 1]) if y4 % 8 else 0
        out[lg - 2, mpm_branch(left, above)] += 1
    return out


def trace_census(trace):
    """What one trace dictionary evaluates.  "probes": (4, 67) distinct SAD probes (kind 0) of log2 size 2..5 per luma mode;
    "full": (4, 67) distinct full candidates (kind 1); "kinds": the set of kinds present."""
    probes = np.zeros((4, N_MODES), np.int64)
    full = np.zeros((4, N_MODES), np.int64)
    kinds = set()
    for (x, y, lg, tree, kind, ml, mc) in trace:
        kinds.add(kind)
        if kind == 0:
            probes[lg - 2, ml] += 1
        elif kind == 1:
            full[lg - 2, ml] += 1
    return {"probes": probes, "full": full, "kinds": kinds}


def total_census():
    """The censuses summed over the set: census() over every encode, trace_census() over the traced ones."""
    rec = {k: 0 for k in ("wins", "dm", "dm_nz", "cclm")}
    tr = {"probes": 0, "full": 0}
    for kind, depth in ENCODES:
        for r in refs(kind, depth):
            c = census(r)
            for k in rec:
                rec[k] = rec[k] + c[k]
        if (kind, depth) in TRACED:
            for t, _ in traces(kind, depth):
                c = trace_census(t)
                for k in tr:
                    tr[k] = tr[k] + c[k]
    rec.update(tr)
    return rec


def table(total):
    """The census as text: per CU size the wins of every mode, and every cell that misses a condition."""
    lines = []
    for name, arr, rows in (("wins", total["wins"], ("4", "8", "16", "32")), ("SAD probes", total["probes"], ("4", "8", "16", "32")),
                            ("full candidates", total["full"], ("4", "8", "16", "32")),
                            ("DM with a non-zero chroma level", total["dm_nz"], SITUATIONS)):
        lines.append("%s (rows: size, columns: mode 0..66)" % name)
        for r, row in zip(rows, arr):
            lines.append("  %8s | %s | min %d, modes at 0: %s" % (r, " ".join("%d" % v for v in row), row.min(),
                                                                  np.flatnonzero(row == 0).tolist()))
    lines.append("CCLM wins (rows: chroma situation; LT, T, L)")
    for r, row in zip(SITUATIONS, total["cclm"]):
        lines.append("  %8s | %s" % (r, " ".join("%d" % v for v in row)))
    return "\n".join(lines)
