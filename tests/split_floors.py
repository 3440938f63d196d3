"""The split cut with floors (wrenc_amd/csrc/dev_search.h, split_floor_cut) on the host, for the tests and for
tools/split_floor_model.py: the floors recomputed from a config's tables with the formula of fill_split_floors
(wrenc_amd/csrc/const_block.cpp), the oracle's candidate trace in evaluation order, the cost of every leaf and node of an
exhaustive search taken from it, and the search replayed under a cut rule with counts of what it visits.
Nothing here touches a GPU."""
import ctypes as C

import numpy as np

F = np.float32
SINGLE, DUAL_LUMA, DUAL_CHROMA = 0, 1, 2


class Floors:
    """leaf4, leafc4, single: a 4x4 luma leaf, the chroma leaf of a split 8x8, an unsplit block; node[level]: a node at
    tree level 0 .. 2 (32x32, 16x16, 8x8) of a search at max-split-depth `depth`."""

    def __init__(self, leaf4, leafc4, single, depth):
        self.leaf4, self.leafc4, self.single, self.depth = F(leaf4), F(leafc4), F(single), depth
        self.node = [None, None, None]
        for level in (2, 1, 0):
            if level >= depth:
                self.node[level] = self.single
                continue
            s = F(0.0)
            for f in self.children(level):
                s = F(s + f)
            self.node[level] = min(self.single, s)

    def children(self, level):
        """The floors of the children of a split node at `level`, in z-order."""
        return [self.leaf4] * 4 + [self.leafc4] if level == 2 else [self.node[level + 1]] * 4


def floors_of_config(cfg):
    """fill_split_floors from the tables of a wrenc_gpu_config (wrenc_amd.gpu.default_config): per tree type the smallest
    header-bit entry a leaf can be charged, a level cost of 0 (no lv_table entry is negative, and a block without levels
    costs 0), as the cost function forms a cost: 0.0f + lambda * ((float)bits / 16384.0f).  All 0.0 where the tables
    prove nothing."""
    hb = np.array(cfg.header_bits_luma, np.int64).reshape(2, 4, 67)
    hc = np.array(cfg.header_bits_chroma, np.int64)
    lv = np.array(cfg.lv_table, np.int64)
    lam, lam_c = F(cfg.lambda_rd), F(cfg.lambda_rd_chroma)
    dual, single, chroma = int(hb[1, 0].min()), int(hb[0].min()), int(hc.min())
    proven = (lv >= 0).all() and lam >= 0 and lam_c >= 0 and min(dual, single, chroma) >= 0

    def floor_of(lm, bits):
        f = F(F(0.0) + F(lm * F(F(bits) / F(16384.0))))
        return f if proven and f >= 0 else F(0.0)
    return Floors(floor_of(lam, dual), floor_of(lam_c, chroma), floor_of(lam, single), int(cfg.max_split_depth))


def zero_floors(depth):
    """The plain rule: every unsearched child counted as 0.0."""
    return Floors(0.0, 0.0, 0.0, depth)


def ordered_trace(y, cb, cr, qp, depth):
    """(record, rows): the oracle's record of the picture and its candidate evaluations in the order it made them, rows of
    (x, y, log2n, tree, kind, ml, mc, f32 cost); kind 1 = a full candidate, 3 = a chroma candidate."""
    from oracle import pyoracle as po
    lib = po.lib()
    lib.wro_trace_enable(1)
    try:
        out = po.encode_picture(y, cb, cr, qp, depth)
        lib.wro_trace_read.restype = C.c_long
        n = lib.wro_trace_read(None, C.c_long(0))
        buf = np.zeros((n, 8), np.int32)
        lib.wro_trace_read(buf.ctypes.data_as(C.c_void_p), C.c_long(n))
    finally:
        lib.wro_trace_enable(0)
    return out, buf


def leaf_costs(rows):
    """{(x, y, log2n, tree): f32 cost the leaf search of that block returned} and {same key: its smallest candidate}.
    block_splitter.rs:886-1078: a SINGLE_TREE leaf returns its last full candidate (the winner's luma with the chroma that
    won), a DUAL_TREE_LUMA leaf the smallest of its full candidates, the DUAL_TREE_CHROMA leaf the smaller of its two
    chroma candidates (:794-885)."""
    cost, low = {}, {}
    vals = rows[:, 7].copy().view(np.float32)
    for r, v in zip(rows[:, :5].tolist(), vals.tolist()):
        x, y, lg, tree, kind = r
        v = F(v)
        if kind != (3 if tree == DUAL_CHROMA else 1):
            continue
        key = (x, y, lg, tree)
        low[key] = min(low.get(key, v), v)
        cost[key] = v if tree == SINGLE else low[key]
    return cost, low


def replay(cost, x, y, level, fl, strict=True, stats=None, exhaustive=False):
    """The search of node (x, y) at tree `level` from the leaf costs of an exhaustive search, with the device's rule: before
    each child, the partial sum plus the floors of the children still to come, added one by one in z-order, against the
    unsplit cost.  Returns the node's cost; `stats` counts what was searched and what cut.  exhaustive: no cut, and
    stats["nodes"] collects (level, cost) of every node."""
    lg = 5 - level
    u = cost[(x, y, lg, SINGLE)]
    if level >= fl.depth:
        if stats is not None and exhaustive:
            stats.setdefault("nodes", []).append((level, u))
        return u
    kf = fl.children(level)
    if level == 2:
        kids = [("leaf4", (x + 4 * (i & 1), y + 4 * (i >> 1), 2, DUAL_LUMA)) for i in range(4)] + [("leafc4", (x, y, 3, DUAL_CHROMA))]
    else:
        h = 1 << (lg - 1)
        kids = [("node%d" % h, (x + h * (i & 1), y + h * (i >> 1))) for i in range(4)]
    s = F(0.0)
    lost = False
    if stats is not None:
        stats["split%d" % (1 << lg)] = stats.get("split%d" % (1 << lg), 0) + 1
    for i, (name, k) in enumerate(kids):
        if not exhaustive:
            b = s
            for f in kf[i:]:
                b = F(b + f)
            if (b > u) if strict else (b >= u):
                lost = True
                if stats is not None:
                    stats["cuts"] = stats.get("cuts", 0) + 1
                    if not s > u:
                        stats["floor_cuts"] = stats.get("floor_cuts", 0) + 1
                    if i == 0:
                        stats["skipped%d" % (1 << lg)] = stats.get("skipped%d" % (1 << lg), 0) + 1
                break
        c = cost[k] if level == 2 else replay(cost, k[0], k[1], level + 1, fl, strict, stats, exhaustive)
        if stats is not None:
            stats[name] = stats.get(name, 0) + 1
        s = F(s + c)
    out = u if lost or s > u else s
    if stats is not None and exhaustive:
        stats.setdefault("nodes", []).append((level, out))
    return out
