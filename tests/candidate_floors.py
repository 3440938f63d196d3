"""The candidate cut of the 4x4 luma leaf search (wrenc_amd/csrc/dev_search.h, kCandidateCut / leaf4_search) on the host,
for the tests and for tools/candidate_floor_model.py: the per-class floors recomputed from a config's tables with the
formula of fill_split_floors (wrenc_amd/csrc/const_block.cpp), the search-time MPM list of every 4x4 DUAL_TREE_LUMA leaf of
an oracle encode, the oracle's candidate trace grouped per leaf, and a leaf search replayed under the rule.
Nothing here touches a GPU."""
import numpy as np

import split_floors as sf

F = np.float32
PLANAR, DC = 0, 1
NO_MODE = -1


def rd_cost(ssd, level, lam):
    """block_splitter.rs:472-473 in f32, term by term as the device forms it."""
    lv = F(F(level) * F(1.0 / 16384.0))
    return F(F(ssd) + F(F(lam) * lv))


class CandFloors:
    """cls[k]: what a candidate of mode class k (0 planar, 1 .. 5 mpm_idx 0 .. 4, 6 .. 66 remainder) costs at least;
    ang: the smallest over the classes 2 .. 66, which only angular modes can have."""

    def __init__(self, cls):
        self.cls = np.asarray(cls, F)
        assert self.cls.shape == (67,)
        self.ang = F(self.cls[2:].min())
        self.proven = bool(np.isfinite(self.cls).all())


def floors_of_config(cfg):
    """DevConst::cand_floor from the tables of a wrenc_gpu_config: rd_cost(0, header_bits_luma[DUAL_LUMA][0][cls], lambda_rd)
    per class under the `proven` condition of the split floors; all -inf (a floor that never fires) otherwise."""
    hb = np.array(cfg.header_bits_luma, np.int64).reshape(2, 4, 67)
    hc = np.array(cfg.header_bits_chroma, np.int64)
    lv = np.array(cfg.lv_table, np.int64)
    lam, lam_c = F(cfg.lambda_rd), F(cfg.lambda_rd_chroma)
    proven = (lv >= 0).all() and lam >= 0 and lam_c >= 0 and min(int(hb[1, 0].min()), int(hb[0].min()), int(hc.min())) >= 0
    with np.errstate(all="ignore"):
        cls = np.array([rd_cost(0, int(b), lam) for b in hb[1, 0]], F)
    if not proven or not np.isfinite(cls).all():
        cls = np.full(67, -np.inf, F)
    return CandFloors(cls)


def mpm_list(left, above):
    """ctu.rs:1498-1635 (dev_search.h, mpm_list) from the two neighbour modes, PLANAR where there is no neighbour."""
    if left == above and left > DC:
        m = left
        return (m, 2 + (m + 61) % 64, 2 + (m - 1) % 64, 2 + (m + 60) % 64, 2 + m % 64)
    if left != above and (left > DC or above > DC):
        mn, mx = min(left, above), max(left, above)
        if mn > DC:
            d = mx - mn
            if d == 1:
                rest = (2 + (mn + 61) % 64, 2 + (mx - 1) % 64, 2 + (mn + 60) % 64)
            elif d >= 62:
                rest = (2 + (mn - 1) % 64, 2 + (mx + 61) % 64, 2 + mn % 64)
            elif d == 2:
                rest = (2 + (mn - 1) % 64, 2 + (mn + 61) % 64, 2 + (mx - 1) % 64)
            else:
                rest = (2 + (mn + 61) % 64, 2 + (mn - 1) % 64, 2 + (mx + 61) % 64)
            return (left, above) + rest
        return (mx, 2 + (mx + 61) % 64, 2 + (mx - 1) % 64, 2 + (mx + 60) % 64, 2 + mx % 64)
    return (DC, 50, 18, 46, 54)


def mpm_class_of(mpl, mode):
    if mode == PLANAR:
        return 0
    if mode in mpl:
        return 1 + mpl.index(mode)
    return 6 + (mode - 1 - sum(k < mode for k in mpl))


class Leaf:
    """One 4x4 DUAL_TREE_LUMA leaf of an exhaustive search: its search-time MPM list, its full candidates (mode, f32 cost)
    in evaluation order [planar, DC, cm, cm - 1, cm + 1] and the SAD of cm (the minimum of its SAD list)."""

    def __init__(self, x, y, mpl):
        self.x, self.y, self.mpl, self.cands, self.sads = x, y, mpl, [], {}

    def exhaustive(self):
        """(mode, cost): the first minimum as a running strict-less update."""
        mode, best = self.cands[0]
        for m, v in self.cands[1:]:
            if v < best:
                mode, best = m, v
        return mode, best


def leaves_of(rec, rows):
    """{(x, y): Leaf} of a traced oracle encode (split_floors.ordered_trace).  During the search of a CTU every in-CTU
    neighbour lookup resolves to the CTU's 32x32 CU, which carries the best unsplit luma mode (the last full candidate of
    the 32x32 leaf); the left CTU answers with its final map, the CTU row above with PLANAR."""
    vals = rows[:, 7].copy().view(np.float32)
    cu32, out = {}, {}
    for r, v in zip(rows[:, :7].tolist(), vals.tolist()):
        x, y, lg, tree, kind, ml, mc = r
        if kind == 1 and lg == 5 and tree == sf.SINGLE:
            cu32[(x, y)] = ml
        if lg != 2 or tree != sf.DUAL_LUMA:
            continue
        leaf = out.get((x, y))
        if leaf is None:
            root = cu32[(x & ~31, y & ~31)]
            if x & 31:
                left = root
            elif x > 0:
                left = int(rec["luma_mode"][(y + 3) >> 2, (x >> 2) - 1])
            else:
                left = PLANAR
            above = root if y & 31 else PLANAR
            leaf = out[(x, y)] = Leaf(x, y, mpm_list(left, above))
        if kind == 1:
            # (rows of the block after its five candidates are the final pass's evaluation of the winner)
            n = len(leaf.cands)
            if n < 3 or n < 3 + (leaf.cands[2][0] >= 3) + (leaf.cands[2][0] + 1 <= 66):
                leaf.cands.append((ml, F(v)))
        elif kind == 0:
            leaf.sads[mc] = int(v)
    for leaf in out.values():
        modes = [m for m, _ in leaf.cands]
        cm = modes[2]
        want = [PLANAR, DC, cm] + ([cm - 1] if cm >= 3 else []) + ([cm + 1] if cm + 1 <= 66 else [])
        assert modes == want, ("a 4x4 leaf's candidates are not [planar, DC, cm, cm - 1, cm + 1]", leaf.x, leaf.y, modes)
    return out


def replay_leaf(leaf, fl, eps=0.0, cls_of=mpm_class_of, second=None):
    """The leaf search under the rule: (mode, cost, what), what = "sad" (the SAD search and pack B skipped), "packB" (pack
    B alone) or None.  eps and cls_of exist to state wrong rules: a cut on floor + eps >= best, the floor of another
    class.  second(leaf, mode, floor) -> a larger floor of one candidate of pack B (the model's optional bound)."""
    mode, best = leaf.cands[0]
    if leaf.cands[1][1] < best:
        mode, best = leaf.cands[1]
    fa = fl.ang
    if leaf.mpl[0] > DC and fl.cls[1] < fa:
        fa = fl.cls[1]
    if best <= F(fa + F(eps)):
        return mode, best, "sad"
    floors = [fl.cls[cls_of(leaf.mpl, m)] for m, _ in leaf.cands[2:]]
    if second is not None:
        floors = [max(f, second(leaf, m, f)) for f, (m, _) in zip(floors, leaf.cands[2:])]
    if all(F(f + F(eps)) >= best for f in floors):
        return mode, best, "packB"
    for m, v in leaf.cands[2:]:
        if v < best:
            mode, best = m, v
    return mode, best, None


class Touched(dict):
    """A cost table that remembers which entries split_floors.replay read: the leaves the split cut still searches."""

    def __init__(self, *a):
        super().__init__(*a)
        self.read = set()

    def __getitem__(self, k):
        self.read.add(k)
        return super().__getitem__(k)


def searched_leaves(cost, w, h, split_fl):
    """The (x, y) of the 4x4 luma leaves the wave schedule searches under the split cut with floors."""
    t = Touched(cost)
    for cy in range(0, h, 32):
        for cx in range(0, w, 32):
            sf.replay(t, cx, cy, 0, split_fl)
    return sorted((k[0], k[1]) for k in t.read if k[2] == 2 and k[3] == sf.DUAL_LUMA)


def counts(rec, rows, w, h, cfg, second=None):
    """What the rule does on one traced encode: {"searched", "sad", "packB"} among the leaves the split cut searches."""
    cost, _ = sf.leaf_costs(rows)
    leaves = leaves_of(rec, rows)
    fl = floors_of_config(cfg)
    out = {"leaves": len(leaves), "searched": 0, "sad": 0, "packB": 0}
    for xy in searched_leaves(cost, w, h, sf.floors_of_config(cfg)):
        what = replay_leaf(leaves[xy], fl, second=second)[2]
        out["searched"] += 1
        if what:
            out[what] += 1
    return out
