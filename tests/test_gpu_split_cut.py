"""The split cut of the wave schedule (wrenc_amd/csrc/dev_search.h, kSplitCut): a node's children are searched only
until their partial cost is strictly greater than the node's unsplit cost.  The decision it anticipates is the
reference's (block_splitter.rs:1116-1145: children summed in z-order in f32 from 0.0, the unsplit candidate wins only
when the sum is strictly greater), so every record must stay what the exhaustive search makes:

  * against the CPU oracle, on every plane of the record, at max-split-depth 1, 2 and 3, on content where splits lose
    early (smooth), where they win at every level (textured, noise), and on flat pictures, where candidates of equal
    cost are common and a cut on >= instead of > would take the other side of a tie;
  * against the exhaustive build of the same sources (libwrenc_gpu_trace.so) on larger pictures;
  * the rule itself in NumPy f32 arithmetic: cutting gives the decision and the cost of the full sum, for the cut
    inside an 8x8 node's split, the cut between siblings, and the bound through the ancestors (a node that is still
    open returns at least min(unsplit cost, partial sum), which may already decide an ancestor's comparison)."""
import os

import numpy as np
import pytest

KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr",
        "ctu_cost")


def _frame(kind, w, h, i):
    from content import content
    from wrenc_amd import synth
    if kind == "smooth":
        return synth.synth_frame(w, h, i)
    if kind == "textured":
        return synth.synth_textured_frame(w, h, i)
    if kind == "flat":      # one value per plane, another one per picture
        y, cb, cr = content("flat", w, h, i)
        return y + np.uint8(17 * i), cb - np.uint8(9 * i), cr + np.uint8(5 * i)
    if kind == "flat_steps":  # flat 16x8 blocks of two values: flat nodes next to nodes with one edge
        return content("extremes", w, h, i)
    return content(kind, w, h, 40 + i)


def _same(got, ref, what):
    for k in KEYS:
        if not np.array_equal(got[k], ref[k]):
            bad = np.argwhere(got[k] != ref[k])
            raise AssertionError("%s: %s differs at %d positions, first %s" % (what, k, len(bad), bad[0]))


CONTENT = [("smooth", 32), ("textured", 32), ("noise", 24), ("flat", 32), ("flat_steps", 37)]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("kind,qp", CONTENT)
def test_records_equal_the_oracle(built, kind, qp, depth):
    """Wave schedule alone, then AUTO over a batch in which the thin diagonals run as teams (exhaustive) and the wide
    ones as waves (cut): every slot's record equals the oracle's on every plane."""
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    w, h, n = 160, 96, 6
    frames = [_frame(kind, w, h, i) for i in range(n)]
    refs = [po.encode_picture(*f, qp, depth) for f in frames]
    if kind in ("textured", "noise") and depth == 3:     # splits win at every level here
        sizes = set(np.concatenate([r["cu_log2_size"].ravel() for r in refs]).tolist())
        assert {2, 3, 4} <= sizes, sizes
    if kind == "smooth":                                 # ... and lose here
        assert all((r["cu_log2_size"] >= 4).all() for r in refs)
    enc = gpu.Encoder(w, h, qp=qp, max_split_depth=depth, n_slots=n, schedule=1)
    for s, f in enumerate(frames):
        enc.upload(s, *f)
    enc.encode(0, n)
    enc.sync()
    assert enc.last_schedule() == 1 and enc.final_pass_mismatches() == 0
    for s in range(n):
        _same(enc.download(s), refs[s], "%s qp%d depth %d wave slot %d" % (kind, qp, depth, s))
    enc.set_schedule(0)
    # team while pictures x CTUs of the diagonal x 100 <= slots x pct (wrenc_gpu.hip, kTeamBelowSlotsPct): one CTU -> team
    enc.test_set_wave_slots((200 * n - 1) // (65 if depth == 3 else 50))
    enc.encode(0, n)
    enc.sync()
    assert enc.last_schedule() == 0 and enc.final_pass_mismatches() == 0
    for s in range(n):
        _same(enc.download(s), refs[s], "%s qp%d depth %d auto slot %d" % (kind, qp, depth, s))
    enc.close()


def _encode_with(gpu, path, frames, w, h, qp, depth, extra_params=None):
    saved = (gpu._lib, gpu.LIB_PATH)
    gpu._lib, gpu.LIB_PATH = None, path
    try:
        enc = gpu.Encoder(w, h, qp=qp, max_split_depth=depth, n_slots=len(frames), schedule=1, extra_params=extra_params)
        for s, f in enumerate(frames):
            enc.upload(s, *f)
        enc.encode(0, len(frames))
        enc.sync()
        assert enc.final_pass_mismatches() == 0
        out = [enc.download(s) for s in range(len(frames))]
        enc.close()
        return out
    finally:
        gpu._lib, gpu.LIB_PATH = saved


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("qp", [27, 37])
def test_records_equal_the_exhaustive_build(built, qp, depth):
    """The product library against the diagnostic build of the same sources, which searches every child of every node."""
    from wrenc_amd import gpu
    w, h = 256, 160
    frames = [_frame(k, w, h, 3) for k in ("smooth", "textured", "noise", "flat", "flat_steps", "cclm", "checker")]
    product = gpu.LIB_PATH
    exhaustive = os.path.join(os.path.dirname(product), "libwrenc_gpu_trace.so")
    assert os.path.exists(exhaustive), "run __graft_entry__.build() first"
    cut = _encode_with(gpu, product, frames, w, h, qp, depth)
    full = _encode_with(gpu, exhaustive, frames, w, h, qp, depth)
    for s in range(len(frames)):
        _same(cut[s], full[s], "qp%d depth %d picture %d" % (qp, depth, s))


# ---- the decision rule on the host -------------------------------------------------------------------------------
# A node is (unsplit cost, children); the children of a 32x32 / 16x16 node are four nodes, those of an 8x8 node five
# leaf costs (four 4x4 luma leaves, then the chroma leaf).  A decided node is (cost, "U") or (cost, (child, ...)).
F = np.float32


def _full(node, lg=5):
    """The exhaustive search: every child, then the comparison (ties go to the split)."""
    u, kids = node
    s, parts = F(0.0), []
    for k in kids:
        if lg == 3:
            c, p = k, "L"
        else:
            c, p = _full(k, lg - 1)
        s = F(s + c)
        parts.append(p)
    return (u, "U") if s > u else (s, tuple(parts))


class _Lost(Exception):
    """An ancestor's split has lost: `up` levels above the node that noticed."""

    def __init__(self, up):
        self.up = up


def _bound_through(anc, low):
    """Ancestors from the nearest up, each (partial sum, unsplit cost); `low` = a lower bound of what the open child
    of the nearest one returns.  The highest ancestor whose comparison the bound decides, 0 for none (1 = nearest)."""
    lost = 0
    for i, (s, u) in enumerate(anc):
        v = F(s + low)          # the same f32 addition the real sum makes, with low <= the child's cost
        if v > u:
            lost, low = i + 1, u   # that ancestor returns its unsplit cost
        else:
            low = v                # it returns min(u, final sum) >= min(u, v) = v
    return lost


def _cut(node, lg, anc, fired, nested=True):
    """The search with the three cut rules; anc = the ancestors' (partial sum, unsplit cost), nearest first."""
    u, kids = node
    s, parts = F(0.0), []
    for i, k in enumerate(kids):
        if lg == 3:
            c, p = k, "L"
        else:
            try:
                c, p = _cut(k, lg - 1, [(s, u)] + anc, fired, nested)
            except _Lost as e:
                if e.up > 1:
                    raise _Lost(e.up - 1)
                fired["nested"] += 1
                return u, "U"
        s = F(s + c)
        parts.append(p)
        if i + 1 == len(kids):
            break
        if s > u:                                   # rules 1 (inside an 8x8 node's split) and 2 (between siblings)
            fired["split8" if lg == 3 else "sibling"] += 1
            return u, "U"
        if nested:                                  # rule 3: this node returns at least min(u, s) = s
            up = _bound_through(anc, s)
            if up:
                raise _Lost(up)
    return (u, "U") if s > u else (s, tuple(parts))


def _random_tree(rng, lg=5):
    if lg == 3:
        kind = rng.integers(0, 4)
        if kind == 0:       # a few values only: equal costs and zeros
            kids = [F(v) for v in rng.choice([0.0, 0.0, 1.0, 2.5, 7.0], 5)]
        elif kind == 1:     # large and small together: sums that round
            kids = [F(v) for v in rng.choice([0.0, 3.0, 1.0e8, 16777216.0, 0.37], 5)]
        else:
            kids = [F(v) for v in rng.random(5) * rng.choice([1.0, 300.0, 5.0e4])]
    else:
        kids = [_random_tree(rng, lg - 1) for _ in range(4)]
    s = _full((F(np.inf), kids), lg)[0]       # what the split costs
    pick = rng.integers(0, 8)
    if pick == 0:
        u = s                                       # a tie: the split wins
    elif pick == 1:
        u = np.nextafter(s, F(np.inf), dtype=F)
    elif pick == 2:
        u = np.nextafter(s, F(0.0), dtype=F) if s > 0 else F(0.0)
    elif pick == 3:
        u = F(0.0)
    else:
        u = F(s * F(rng.choice([0.2, 0.6, 0.9, 1.1, 1.6, 4.0])))
    return (F(u), kids)


def test_cut_rules_decide_like_the_full_sum():
    rng = np.random.default_rng(2024)
    fired = {"split8": 0, "sibling": 0, "nested": 0}
    plain = {"split8": 0, "sibling": 0, "nested": 0}
    ties = 0
    for _ in range(400):
        tree = _random_tree(rng)
        want = _full(tree)
        assert want[0].dtype == np.float32
        ties += int(_full((F(np.inf), tree[1]))[0] == tree[0])
        for nested, count in ((True, fired), (False, plain)):
            got = _cut(tree, 5, [], count, nested)
            assert got[1] == want[1], "another partition"
            assert got[0] == want[0] and np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes(), "another cost"
    assert min(fired.values()) > 0 and plain["split8"] > 0 and plain["sibling"] > 0 and plain["nested"] == 0, (fired, plain)
    assert ties > 0


def test_tie_goes_to_the_split_and_is_not_cut():
    """Partial sum equal to the unsplit cost, then children of cost zero: the split wins; a cut on >= would lose it."""
    node8 = (F(3.0), [F(1.0), F(2.0), F(0.0), F(0.0), F(0.0)])
    fired = {"split8": 0, "sibling": 0, "nested": 0}
    assert _full(node8, 3) == _cut(node8, 3, [], fired) == (F(3.0), ("L",) * 5)
    assert fired == {"split8": 0, "sibling": 0, "nested": 0}
    over = (F(3.0), [F(1.0), F(2.5), F(0.0), F(0.0), F(0.0)])
    assert _full(over, 3) == _cut(over, 3, [], fired) == (F(3.0), "U") and fired["split8"] == 1
