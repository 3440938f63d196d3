"""Pictures on which the search's tie rules decide something (test_tie_cases.py on the CPU, test_gpu_ties.py on the
device).

With the default rate model a cost is (float)ssd + lambda * bits and the header bits of two candidates that could tie on
distortion differ, so a tie almost never decides anything.  The reference's own --extra-params reach a model in which
ties are everywhere: lambda_mul_dq_trellis=0 and a=0 make lambda_rd and lambda_rd_chroma zero (the quantiser's lambda is
untouched, so levels and reconstructions stay ordinary) and a cost is (float)ssd.  The first CTU of a picture has no
neighbours, so planar, DC and mode 2 predict the same block there and so do DM and CCLM chroma; on flat and striped
content split and unsplit tie at every level.

The seven rules, by their switch in the oracle (pyoracle.TIE_RULES, oracle/wrenc_oracle.h):

    R1  first minimum of the 13 coarse SADs             R5  CCLM pick on <= (LT, then T, then L)
    R2  step search: the current mode keeps a tie       R6  the derived chroma mode keeps a tie against CCLM
    R3  step search: mode - step before mode + step     R7  split_cost > no_split_cost: a tie goes to the split
    R4  first minimum of [planar, DC, directional]

decisive() says where a rule decides in a case, by comparing the oracle's record with the record of the oracle that
takes the other side.  A block counts only where the cause is the block's own: the two records agree on every
reconstructed sample the block can predict from (the row above and the column to the left, twice the block's size, in
all three planes), so that a difference carried over from an earlier block is not counted as a tie of this one."""
import functools

import numpy as np

from content import content

ZERO = "lambda_mul_dq_trellis=0,a=0"     # lambda_rd = lambda_rd_chroma = 0: a cost is (float)ssd
ZERO_CHROMA = "a=0"                      # lambda_rd_chroma = 0 alone
DEFAULT = None
RULES = ("R1", "R2", "R3", "R4", "R5", "R6", "R7")
LUMA_RULES, CHROMA_RULES = ("R1", "R2", "R3", "R4"), ("R5", "R6")
KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr", "ctu_cost")

# (kind, width, height, seed, qp, max-split-depth).  64x64: a corner, a top-edge, a left-edge and an interior CTU;
# 96x64 a second interior CTU.  What each case is in the list for (measured, test_tie_cases.py holds it):
_KINDS = {
    0: ("flat", "extremes", "cclm", "noise"),                       # R4, R5, R6 at 32x32
    1: ("flat", "stripes110", "extremes", "noise"),                 # R7 at the 32x32 node; R2, R4, R5, R6 at 16x16
    2: ("flat", "stripes0", "stripes110", "extremes", "cclm", "noise"),    # R4, R5, R6 at 8x8; R7 at 32x32 only
    3: ("flat", "stripes0", "stripes45", "stripes110", "extremes", "cclm", "checker", "noise"),
    # depth 3: every rule at 4x4; R7 at the 16x16 and 8x8 nodes (stripes0, extremes); R3 (stripes110)
}
CASES = tuple((kind, 64, 64, 5, 32, depth) for depth in (0, 1, 2, 3) for kind in _KINDS[depth]) + (
    # 96x64 is the smallest picture with two CTUs on one anti-diagonal, where an AUTO call mixes team and wave launches
    ("cclm", 96, 64, 7, 37, 0), ("flat", 96, 64, 5, 32, 1), ("stripes0", 96, 64, 5, 32, 2),
    ("noise", 96, 64, 7, 27, 3), ("checker", 96, 64, 5, 22, 3))     # R3 twice more, other QPs and seeds


def groups():
    """The cases by (width, height, max-split-depth): one device context each, a case per slot."""
    out = {}
    for c in CASES:
        out.setdefault((c[1], c[2], c[5]), []).append(c)
    return out


def case_id(case):
    return "%s-%dx%d-s%d-qp%d-d%d" % case


def frame(case):
    kind, w, h, seed = case[:4]
    return content(kind, w, h, seed)


@functools.lru_cache(maxsize=None)
def record(case, extra=DEFAULT, rule=None):
    """The oracle's record of a case under an extra-params string, with one tie rule flipped if `rule` names one.
    Cached and shared: treat the arrays as read-only."""
    from oracle import pyoracle as po
    po.set_extra_params(extra)
    po.debug_perturb(po.TIE_RULES[rule] if rule else 0)
    try:
        rec = po.encode_picture(*frame(case), case[4], case[5])
    finally:
        po.debug_perturb(0)
        po.set_extra_params(None)
    assert rec["final_pass_mismatches"] == 0
    for a in rec.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return rec


def changed(case, extra, rule):
    """Does flipping `rule` change any key of the case's record?"""
    a, b = record(case, extra), record(case, extra, rule)
    return any(not np.array_equal(a[k], b[k]) for k in KEYS)


def _same_surroundings(a, b, x, y, n):
    """Both records hold the same reconstruction in the row above and the column left of the n x n luma block at
    (x, y), over twice its size (everything a prediction of the block can read), in all three planes."""
    for key, sh in (("rec_y", 0), ("rec_cb", 1), ("rec_cr", 1)):
        pa, pb = a[key], b[key]
        x0, y0, m = x >> sh, y >> sh, n >> sh
        if y0 > 0 and not np.array_equal(pa[y0 - 1, max(x0 - 1, 0):x0 + 2 * m], pb[y0 - 1, max(x0 - 1, 0):x0 + 2 * m]):
            return False
        if x0 > 0 and not np.array_equal(pa[y0:y0 + 2 * m, x0 - 1], pb[y0:y0 + 2 * m, x0 - 1]):
            return False
    return True


def decisive(case, extra, rule):
    """The set of log2 sizes at which `rule` decides in the case.

    R1..R4: the log2 size of a luma block of the same partition in both records whose luma mode differs.
    R5, R6: the log2 size of the CU of a chroma block whose chroma mode differs while partition, luma mode and luma
            reconstruction of the CU are the same; 2 stands for the 4x4 chroma leaf of a split 8x8.
    R7:     the log2 size of a node that the flipped oracle leaves unsplit and the oracle splits.
    In each case the block's surroundings are the same in both records (module docstring)."""
    a, b = record(case, extra), record(case, extra, rule)
    sa, sb = a["cu_log2_size"], b["cu_log2_size"]
    out = set()
    if rule == "R7":
        for y4, x4 in np.argwhere(sb > sa):
            lg = int(sb[y4, x4])
            n = 1 << lg
            x, y = (x4 * 4) & ~(n - 1), (y4 * 4) & ~(n - 1)
            if _same_surroundings(a, b, x, y, n):
                out.add(lg)
        return out
    if rule in LUMA_RULES:
        for y4, x4 in np.argwhere((sa == sb) & (a["luma_mode"] != b["luma_mode"])):
            lg = int(sa[y4, x4])
            n = 1 << lg
            x, y = (x4 * 4) & ~(n - 1), (y4 * 4) & ~(n - 1)
            if _same_surroundings(a, b, x, y, n):
                out.add(lg)
        return out
    for y8, x8 in np.argwhere(a["chroma_mode"] != b["chroma_mode"]):
        lg = int(sa[2 * y8, 2 * x8])
        n = max(1 << lg, 8)
        x, y = (x8 * 8) & ~(n - 1), (y8 * 8) & ~(n - 1)
        cu4 = (slice(y // 4, (y + n) // 4), slice(x // 4, (x + n) // 4))
        cu = (slice(y, y + n), slice(x, x + n))
        if (np.array_equal(sa[cu4], sb[cu4]) and np.array_equal(a["luma_mode"][cu4], b["luma_mode"][cu4])
                and np.array_equal(a["rec_y"][cu], b["rec_y"][cu]) and _same_surroundings(a, b, x, y, n)):
            out.add(lg)
    return out
