"""The pictures of test_gpu_pack_records.py and what the oracle's records of them hold (test_pack_records_cases.py checks it
on the CPU).  The packed leaf searches dequantise and transform back only the blocks of a pack that have a level, and the
CCLM tail of a leaf predicts from the probe's down-sampled luma: the records compared must hold CUs of every size with
levels in luma alone, in chroma alone, in both and in neither, and CUs of every size whose chroma is a CCLM mode with the
left neighbour available and not."""
import functools
import itertools

import numpy as np

from content import content

SIZES = ((64, 64), (96, 64))          # the smallest with every neighbour-availability pattern of a CTU
# (stripes0 beside the four kinds the comparison was asked for: the only one whose records hold 32x32 CUs with levels in
# chroma alone and with none at all)
KINDS = ("cclm", "ramp", "stripes20", "checker", "stripes0")
QPS = (22, 32, 42)
DEPTHS = (1, 2, 3)
CASES = list(itertools.product(KINDS, SIZES, QPS, DEPTHS))
KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr", "ctu_cost")
STATES = ("luma", "chroma", "both", "neither")


def picture(kind, size, qp):
    w, h = size
    return content(kind, w, h, 1234 + w + h + qp)


@functools.lru_cache(maxsize=None)
def reference(kind, size, qp, depth):
    """The oracle's record of a case: computed once, shared by the tests, never modified."""
    from oracle import pyoracle as po
    ref = po.encode_picture(*picture(kind, size, qp), qp, depth)
    for k in KEYS:
        ref[k].setflags(write=False)
    return ref


def cus(ref):
    """(log2 size, x, y, state, chroma mode) of every CU of 8x8 .. 32x32 in a record; state names where its levels are."""
    h4, w4 = ref["cu_log2_size"].shape
    out = []
    for lg in (3, 4, 5):
        n = 1 << lg
        for y in range(0, 4 * h4, n):
            for x in range(0, 4 * w4, n):
                if ref["cu_log2_size"][y // 4, x // 4] != lg:
                    continue
                luma = bool(ref["lev_y"][y:y + n, x:x + n].any())
                c = (slice(y // 2, (y + n) // 2), slice(x // 2, (x + n) // 2))
                chroma = bool(ref["lev_cb"][c].any() or ref["lev_cr"][c].any())
                state = "both" if luma and chroma else ("luma" if luma else ("chroma" if chroma else "neither"))
                out.append((lg, x, y, state, int(ref["chroma_mode"][y // 8, x // 8])))
    return out


def coverage():
    """{(log2 size, state)} and {(log2 size, left neighbour available)} of the CUs with a CCLM chroma mode, over all cases."""
    states, cclm = set(), set()
    for case in CASES:
        for lg, x, y, state, mc in cus(reference(*case)):
            states.add((lg, state))
            if mc >= 81:
                cclm.add((lg, x > 0))
    return states, cclm
