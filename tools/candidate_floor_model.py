"""CPU model of the candidate cut of the 4x4 luma leaf search (wrenc_amd/csrc/dev_search.h, kCandidateCut),
replayed from the oracle's candidate trace of a crop of the benchmark's content.  No GPU.
    python tools/candidate_floor_model.py [WxH] [X,Y] [QP] [DEPTH]     (default 256x128 at 1024,768 of picture 0, QP 32, depth 3)
Per content, among the 4x4 luma leaves the split cut with floors still searches (tests/split_floors.py): the leaves that
skip the SAD search and pack B, the leaves that skip pack B alone, and what the second bound of the issue would add to
the latter: a candidate of pack B whose SAD the search holds (cm, the SAD search's minimum) costs at least
min(rd_cost(ceil(SAD^2 / 16), hb), rd_cost(0, hb + L1)), L1 = the least level cost of a block with a non-zero level.
L1 is taken here as the cheapest 4x4 block with a single level of +-1 (oracle's level_cost): an upper estimate of the
true L1, so the counts it gives are an upper limit of what that bound could cut."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import candidate_floors as cf  # noqa: E402
import split_floors as sf  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from wrenc_amd import gpu, synth  # noqa: E402

w, h = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "256x128").split("x")]
x0, y0 = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "1024,768").split(",")]
qp = int(sys.argv[3]) if len(sys.argv) > 3 else 32
depth = int(sys.argv[4]) if len(sys.argv) > 4 else 3
cfg = gpu.default_config(w, h, qp, depth)
fl = cf.floors_of_config(cfg)
hb = np.array(cfg.header_bits_luma, np.int64).reshape(2, 4, 67)[1, 0]
lam = cfg.lambda_rd
l1 = None
for p in range(16):
    for s in (1, -1):
        blk = np.zeros((4, 4), np.int16)
        blk[p // 4, p % 4] = s
        c = po.level_cost(blk)
        l1 = c if l1 is None else min(l1, c)
print("%dx%d at (%d, %d), QP %d, depth %d; floors: planar %.1f, mpm_idx 0 %.1f, cheapest angular class %.1f; L1 estimate %d (%.1f)" % (
    w, h, x0, y0, qp, depth, fl.cls[0], fl.cls[1], fl.ang, l1, cf.rd_cost(0, l1, lam)))


def second(leaf, mode, floor):
    if mode != leaf.cands[2][0] or mode not in leaf.sads:
        return floor
    bits = int(hb[cf.mpm_class_of(leaf.mpl, mode)])
    sad = leaf.sads[mode]
    return min(cf.rd_cost((sad * sad + 15) // 16, bits, lam), cf.rd_cost(0, bits + l1, lam))


for name, make in (("synth_frame", synth.synth_frame), ("synth_textured_frame", synth.synth_textured_frame)):
    y, cb, cr = make(3840, 2176, 0)
    crop = (y[y0:y0 + h, x0:x0 + w], cb[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], cr[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2])
    rec, rows = sf.ordered_trace(*crop, qp, depth)
    a = cf.counts(rec, rows, w, h, cfg)
    b = cf.counts(rec, rows, w, h, cfg, second=second)
    nctu = (w // 32) * (h // 32)
    n = max(a["searched"], 1)
    print("%s (%d CTUs): %d 4x4 luma leaves, %d searched under the split cut (%.2f per CTU)" % (name, nctu, a["leaves"], a["searched"], a["searched"] / nctu))
    print("  skip the SAD search and pack B   %5d  %5.1f %%  %.2f per CTU" % (a["sad"], 100.0 * a["sad"] / n, a["sad"] / nctu))
    print("  skip pack B alone                %5d  %5.1f %%  %.2f per CTU" % (a["packB"], 100.0 * a["packB"] / n, a["packB"] / nctu))
    print("  pack B skipped in all            %5d  %5.1f %%;  with the second bound at most %d (%.1f %%)" % (
        a["sad"] + a["packB"], 100.0 * (a["sad"] + a["packB"]) / n, b["sad"] + b["packB"], 100.0 * (b["sad"] + b["packB"]) / n))
