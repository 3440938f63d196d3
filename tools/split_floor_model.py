"""CPU model of the split cut with floors (wrenc_amd/csrc/dev_search.h, split_floor_cut): what the
wave schedule searches per node under the plain rule (unsearched children counted as 0) and with floors, replayed from
the oracle's candidate trace of a crop of the benchmark's content.  No GPU.
    python tools/split_floor_model.py [WxH] [X,Y] [QP] [DEPTH]        (default 512x256 at 1024,768 of picture 0, QP 32, depth 3)
The crop is taken out of a 3840x2176 picture, so it is the benchmark's content at that place; the oracle encodes the crop
as a picture of its own (its edge CTUs see picture edges the benchmark's do not)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import split_floors as sf  # noqa: E402
from wrenc_amd import gpu, synth  # noqa: E402

w, h = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "512x256").split("x")]
x0, y0 = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "1024,768").split(",")]
qp = int(sys.argv[3]) if len(sys.argv) > 3 else 32
depth = int(sys.argv[4]) if len(sys.argv) > 4 else 3
fl = sf.floors_of_config(gpu.default_config(w, h, qp, depth))
print("%dx%d at (%d, %d), QP %d, depth %d; floors: 4x4 luma leaf %.1f, chroma leaf %.1f, node 32 / 16 / 8 %s" % (
    w, h, x0, y0, qp, depth, fl.leaf4, fl.leafc4, " / ".join("%.1f" % v for v in fl.node)))
for name, make in (("synth_frame", synth.synth_frame), ("synth_textured_frame", synth.synth_textured_frame)):
    y, cb, cr = make(3840, 2176, 0)
    crop = (y[y0:y0 + h, x0:x0 + w], cb[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], cr[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2])
    rec, rows = sf.ordered_trace(*crop, qp, depth)
    cost, low = sf.leaf_costs(rows)
    stats = {}
    for tag, rule in (("today", sf.zero_floors(depth)), ("floors", fl)):
        st = stats[tag] = {}
        for cy in range(0, h, 32):
            for cx in range(0, w, 32):
                sf.replay(cost, cx, cy, 0, rule, stats=st)
    nctu = (w // 32) * (h // 32)
    print("%s (%d CTUs), today -> with floors:" % (name, nctu))
    for key, per, what in (("leaf4", "split8", "4x4 luma leaves searched per 8x8 split searched"),
                           ("leafc4", "split8", "chroma leaves searched per 8x8 split searched"),
                           ("node8", "split16", "8x8 nodes searched per 16x16 split searched"),
                           ("node16", "split32", "16x16 nodes searched per 32x32 split searched")):
        a, b = stats["today"], stats["floors"]
        print("  %-52s %.2f -> %.2f   (%d of %d -> %d of %d)" % (what, a.get(key, 0) / max(a.get(per, 0), 1), b.get(key, 0) / max(b.get(per, 0), 1),
                                                                a.get(key, 0), a.get(per, 0), b.get(key, 0), b.get(per, 0)))
    for key in ("cuts", "floor_cuts", "skipped8", "skipped16", "skipped32"):
        print("  %-52s %d -> %d" % (key, stats["today"].get(key, 0), stats["floors"].get(key, 0)))
    # as the profile build counts them (cut_leaf4 / cut_leafc4 / cut_node8): children of the splits that were searched
    def left(st, key, per, n):
        return (n * st.get(per, 0) - st.get(key, 0)) / nctu
    a, b = stats["today"], stats["floors"]
    print("  per CTU not searched: 4x4 luma leaves %.2f -> %.2f, chroma leaves %.2f -> %.2f, 8x8 nodes %.2f -> %.2f" % (
        left(a, "leaf4", "split8", 4), left(b, "leaf4", "split8", 4), left(a, "leafc4", "split8", 1), left(b, "leafc4", "split8", 1),
        left(a, "node8", "split16", 4), left(b, "node8", "split16", 4)))
