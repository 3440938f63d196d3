"""Micro-benchmark of north_star's MFMA question: kernel time of the forward and inverse DCT-2 for N groups x REPS
repetitions, v_dot2 / v_mad_i24 code (what the search kernel ran) against the i8-MFMA versions it runs now
(wrenc_amd/csrc/dev_transform.h: fwd_dct32_mfma, inv_dct32_mfma at 32x32; fwd_dct_mfma, inv_dct_mfma at 8x8 and 16x16,
groups of 1, 2, 3 and 4 blocks as the leaf packs hand them over).  One wave per group, both bit-exact against each other.
    python tools/dct_bench.py [N=16384] [REPS=64]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wrenc_amd import gpu  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
rng = np.random.default_rng(1)
blocks = rng.integers(-255, 256, (n, 32, 32)).astype(np.int16)
enc = gpu.Encoder(64, 64, qp=32, max_split_depth=0)
doc = {"blocks": n, "reps": reps}
for direction, fn, data in (("forward", enc.fwd_dct32, blocks),
                            ("inverse", enc.inv_dct32, rng.integers(-4000, 4001, (n, 32, 32)).astype(np.int16))):
    res = {}
    for name, flag in (("vdot2", 0), ("mfma_i8", 1)):
        out, _ = fn(data, flag, 1)          # warm-up, and the output for the equality check
        best = min(fn(data, flag, reps)[1] for _ in range(3))
        res[name] = {"kernel_ms": best, "ns_per_transform": best * 1e6 / (n * reps), "out": out}
    same = bool(np.array_equal(res["vdot2"].pop("out"), res["mfma_i8"].pop("out")))
    doc[direction] = {"outputs_equal": same, **res, "speedup_mfma": res["vdot2"]["kernel_ms"] / res["mfma_i8"]["kernel_ms"]}
for lg in (3, 4):
    side = 1 << lg
    for nb in (1, 2, 3, 4):
        for direction, fn, lim in (("forward", enc.fwd_dct_groups_arm, 255), ("inverse", enc.inv_dct_groups_arm, 4000)):
            data = rng.integers(-lim, lim + 1, (n, nb, side, side)).astype(np.int16)
            res = {}
            for name, flag in (("vdot2", 0), ("mfma_i8", 1)):
                out, _ = fn(data, flag, 0, 1)
                best = min(fn(data, flag, 0, reps)[1] for _ in range(3))
                res[name] = {"kernel_ms": best, "ns_per_group": best * 1e6 / (n * reps), "out": out}
            same = bool(np.array_equal(res["vdot2"].pop("out"), res["mfma_i8"].pop("out")))
            doc["%s_%dx%d_nb%d" % (direction, side, side, nb)] = {
                "outputs_equal": same, **res, "speedup_mfma": res["vdot2"]["kernel_ms"] / res["mfma_i8"]["kernel_ms"]}
print(json.dumps(doc))
enc.close()
