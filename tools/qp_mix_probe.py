#!/usr/bin/env python3
"""Per-picture QP throughput: the pictures of an RD sweep -- every picture at every QP -- searched
as ONE mixed-QP encode call (wrenc_gpu_set_slot_qp) against one call per QP, on one context, same slots, same results.
Content alternates smooth (synth_frame) and textured (synth_textured_frame) pictures.  Prints one JSON line per case.

    python tools/qp_mix_probe.py [--reps 2]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [  # (width, height, depth, QPs, pictures per QP)
    (3840, 2176, 3, (22, 27, 32, 37), 60),
    (352, 288, 3, (20, 23, 26, 29, 32, 35, 38, 41), 30),
]
WPB = 4


def run_case(w, h, depth, qps, per_qp, reps):
    from wrenc_amd import gpu, synth
    frames = [(synth.synth_frame if f % 2 == 0 else synth.synth_textured_frame)(w, h, f) for f in range(per_qp)]
    n = per_qp * len(qps)
    enc = gpu.Encoder(w, h, qp=qps[0], max_split_depth=depth, n_slots=n)
    for i, q in enumerate(qps):
        for f in range(per_qp):
            enc.upload(i * per_qp + f, *frames[f])
            enc.set_qp(i * per_qp + f, q)
    enc.sync()
    enc.encode(0, n)        # warm-up
    enc.sync()
    t_mixed, t_split = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        enc.encode(0, n)
        enc.sync()
        t_mixed.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for i in range(len(qps)):
            enc.encode(i * per_qp, per_qp)
            enc.sync()
        t_split.append(time.perf_counter() - t0)
    mism = enc.final_pass_mismatches()
    enc.close()
    pad = len(qps) * ((-per_qp) % WPB)
    return {"size": "%dx%d" % (w, h), "depth": depth, "qps": list(qps), "pictures_per_qp": per_qp,
            "mixed_call_fps": round(n / min(t_mixed), 2), "per_qp_calls_fps": round(n / min(t_split), 2),
            "speedup": round(min(t_split) / min(t_mixed), 3), "padding_waves_per_ctu": pad,
            "final_pass_mismatches": mism}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    for c in CASES:
        print(json.dumps(run_case(*c, reps=a.reps)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
