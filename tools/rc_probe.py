"""Rate control's measurements: the prior of include/wrenc_rate.h and the complexity kernel's rate.

    python3 tools/rc_probe.py fit [OUT.json] [--oracle]
        fixed-QP searches of the synthetic content (wrenc_amd/synth.py smooth and textured, tests/content.py) over QP
        17..47, 352x288 and a few 1920x1088 pictures, the bytes of every picture's NAL units against its complexity;
        least squares of ln bytes = ln a + ln N + b ln(C / N) - qp ln 2 / s, and the residuals.  --oracle: the same
        pictures through the CPU oracle (bit-exact with the device, so the same bytes; 352x288 only, on every core)
    python3 tools/rc_probe.py curve FIT.json [OUT.json]
        the buffer model's predictor on the rows of a `fit --oracle` run: every picture's rate
        histogram (tests/ratecurve_ref.py), bytes ~ a P(q) + c CTUs with the library's curve and c and ONE global a (least
        squares in ln bytes), the residuals per content, and the complexity model's on the same rows
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/rc_probe.py kernel [WxH=1920x1088] [N=256] [REPS=4]
    python3 tools/rc_probe.py stats DIR/.../*_kernel_stats.csv [WxH] [N]
        complexity_kernel next to metrics_kernel (which reads twice the bytes: originals and reconstruction)
"""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _pictures(w, h, full):
    from wrenc_amd import synth
    from content import content
    pics = [("smooth%d" % f, synth.synth_frame(w, h, f)) for f in range(4 if full else 2)]
    pics += [("textured%d" % f, synth.synth_textured_frame(w, h, f)) for f in range(4 if full else 2)]
    if full:
        pics += [(k, content(k, w, h, 1)) for k in ("cclm", "ramp", "stripes20", "checker", "noise")]
    return pics


def _measure(w, h, qps, full, depth=2):
    """Rows (name, w, h, qp, C, bytes): every picture at every QP in ONE mixed-QP encode call."""
    from wrenc_amd import bitstream, gpu, rate
    pics = _pictures(w, h, full)
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=depth, n_slots=len(pics) * len(qps))
    slot = 0
    for _, p in pics:
        for q in qps:
            enc.upload(slot, *p)
            enc.set_qp(slot, q)
            slot += 1
    cplx = enc.download_complexity(0, slot, ctu_map=False)
    enc.encode(0, slot)
    rows, slot = [], 0
    for name, _ in pics:
        for q in qps:
            rec = enc.download(slot)
            n = len(bitstream.write_picture_qp(w, h, 32, q, slot, rec))
            s = cplx[slot]["satd"]
            rows.append((name, w, h, q, s[0] + rate.CHROMA_WEIGHT * (s[1] + s[2]), n))
            slot += 1
    enc.close()
    return rows


def _oracle_one(job):
    from oracle import pyoracle
    from wrenc_amd import bitstream
    w, h, q, depth, p = job
    return len(bitstream.write_picture_qp(w, h, 32, q, 0, pyoracle.encode_picture(p[0], p[1], p[2], q, depth)))


def _measure_oracle(w, h, qps, depth=2):
    import multiprocessing
    import complexity_ref
    from wrenc_amd import rate
    pics = _pictures(w, h, True)
    jobs = [(w, h, q, depth, p) for _, p in pics for q in qps]
    with multiprocessing.Pool() as pool:
        sizes = pool.map(_oracle_one, jobs, chunksize=1)
    rows = []
    for (name, p), k in zip(pics, range(0, len(jobs), len(qps))):
        s = complexity_ref.complexity(*p)["satd"]
        rows += [(name, w, h, q, s[0] + rate.CHROMA_WEIGHT * (s[1] + s[2]), sizes[k + i]) for i, q in enumerate(qps)]
    return rows


def fit(argv):
    oracle = "--oracle" in argv
    argv = [a for a in argv if a != "--oracle"]
    if oracle:
        rows = _measure_oracle(352, 288, list(range(17, 48, 2)))
    else:
        rows = _measure(352, 288, list(range(17, 48, 2)), True) + _measure(1920, 1088, list(range(17, 48, 6)), False)
    n = np.array([r[1] * r[2] for r in rows], np.float64)
    x = np.stack([np.ones(len(rows)), np.log(np.array([r[4] for r in rows]) / n), -np.array([r[3] for r in rows], np.float64)], axis=1)
    y = np.log(np.array([r[5] for r in rows], np.float64) / n)
    coef, *_ = np.linalg.lstsq(x, y, rcond=None)
    res = y - x @ coef
    out = {"a": float(np.exp(coef[0])), "b": float(coef[1]), "s": float(np.log(2.0) / coef[2]), "pictures": len(rows),
           "residual_rms_ln": float(np.sqrt(np.mean(res * res))), "residual_max_ln": float(np.max(np.abs(res))), "by_content": {}}
    for name in sorted({r[0] + "@%d" % r[1] for r in rows}):
        sel = np.array([r[0] + "@%d" % r[1] == name for r in rows])
        out["by_content"][name] = {"mean_ln": float(np.mean(res[sel])), "rms_ln": float(np.sqrt(np.mean(res[sel] ** 2))),
                                   "C_per_sample": float(np.mean(np.exp(x[sel, 1])))}
    out["rows"] = [list(r) for r in rows]
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}, indent=1))
    if argv:
        os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
        json.dump(out, open(argv[0], "w"))


def curve(argv):
    import ratecurve_ref
    from wrenc_amd import rate
    fitted = json.load(open(argv[0]))
    rows = [r for r in fitted["rows"] if (r[1], r[2]) == (352, 288)]
    curves = {name: rate.curve(ratecurve_ref.rate_hist(*p)) for name, p in _pictures(352, 288, True)}
    _, c = rate.curve_prior()
    ctus = 11 * 9
    got = np.array([r[5] for r in rows], np.float64)
    unit = np.array([curves[r[0]][r[3]] for r in rows])
    best = None
    for ln_a in np.linspace(-7.0, 1.0, 8001):          # one global a: least squares of ln bytes - ln(a P + c CTUs)
        res = np.log(got) - np.log(np.exp(ln_a) * unit + c * ctus)
        rms = float(np.sqrt(np.mean(res * res)))
        if best is None or rms < best[0]:
            best = (rms, float(np.exp(ln_a)), res)
    rms, a, res = best
    out = {"a": a, "c": c, "pictures": len(rows), "residual_rms_ln": rms, "residual_max_ln": float(np.max(np.abs(res))),
           "complexity_model": {"residual_rms_ln": fitted["residual_rms_ln"], "residual_max_ln": fitted["residual_max_ln"]}, "by_content": {}}
    for name in sorted(curves):
        sel = np.array([r[0] == name for r in rows])
        out["by_content"][name] = {"mean_ln": float(np.mean(res[sel])), "rms_ln": float(np.sqrt(np.mean(res[sel] ** 2))),
                                   "max_ln": float(np.max(np.abs(res[sel])))}
    print(json.dumps(out, indent=1))
    if len(argv) > 1:
        json.dump(out, open(argv[1], "w"), indent=1)


def _args(argv):
    w, h = [int(v) for v in (argv[0] if argv else "1920x1088").split("x")]
    return w, h, int(argv[1]) if len(argv) > 1 else 256, int(argv[2]) if len(argv) > 2 else 4


def kernel(argv):
    from wrenc_amd import gpu, synth
    w, h, n, reps = _args(argv)
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=n)
    frames = [synth.synth_frame(w, h, f) for f in range(8)]
    for s in range(n):
        enc.upload(s, *frames[s % 8])
    enc.encode(0, n)
    enc.sync()
    for rep in range(reps + 1):      # the first round warms up
        m = enc.download_metrics(0, n)
        c = enc.download_complexity(0, n, ctu_map=False)
        r = enc.download_rate_hist(0, n)
        print("%dx%d, %d pictures: PSNR Y %.3f dB, satd %s, zero coefficients %s" % (w, h, n, m[0]["PSNR"]["Y"], c[0]["satd"], r[0, :, 0].tolist()), flush=True)
    enc.close()


def stats(argv):
    w, h, n, _ = _args(argv[1:])
    for row in csv.DictReader(open(argv[0])):
        name = row["Name"]
        for key, per_sample in (("complexity_kernel", 1.5), ("rate_hist_kernel", 1.5), ("metrics_kernel", 3.0)):
            if key in name:
                avg_ns = float(row["AverageNs"])
                print("%-24s %3d calls  avg %9.1f us  min %9.1f  max %9.1f  %.3f TB/s (%.1f B x %d x %d samples per call)" % (
                    key, int(row["Calls"]), avg_ns / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3,
                    per_sample * w * h * n / avg_ns / 1e3, per_sample, n, w * h))


if __name__ == "__main__":
    {"fit": fit, "curve": curve, "kernel": kernel, "stats": stats}[sys.argv[1]](sys.argv[2:])
