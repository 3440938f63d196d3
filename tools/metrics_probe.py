"""Rate of the metrics pass next to the compact read-back's kernel, which moves the same 3 bytes per luma sample:
N resident pictures after one encode call, download_compact and download_metrics a few times each, warmed up.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python3 tools/metrics_probe.py [WxH=1920x1088] [N=256] [REPS=4]
    python3 tools/metrics_probe.py --stats DIR/.../*_kernel_stats.csv [WxH] [N]      # bytes per second of both kernels

Kernel times come from the trace (a run of its own, no counters); the wall times printed by the run itself include the
copies and the host side of the calls."""
import csv
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _args(argv):
    w, h = [int(v) for v in (argv[0] if argv else "1920x1088").split("x")]
    return w, h, int(argv[1]) if len(argv) > 1 else 256, int(argv[2]) if len(argv) > 2 else 4


def summarise(path, argv):
    w, h, n, _ = _args(argv)
    moved = 3.0 * w * h * n
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        if "metrics_kernel" in name or "compact_levels_kernel" in name or "metrics_finish_kernel" in name:
            avg_ns = float(row["AverageNs"])
            rate = "" if "finish" in name else "  %.3f TB/s (3 B x %d x %d samples per call)" % (moved / avg_ns / 1e3, n, w * h)
            print("%-40s %3d calls  avg %9.1f us  min %9.1f  max %9.1f%s" % (
                name.split("(")[0][-40:], int(row["Calls"]), avg_ns / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3, rate))


def main(argv):
    from wrenc_amd import gpu, synth
    w, h, n, reps = _args(argv)
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=n)
    frames = [synth.synth_frame(w, h, f) for f in range(8)]
    for s in range(n):
        enc.upload(s, *frames[s % 8])
    enc.encode(0, n)
    enc.sync()
    for rep in range(reps + 1):      # the first round warms up
        t0 = time.perf_counter()
        enc.download_compact(0, n)
        tc = time.perf_counter() - t0
        t0 = time.perf_counter()
        m = enc.download_metrics(0, n)
        tm = time.perf_counter() - t0
        print("%dx%d, %d pictures: compact read-back %.1f ms, metrics read-back %.2f ms (PSNR Y of picture 0: %.3f dB)%s"
              % (w, h, n, tc * 1e3, tm * 1e3, m[0]["PSNR"]["Y"], "  [warm-up]" if rep == 0 else ""), flush=True)
    enc.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        summarise(sys.argv[2], sys.argv[3:])
    else:
        main(sys.argv[1:])
