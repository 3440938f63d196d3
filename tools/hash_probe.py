"""Time of the decoded picture hash passes (wrenc_amd/csrc/dev_hash.h): N resident pictures after one encode call, then
download_hashes of all N a few times per type with HIP events around the pass's kernels (wrenc_gpu_last_hash_ms).

    python3 tools/hash_probe.py [WxH=1920x1088] [N=256] [REPS=4]

Prints per type the best and median device time of a call, the bytes it read per second (1.5 bytes per luma sample and
picture) and that rate's share of the 8 TB/s HBM peak, and the wall time of the blocking call."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def main(argv):
    from wrenc_amd import gpu, synth
    w, h = [int(v) for v in (argv[0] if argv else "1920x1088").split("x")]
    n = int(argv[1]) if len(argv) > 1 else 256
    reps = int(argv[2]) if len(argv) > 2 else 4
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=n)
    frames = [synth.synth_frame(w, h, f) for f in range(8)]
    for s in range(n):
        enc.upload(s, *frames[s % 8])
    enc.encode(0, n)
    enc.sync()
    enc.stats_enable()
    moved = 1.5 * w * h * n
    for name in ("checksum", "crc", "md5"):
        ms, wall = [], []
        for rep in range(reps + 1):      # the first round warms up (and makes the pass's stream, tables and scratch)
            t0 = time.perf_counter()
            got = enc.download_hashes(0, n, name)
            dt = time.perf_counter() - t0
            if rep:
                ms.append(enc.last_hash_ms())
                wall.append(dt * 1e3)
        ms.sort()
        best, med = ms[0], ms[len(ms) // 2]
        print("%dx%d, %d pictures, %-8s: %9.3f ms best, %9.3f ms median per call (wall %.3f ms); %.3f TB/s = %.1f %% of HBM peak; "
              "picture 0 Y: %s" % (w, h, n, name, best, med, min(wall), moved / (best * 1e-3) / 1e12,
                                   100.0 * moved / (best * 1e-3) / HBM_PEAK, got[0].values(name)[0].hex()), flush=True)
    enc.close()


if __name__ == "__main__":
    main(sys.argv[1:])
