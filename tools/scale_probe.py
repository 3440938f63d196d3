"""What scaling on the device costs (the section on --scale).  Needs an MI355X; there is no CPU path.

    python tools/scale_probe.py device [--reps 30] [--out profiles/scale_device.txt]
        Per size pair, from page-locked memory with the search idle, host clock around REPS uploads that end in
        wrenc_gpu_sync: a scaling context (copies of the source planes + scale_kernel + pad + retile) next to a plain
        context of the output size (copies of the output-size planes + pad + retile), the bytes each moves, and the
        search's device time per picture at the output size (depth 2, QP 32, wrenc_gpu_last_encode_stats).  The kernel's own
        time comes from running this mode under `rocprofv3 --kernel-trace --stats` (scale_kernel in the kernel table).
    python tools/scale_probe.py e2e [--frames 96] [--out profiles/scale_e2e.txt]
        File to stream: `wrenc --scale` from a 3840x2160 file to 1920x1080 --pad against the same program without --scale
        on the file the device pre-scaled (a context without a source size launches what the parent commit launches), same
        options, three runs each, alternating; the two streams must be the same bytes.
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wrenc_amd import gpu, synth  # noqa: E402

NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
PAIRS = [((3840, 2160), (1920, 1080)), ((1920, 1080), (1280, 720)), ((7680, 4320), (1920, 1080))]


def coded(w, h):
    return (w + 31) // 32 * 32, (h + 31) // 32 * 32


def frame(w, h, seed):
    """A textured frame of any even size: the synthetic 1088p / 2176p texture tiled and cropped."""
    cw, ch = coded(w, h)
    y, cb, cr = synth.synth_textured_frame(min(cw, 3840), min(ch, 2176), seed)
    reps = ((ch + y.shape[0] - 1) // y.shape[0], (cw + y.shape[1] - 1) // y.shape[1])
    return (np.ascontiguousarray(np.tile(y, reps)[:h, :w]), np.ascontiguousarray(np.tile(cb, reps)[:h // 2, :w // 2]),
            np.ascontiguousarray(np.tile(cr, reps)[:h // 2, :w // 2]))


def pinned_planes(enc, planes):
    buf = enc.alloc_host(sum(p.size for p in planes))
    out, at = [], 0
    for p in planes:
        v = buf[at:at + p.size].reshape(p.shape)
        v[...] = p
        out.append(v)
        at += p.size
    return out


def timed_uploads(enc, planes, reps):
    """ms per upload: host clock around reps uploads into slot 0, ended by a device synchronise."""
    for _ in range(3):
        enc.upload_strided(0, *planes)
    enc.sync()
    t = time.perf_counter()
    for _ in range(reps):
        enc.upload_strided(0, *planes)
    enc.sync()
    return (time.perf_counter() - t) * 1e3 / reps


def device(args):
    lines = ["source -> output (coded): ms per upload, scaling context | plain context of the output size | difference; "
             "bytes in + out; search ms per picture (depth 2, QP 32, 8 pictures in flight); difference / search"]
    for src, dst in PAIRS:
        cw, ch = coded(*dst)
        vis = dst if dst != (cw, ch) else None
        pic = frame(*src, 1)
        enc = gpu.Encoder(cw, ch, qp=32, max_split_depth=2, n_slots=8, visible=vis, source=src)
        t_scale = timed_uploads(enc, pinned_planes(enc, pic), args.reps)
        small = [np.ascontiguousarray(p[:dst[1] >> (i > 0), :dst[0] >> (i > 0)]) for i, p in enumerate(enc.download_originals(0))]
        enc.close()
        plain = gpu.Encoder(cw, ch, qp=32, max_split_depth=2, n_slots=8, visible=vis)
        pp = pinned_planes(plain, small)
        t_plain = timed_uploads(plain, pp, args.reps)
        for s in range(8):
            plain.upload_strided(s, *pp)
        plain.stats_enable(True)
        for _ in range(2):
            plain.encode(0, 8)
            plain.sync()
        search = plain.last_encode_stats()["total_ms"] / 8
        plain.close()
        moved = src[0] * src[1] * 3 // 2 + dst[0] * dst[1] * 3 // 2
        lines.append("%dx%d -> %dx%d (%dx%d): %.3f | %.3f | %.3f ms; %.1f MB, %.1f GB/s over the difference; search %.2f ms; %.2f %%"
                     % (src + dst + (cw, ch) + (t_scale, t_plain, t_scale - t_plain, moved / 1e6,
                                                moved / 1e6 / max(t_scale - t_plain, 1e-6), search, 100 * (t_scale - t_plain) / search)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def e2e(args):
    src, dst, n = (3840, 2160), (1920, 1080), args.frames
    cw, ch = coded(*dst)
    d = tempfile.mkdtemp(prefix="scale_probe")
    big, small = os.path.join(d, "big.yuv"), os.path.join(d, "small.yuv")
    enc = gpu.Encoder(cw, ch, qp=32, max_split_depth=2, visible=dst, source=src)
    raw = []                                            # four distinct frames, repeated: (source bytes, scaled bytes)
    for i in range(4):
        pic = frame(*src, i)
        enc.upload(0, *pic)
        scaled = [np.ascontiguousarray(p[:dst[1] >> (k > 0), :dst[0] >> (k > 0)]) for k, p in enumerate(enc.download_originals(0))]
        raw.append((b"".join(p.tobytes() for p in pic), b"".join(p.tobytes() for p in scaled)))
    enc.close()
    with open(big, "wb") as fb, open(small, "wb") as fs:
        for i in range(n):
            fb.write(raw[i % 4][0])
            fs.write(raw[i % 4][1])
    common = ["--input-size", "%dx%d" % src, "--output-size", "%dx%d" % dst, "--pad", "--num-pictures", str(n), "--qp", "32",
              "--max-split-depth", "2", "--batch", "16", "--threads", "16"]
    lines, streams = [], {}
    for run in range(3):
        for name, path, extra in (("scale", big, ["--scale"]), ("prescaled", small, [])):
            out = os.path.join(d, name + ".vvc")
            t = time.perf_counter()
            r = subprocess.run([NATIVE, "-i", path, "-o", out] + common + extra, capture_output=True)
            dt = time.perf_counter() - t
            if r.returncode or r.stderr:
                sys.exit("wrenc failed: %r" % r.stderr)
            streams[name] = open(out, "rb").read()
            lines.append("run %d %-9s %d pictures in %.3f s = %.1f pictures/s (process start to exit), %d stream bytes"
                         % (run + 1, name, n, dt, n / dt, len(streams[name])))
            print(lines[-1], flush=True)
    lines.append("streams identical: %s" % (streams["scale"] == streams["prescaled"]))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    os.rmdir(d)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["device", "e2e"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--out")
    a = ap.parse_args()
    device(a) if a.mode == "device" else e2e(a)
