"""What the source formats cost (the section on --input-format).  Needs an MI355X; there is no CPU path.

    python tools/format_probe.py device [--reps 30] [--out profiles/format_device.txt]
        3840x2160 in 3840x2176, from page-locked memory with the search idle: host clock around REPS uploads that end in one
        wrenc_gpu_sync, for every format -- raw copies + convert_format_kernel + pad + retile -- next to its yardstick, the
        plain yuv420p upload (copies + pad + retile) of the SAME BYTE COUNT on the same run: 3840x2160 for the 8-bit formats,
        3840x4320 for the 16-bit ones.  Per line: ms per picture, bytes over the bus per picture and per second.  The
        kernel's own time comes from running this mode under `rocprofv3 --kernel-trace --stats`.
    python tools/format_probe.py e2e [--frames 512] [--verbose] [--out profiles/format_e2e.txt]
        File to stream, 1920x1088 depth 2 QP 32, --batch 256 --threads 16: `wrenc --input-format yuv420p10le` on a 10-bit file
        once, and the same program three times on the file converted to 8 bits beforehand (the run-to-run spread); the
        streams must be the same bytes.  --verbose hands the program its own --verbose and keeps its account of every batch.
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


def raw_planes(fmt, y, cb, cr, rng):
    """8-bit 4:2:0 planes -> the planes of format `fmt` (a name) holding that picture: 10-bit words carry random low bits,
    4:2:2 chroma repeats every row."""
    lay = gpu.format_layout(fmt, y.shape[1], y.shape[0])
    if lay["rows"][1] == y.shape[0]:
        cb, cr = np.repeat(cb, 2, axis=0), np.repeat(cr, 2, axis=0)
    planes = [y, cb, cr]
    if lay["n_planes"] == 2:
        c = np.empty((cb.shape[0], 2 * cb.shape[1]), np.uint8)
        c[:, 0::2], c[:, 1::2] = cb, cr
        planes = [y, c]
    if lay["bytes_per_sample"] == 1:
        return [np.ascontiguousarray(p) for p in planes]
    out = []
    for p in planes:
        v = (p.astype(np.uint16) << 2) | rng.integers(0, 4, p.shape).astype(np.uint16)
        out.append(v << 6 if fmt == "p010le" else v)
    return out


def pinned(enc, planes):
    buf = enc.alloc_host(sum(p.nbytes for p in planes))
    out, at = [], 0
    for p in planes:
        v = buf[at:at + p.nbytes].view(p.dtype).reshape(p.shape)
        v[...] = p
        out.append(v)
        at += p.nbytes
    return out


def timed_uploads(enc, planes, reps):
    """ms per upload: host clock around reps uploads into slot 0, ended by one device synchronise."""
    for _ in range(3):
        enc.upload_planes(0, planes)
    enc.sync()
    t = time.perf_counter()
    for _ in range(reps):
        enc.upload_planes(0, planes)
    enc.sync()
    return (time.perf_counter() - t) * 1e3 / reps


def device(args):
    w, h = 3840, 2160
    pic = synth.synth_textured_frame(w, 2176, 1)
    pic = tuple(np.ascontiguousarray(p[:h >> (i > 0)]) for i, p in enumerate(pic))
    tall = tuple(np.ascontiguousarray(np.tile(p, (2, 1))) for p in pic)                  # 3840x4320: the bytes of a 16-bit frame
    rng = np.random.default_rng(1)
    lines = ["3840x2160, %d uploads + one sync, page-locked source: format: ms per picture | MB per picture | GB/s over the bus" % args.reps]

    def measure(label, width, height, fmt, planes):
        cw, ch = (width + 31) // 32 * 32, (height + 31) // 32 * 32
        enc = gpu.Encoder(cw, ch, qp=32, max_split_depth=2, n_slots=1, visible=(width, height) if (width, height) != (cw, ch) else None,
                          source_format=fmt)
        ms = timed_uploads(enc, pinned(enc, planes), args.reps)
        enc.close()
        mb = sum(p.nbytes for p in planes) / 1e6
        lines.append("%-34s %7.3f ms | %6.2f MB | %6.2f GB/s" % (label + ":", ms, mb, mb / ms))
        print(lines[-1], flush=True)
        return ms

    for run in range(2):                                   # twice: the second pass shows the run-to-run spread
        y8 = measure("yuv420p 3840x2160 (yardstick, 8-bit)", w, h, None, list(pic))
        y16 = measure("yuv420p 3840x4320 (yardstick, 16-bit)", w, 2 * h, None, list(tall))
        for fmt in ("nv12", "yuv422p", "yuv420p10le", "p010le", "yuv422p10le"):
            ms = measure(fmt + " 3840x2160", w, h, fmt, raw_planes(fmt, *pic, rng))
            base = y16 if gpu.format_layout(fmt, w, h)["bytes_per_sample"] == 2 else y8
            lines[-1] += " | %+.3f ms against its yardstick" % (ms - base)
            print("    " + lines[-1].rsplit("|", 1)[1].strip(), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def e2e(args):
    w, h, n = 1920, 1088, args.frames
    d = tempfile.mkdtemp(prefix="format_probe")
    ten, eight = os.path.join(d, "ten.yuv"), os.path.join(d, "eight.yuv")
    rng = np.random.default_rng(2)
    raw = []                                                # eight distinct frames, repeated: (10-bit bytes, converted bytes)
    for i in range(8):
        words = raw_planes("yuv420p10le", *synth.synth_frame(w, h, i), rng)
        conv = [((np.minimum(p, 1023) + 2) >> 2).clip(0, 255).astype(np.uint8) for p in words]       # include/wrenc_format.h
        raw.append((b"".join(p.astype("<u2").tobytes() for p in words), b"".join(p.tobytes() for p in conv)))
    with open(ten, "wb") as ft, open(eight, "wb") as fe:
        for i in range(n):
            ft.write(raw[i % 8][0])
            fe.write(raw[i % 8][1])
    common = ["--input-size", "%dx%d" % (w, h), "--output-size", "%dx%d" % (w, h), "--num-pictures", str(n), "--qp", "32",
              "--max-split-depth", "2", "--batch", "256", "--threads", "16"] + (["--verbose"] if args.verbose else [])
    lines, streams = [], {}
    for name, path, extra in (("8-bit", eight, []), ("10-bit", ten, ["--input-format", "yuv420p10le"]), ("8-bit", eight, []), ("8-bit", eight, [])):
        out = os.path.join(d, name + ".vvc")
        t = time.perf_counter()
        r = subprocess.run([NATIVE, "-i", path, "-o", out] + common + extra, capture_output=True)
        dt = time.perf_counter() - t
        if r.returncode or (r.stderr and not args.verbose):
            sys.exit("wrenc failed: %r" % r.stderr)
        streams[name] = open(out, "rb").read()
        lines.append("%-6s %d pictures in %.3f s = %.1f pictures/s (process start to exit), %d input bytes, %d stream bytes"
                     % (name, n, dt, n / dt, os.path.getsize(path), len(streams[name])))
        print(lines[-1], flush=True)
        if args.verbose:
            lines += ["    " + ln for ln in r.stderr.decode().splitlines()]
    lines.append("streams identical: %s" % (streams["10-bit"] == streams["8-bit"]))
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
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    device(a) if a.mode == "device" else e2e(a)
