"""What RGB sources and device-resident pictures cost.  Needs an MI355X and torch; there is no CPU path.

    python tools/rgb_probe.py kernels [--reps 30]
        3840x2160 in 3840x2176: REPS uploads of a device-resident picture for every RGB layout and, as the yardstick, for
        yuv420p10le -- a pass of the same shape.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/rgb_probe.py
        kernels`: the kernels' own times are in the statistics; `python tools/rgb_probe.py bytes` prints the bytes each
        converter must move, to put beside them.
    python tools/rgb_probe.py device [--reps 20] [--out profiles/rgb_device.txt]
        "tensor ready" to "slot uploaded" for a 3840x2160 rgb24 picture: torch_source.upload_tensor against
        t.cpu().numpy() + upload_rgb, host clock around REPS rounds, each ended by wrenc_gpu_sync.
    python tools/rgb_probe.py e2e [--frames 512] [--native PATH] [--out profiles/rgb_e2e.txt]
        File to stream, 1920x1088 depth 2 QP 32, --batch 256 --threads 16: the program on an rgb24 file, on the yuv420p file
        of the same pictures (converted by the library's host converter) three times -- the run-to-run spread -- and on a
        yuv420p10le file of them.  --native names another build of the program (the parent commit's) for the yuv420p runs.
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
LAYOUTS = ("rgb24", "bgr24", "rgb0", "bgr0", "gbrp")
W, H, CH = 3840, 2160, 2176


def rgb_frame(w, h, i):
    """(h, w, 3) uint8: a synthetic picture's planes taken as R, G and B."""
    y, cb, cr = synth.synth_frame(w, (h + 31) // 32 * 32, i)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    return np.ascontiguousarray(np.stack([y[:h], up(cb)[:h], up(cr)[:h]], axis=2))


def pack(layout, rgb):
    """The planes of `layout` as one array or a list of three."""
    if layout == "gbrp":
        return [np.ascontiguousarray(rgb[:, :, c]) for c in (1, 2, 0)]
    order = (2, 1, 0) if layout.startswith("bgr") else (0, 1, 2)
    n = 4 if layout.endswith("0") else 3
    out = np.zeros(rgb.shape[:2] + (n,), np.uint8)
    for k, c in enumerate(order):
        out[:, :, k] = rgb[:, :, c]
    return out.reshape(rgb.shape[0], rgb.shape[1] * n)


def bytes_moved():
    for name in LAYOUTS + ("yuv420p10le",):
        read = W * H * 3 if name == "yuv420p10le" else sum(gpu.rgb_layout(name, W, H)["row_bytes"]) * H
        print("%-12s reads %6.2f MB, writes %5.2f MB: %6.2f MB" % (name, read / 1e6, W * H * 1.5 / 1e6, (read + W * H * 1.5) / 1e6))


def kernels(args):
    import torch
    from wrenc_amd import torch_source
    rgb = rgb_frame(W, H, 1)
    for name in LAYOUTS:
        enc = gpu.Encoder(W, CH, qp=32, max_split_depth=2, visible=(W, H), source_rgb=(name, "bt709", "tv"))
        if name == "gbrp":
            t = torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1))).cuda()
        else:
            t = torch.from_numpy(pack(name, rgb).reshape(H, W, -1)).cuda()
        for _ in range(args.reps):
            torch_source.upload_tensor(enc, 0, t)
        enc.sync()
        enc.close()
    y, cb, cr = (torch.from_numpy(p.astype(np.int16) << 2).cuda() for p in synth.synth_frame(W, CH, 1))
    enc = gpu.Encoder(W, CH, qp=32, max_split_depth=2, visible=(W, H), source_format="yuv420p10le")
    for _ in range(args.reps):
        torch_source.upload_tensor(enc, 0, (y[:H], cb[:H // 2], cr[:H // 2]))
    enc.sync()
    enc.close()
    print("%d uploads per layout done" % args.reps)


def device(args):
    import torch
    from wrenc_amd import torch_source
    rgb = rgb_frame(W, H, 1)
    t = torch.from_numpy(rgb).cuda()
    enc = gpu.Encoder(W, CH, qp=32, max_split_depth=2, visible=(W, H), source_rgb=("rgb24", "bt709", "tv"))
    lines = ["3840x2160 rgb24 (24.88 MB), tensor ready -> slot uploaded, %d rounds each ended by wrenc_gpu_sync: ms per picture" % args.reps]

    def resident():
        torch_source.upload_tensor(enc, 0, t)

    def through_host():
        enc.upload_rgb(0, t.cpu().numpy().reshape(H, 3 * W))

    for run in range(3):                                    # three passes: the run-to-run spread
        for label, fn in (("upload_tensor (device to device)", resident), ("t.cpu().numpy() + upload_rgb", through_host)):
            for _ in range(3):
                fn()
                enc.sync()
            torch.cuda.synchronize()
            s = time.perf_counter()
            for _ in range(args.reps):
                fn()
                enc.sync()
            lines.append("%-36s %8.3f ms" % (label + ":", (time.perf_counter() - s) * 1e3 / args.reps))
            print(lines[-1], flush=True)
    enc.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def e2e(args):
    w, h, n = 1920, 1088, args.frames
    d = tempfile.mkdtemp(prefix="rgb_probe")
    paths = {k: os.path.join(d, k + ".raw") for k in ("rgb24", "yuv420p", "yuv420p10le")}
    frames = []                                             # eight distinct frames, repeated
    for i in range(8):
        rgb = rgb_frame(w, h, i)
        conv = gpu.rgb_convert_host("rgb24", "bt709", "tv", w, h, rgb.reshape(h, 3 * w))
        frames.append((rgb.tobytes(), b"".join(p.tobytes() for p in conv), b"".join((p.astype("<u2") << 2).tobytes() for p in conv)))
    files = {k: open(p, "wb") for k, p in paths.items()}
    for i in range(n):
        for k, data in zip(("rgb24", "yuv420p", "yuv420p10le"), frames[i % 8]):
            files[k].write(data)
    for f in files.values():
        f.close()
    common = ["--input-size", "%dx%d" % (w, h), "--output-size", "%dx%d" % (w, h), "--num-pictures", str(n), "--qp", "32",
              "--max-split-depth", "2", "--batch", "256", "--threads", "16"]
    runs = [("yuv420p", [], NATIVE), ("rgb24", ["--input-format", "rgb24"], NATIVE), ("yuv420p10le", ["--input-format", "yuv420p10le"], NATIVE),
            ("yuv420p", [], NATIVE), ("yuv420p", [], NATIVE)]
    if args.native:
        runs += [("yuv420p", [], args.native)] * 3
    lines, streams = [], {}
    for name, extra, exe in runs:
        out = os.path.join(d, name + ".vvc")
        s = time.perf_counter()
        r = subprocess.run([exe, "-i", paths[name], "-o", out, "--verbose"] + common + extra, capture_output=True)
        dt = time.perf_counter() - s
        own = [ln for ln in r.stderr.decode().splitlines() if "file to stream" in ln]       # the program's own clock
        if r.returncode or b"error" in r.stderr or not own:
            sys.exit("wrenc failed: %r" % r.stderr)
        streams.setdefault(name, set()).add(open(out, "rb").read())
        lines.append("%-12s %-8s process start to exit %.3f s; own clock: %s" % (name, "this" if exe == NATIVE else "--native", dt, own[-1]))
        print(lines[-1], flush=True)
    lines.append("streams identical: %s" % (len(set.union(*streams.values())) == 1))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    os.rmdir(d)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "bytes", "device", "e2e"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--native")
    ap.add_argument("--out")
    a = ap.parse_args()
    {"kernels": kernels, "bytes": lambda _: bytes_moved(), "device": device, "e2e": e2e}[a.mode](a)
