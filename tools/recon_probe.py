"""What the reconstruction costs on its way out.  Needs an MI355X and torch; there is no CPU path.

    python tools/recon_probe.py kernels [--reps 30]
        3840x2160 in 3840x2176, search idle: REPS download_tensor calls for every output format and, as the yardstick in the
        same run, REPS rgb24 uploads of a device-resident picture (convert_rgb_kernel<rgb24> moves the same bytes the other
        way).  Run it under `rocprofv3 --kernel-trace --stats -- python tools/recon_probe.py kernels`: the kernels' own times
        are in the statistics; `python tools/recon_probe.py bytes` prints the bytes each kernel must move, to put beside them.
    python tools/recon_probe.py device [--reps 20] [--out profiles/recon_device.txt]
        "encode finished" to "tensor ready" for one 3840x2160 picture: torch_source.download_tensor("rgb24") against
        download + host crop + a torch colour conversion + .cuda(); three passes, host clock, no profiler.
    python tools/recon_probe.py e2e [--frames 512] [--native PATH] [--out profiles/recon_e2e.txt]
        File to stream, 1920x1080 --pad depth 2 QP 32, --batch 256 --threads 16, three runs each: no --reconst, --reconst
        plain, --reconst --reconst-format rgb24; --native names another build of the program (the parent commit's) for three
        more runs without --reconst.
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
FORMATS = ("rgb24", "bgr24", "rgb0", "bgr0", "gbrp", "yuv420p", "nv12")
W, H, CH = 3840, 2160, 2176


def bytes_moved():
    for name in FORMATS:
        write = gpu.recon_layout(name, W, H)["frame_bytes"]
        print("%-8s reads %5.2f MB, writes %5.2f MB: %6.2f MB" % (name, W * H * 1.5 / 1e6, write / 1e6, (W * H * 1.5 + write) / 1e6))
    print("%-8s reads %5.2f MB, writes %5.2f MB: %6.2f MB   (convert_rgb_kernel<rgb24>, the yardstick)"
          % ("upload", W * H * 3 / 1e6, W * H * 1.5 / 1e6, W * H * 4.5 / 1e6))


def loaded_encoder(**kw):
    """A 3840x2176 context with visible 3840x2160 whose slot 0 holds a synthetic reconstruction, marked encoded."""
    enc = gpu.Encoder(W, CH, qp=32, max_split_depth=2, visible=(W, H), **kw)
    enc.test_load_recon(0, *synth.synth_frame(W, CH, 1))
    return enc


def kernels(args):
    import torch
    from wrenc_amd import torch_source
    enc = loaded_encoder()
    for name in FORMATS:
        for _ in range(args.reps):
            out = torch_source.download_tensor(enc, 0, name)
        torch.cuda.synchronize()
        del out
    enc.close()
    y, cb, cr = synth.synth_frame(W, CH, 1)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    t = torch.from_numpy(np.ascontiguousarray(np.stack([y[:H], up(cb)[:H], up(cr)[:H]], axis=2))).cuda()
    enc = gpu.Encoder(W, CH, qp=32, max_split_depth=2, visible=(W, H), source_rgb=("rgb24", "bt709", "tv"))
    for _ in range(args.reps):
        torch_source.upload_tensor(enc, 0, t)
    enc.sync()
    enc.close()
    print("%d calls per format done" % args.reps)


def device(args):
    import torch
    from wrenc_amd import torch_source
    enc = loaded_encoder()
    k = gpu.recon_coefficients("bt709", "tv")
    lines = ["3840x2160 in 3840x2176, slot encoded -> rgb24 tensor on the device, %d rounds each ended by torch.cuda.synchronize: ms per picture" % args.reps]

    def resident():
        return torch_source.download_tensor(enc, 0, "rgb24")

    def through_host():
        # the planes over the bus, a host crop, torch's own conversion (nearest chroma, float): another definition
        rec = enc.download(0, keys=("rec_y", "rec_cb", "rec_cr"))
        y = torch.from_numpy(rec["rec_y"][:H, :W].astype(np.float32))
        u = torch.from_numpy(rec["rec_cb"][:H // 2, :W // 2].astype(np.float32)).repeat_interleave(2, 0).repeat_interleave(2, 1) - 128
        v = torch.from_numpy(rec["rec_cr"][:H // 2, :W // 2].astype(np.float32)).repeat_interleave(2, 0).repeat_interleave(2, 1) - 128
        yd = (y - k[5]) * (k[0] / 16384.0)
        rgb = torch.stack([yd + v * (k[1] / 16384.0), yd + u * (k[2] / 16384.0) + v * (k[3] / 16384.0), yd + u * (k[4] / 16384.0)], dim=2)
        return (rgb.clamp(0, 255) + 0.5).to(torch.uint8).cuda()

    for run in range(3):                                    # three passes: the run-to-run spread
        for label, fn in (("download_tensor (device to device)", resident), ("download + crop + torch + .cuda()", through_host)):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            s = time.perf_counter()
            for _ in range(args.reps):
                fn()
                torch.cuda.synchronize()
            lines.append("%-36s %8.3f ms" % (label + ":", (time.perf_counter() - s) * 1e3 / args.reps))
            print(lines[-1], flush=True)
    enc.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def e2e(args):
    w, h, n = 1920, 1080, args.frames
    d = tempfile.mkdtemp(prefix="recon_probe")
    src = os.path.join(d, "in.yuv")
    frames = [b"".join(p[:(h if k == 0 else h // 2)].tobytes() for k, p in enumerate(synth.synth_frame(w, 1088, i))) for i in range(8)]
    with open(src, "wb") as f:                              # eight distinct frames, repeated
        for i in range(n):
            f.write(frames[i % 8])
    common = ["-i", src, "--pad", "--input-size", "%dx%d" % (w, h), "--output-size", "%dx%d" % (w, h), "--num-pictures", str(n), "--qp", "32",
              "--max-split-depth", "2", "--batch", "256", "--threads", "16", "--verbose"]
    rec = os.path.join(d, "rec.raw")
    runs = []
    for _ in range(3):
        runs += [("no --reconst", [], NATIVE), ("--reconst", ["-r", rec], NATIVE), ("--reconst rgb24", ["-r", rec, "--reconst-format", "rgb24"], NATIVE)]
        if args.native:
            runs.append(("no --reconst", [], args.native))
    lines, streams = [], set()
    for name, extra, exe in runs:
        out = os.path.join(d, "out.vvc")
        s = time.perf_counter()
        r = subprocess.run([exe, "-o", out] + common + extra, capture_output=True)
        dt = time.perf_counter() - s
        own = [ln for ln in r.stderr.decode().splitlines() if "file to stream" in ln]       # the program's own clock
        if r.returncode or b"error" in r.stderr or not own:
            sys.exit("wrenc failed: %r" % r.stderr)
        streams.add(open(out, "rb").read())
        lines.append("%-16s %-8s process start to exit %.3f s; own clock: %s" % (name, "this" if exe == NATIVE else "--native", dt, own[-1]))
        print(lines[-1], flush=True)
    lines.append("streams identical: %s" % (len(streams) == 1))
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
