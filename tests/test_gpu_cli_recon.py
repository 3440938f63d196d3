"""--reconst-format of the command line (wrenc_amd/csrc/host/wrenc_main.cpp): one short --pad run at 50x40 per format.  The
yuv420p file is the file of a run without the option, the RGB files are the library's host converter (include/wrenc_recon.h)
of that file, frame by frame -- the output is a function of the visible reconstruction alone -- and the stream never depends
on these options."""
import os
import subprocess

import numpy as np
import pytest

import recon_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
W, H, N, QP = 50, 40, 3, 32


def _run(args):
    r = subprocess.run([NATIVE] + args, cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    return r


def test_reconst_formats(built, tmp_path):
    from wrenc_amd import gpu
    frames = []
    for i in range(N):
        y, cb, cr = rr.noise(W, H, 60 + i)
        y = (y // 4 + np.indices((H, W))[1] * 3 + 10 * i).astype(np.uint8)
        frames.append(y.tobytes() + cb.tobytes() + cr.tobytes())
    src = tmp_path / "in.yuv"
    src.write_bytes(b"".join(frames))
    outs = {}
    for tag, option in (("plain", []), ("yuv420p", ["--reconst-format", "yuv420p"]), ("rgb24", ["--reconst-format", "rgb24"]),
                        ("bgr0", ["--reconst-format", "bgr0", "--reconst-colorspace", "bt601", "--reconst-range", "pc"])):
        out, rec = tmp_path / (tag + ".vvc"), tmp_path / (tag + ".rec")
        _run(["-i", str(src), "-o", str(out), "-r", str(rec), "--pad", "--input-size", "%dx%d" % (W, H), "--output-size", "%dx%d" % (W, H),
              "--num-pictures", str(N), "--qp", str(QP), "--max-split-depth", "2", "--batch", "2"] + option)
        outs[tag] = (out.read_bytes(), rec.read_bytes())
    stream, yuv = outs["plain"]
    per = W * H * 3 // 2
    assert len(stream) > 200 and len(yuv) == N * per
    for tag in outs:
        assert outs[tag][0] == stream, tag                      # the stream never depends on the options
    assert outs["yuv420p"][1] == yuv
    for tag, matrix, rng, bpp in (("rgb24", "bt709", "tv", 3), ("bgr0", "bt601", "pc", 4)):
        got = outs[tag][1]
        assert len(got) == N * W * H * bpp, tag
        for i in range(N):
            f = np.frombuffer(yuv[i * per:(i + 1) * per], np.uint8)
            y, cb, cr = f[:W * H].reshape(H, W), f[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), f[W * H * 5 // 4:].reshape(H // 2, W // 2)
            want = gpu.recon_convert_host(tag, matrix, rng, W, H, y, cb, cr)[0]
            assert got[i * W * H * bpp:(i + 1) * W * H * bpp] == want.tobytes(), (tag, i)
            assert np.array_equal(want, rr.convert(rr.NAMES.index(tag), rr.BT601 if matrix == "bt601" else rr.BT709,
                                                   rr.PC if rng == "pc" else rr.TV, y, cb, cr)[0])
