"""bench.py --dump-outputs on the CPU: what dump_outputs writes for the headline workload's shape, from a stand-in
encoder whose records are a known function of the slot."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Records:
    """enc.download(slot) of the real encoder, with every plane filled from the slot number."""

    def __init__(self, w, h):
        from wrenc_amd import gpu
        self.w, self.h = w, h
        self.alloc = gpu.alloc_picture
        self.downloads = []

    def download(self, slot):
        self.downloads.append(slot)
        rec = self.alloc(self.w, self.h)
        for i, (k, a) in enumerate(sorted(rec.items())):
            flat = a.reshape(-1)
            flat[:] = (np.arange(flat.size) * (slot + 1) + 7 * i) % (251 if a.dtype == np.uint8 else 30011)
        return rec


def test_dump_outputs_headline_shape(tmp_path):
    import bench
    w, h, n_slots = bench.HEADLINE["w"], bench.HEADLINE["h"], bench.HEADLINE["batch"]
    enc = _Records(w, h)
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(enc, n_slots, str(a))
    assert info["slots"] == sorted(set(info["slots"])) and len(info["slots"]) == bench.DUMP_PICTURES
    assert all(0 <= s < n_slots for s in info["slots"]) and enc.downloads == info["slots"]
    assert bench.dump_outputs(_Records(w, h), n_slots, str(b))["slots"] == info["slots"]
    total = 0
    for k in bench.REC_KEYS:
        x, y = np.load(a / (k + ".npy")), np.load(b / (k + ".npy"))
        assert x.dtype == np.float32 and x.shape[0] == len(info["slots"]), k
        assert np.array_equal(x, y), k         # same arguments: same positions, same values
        total += os.path.getsize(a / (k + ".npy"))
    assert np.load(a / "ctu_cost.npy").shape[1] == (w // 32) * (h // 32)     # whole
    assert total <= 64 << 20 and info["bytes"] <= total


def test_dump_outputs_small_batch(tmp_path):
    import bench
    enc = _Records(64, 64)
    info = bench.dump_outputs(enc, 3, str(tmp_path))
    assert info["slots"] == [0, 1, 2]
    for k in bench.REC_KEYS:        # planes smaller than the sample cap are dumped whole, in order
        x = np.load(tmp_path / (k + ".npy"))
        for row, slot in zip(x, info["slots"]):
            assert np.array_equal(row, enc.download(slot)[k].reshape(-1).astype(np.float32)), k


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr
