"""Reference side of the device-metrics tests: the per-window SSIM values wrenc_amd/metrics.py's ssim_plane averages
(that function returns only their mean), the raw sums of include/wrenc_gpu.h's wrenc_gpu_metrics from numpy, and the
comparison rules the tests share."""
import numpy as np

from wrenc_amd import metrics


def ssim_windows(a, b):
    """The (h/4 - 1, w/4 - 1) f32 values of metrics.ssim_plane's windows, computed by its own expressions."""
    h, w = a.shape
    bw, bh = w >> 2, h >> 2
    a = a[:bh * 4, :bw * 4].astype(np.int64)
    b = b[:bh * 4, :bw * 4].astype(np.int64)

    def blocks(x):
        return x.reshape(bh, 4, bw, 4).sum(axis=(1, 3))

    def windows(x):
        return x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]

    s1, s2 = windows(blocks(a)), windows(blocks(b))
    ss, s12 = windows(blocks(a * a + b * b)), windows(blocks(a * b))
    var = ss * 64 - s1 * s1 - s2 * s2
    cov = s12 * 64 - s1 * s2
    f = np.float32
    c1, c2 = metrics._C1, metrics._C2
    return (f(1) * (2 * s1 * s2 + c1).astype(f) * (2 * cov + c2).astype(f)) / ((s1 * s1 + s2 * s2 + c1).astype(f) * (var + c2).astype(f))


def plane_sums(a, b):
    """(sse, per-window f32 array) of one plane pair."""
    d = a.astype(np.int64) - b.astype(np.int64)
    return int(np.sum(d * d)), ssim_windows(a, b)


def mean_bound(n_windows):
    """|device mean - numpy mean| of a plane: both add the same N f32 values of magnitude <= 1 + 2^-22 in double, each
    order off by at most (N - 1) 2^-53 sum |v|; divided by N and with the division's own rounding: 4 N 2^-53."""
    return 4.0 * n_windows * 2.0 ** -53


def check_raw(raw, org, rec, maps=None, refs=None):
    """A device record's raw sums (gpu.metrics_values(...)["_raw"]) against numpy for the planes (y, cb, cr) of org and
    rec: sse and window count exact, the mean within mean_bound, the maps (when given) bit for bit.  refs: per plane a
    precomputed plane_sums result or None."""
    for p in range(3):
        sse, win = refs[p] if refs is not None and refs[p] is not None else plane_sums(org[p], rec[p])
        n = win.size
        assert raw["sse"][p] == sse, (p, raw["sse"][p], sse)
        assert raw["ssim_windows"][p] == n == (org[p].shape[0] // 4 - 1) * (org[p].shape[1] // 4 - 1), p
        want = float(np.sum(win.astype(np.float64)) / n)     # metrics.ssim_plane's mean (test_metrics_abi.py holds the two together)
        got = raw["ssim_sum"][p] / n
        assert abs(got - want) <= mean_bound(n), (p, got, want, mean_bound(n))
        if maps is not None:
            assert maps[p].shape == win.shape and maps[p].dtype == np.float32
            assert np.array_equal(maps[p].view(np.uint32), win.astype(np.float32).view(np.uint32)), \
                (p, int(np.sum(maps[p].view(np.uint32) != win.view(np.uint32))))


def check_entry(entry, org, rec):
    """A download_metrics / report entry's values against metrics.frame_metrics: PSNR the same formula in doubles (1e-12
    relative, infinity for identical planes), SSIM planes within mean_bound, Avg = (4 Y + U + V) / 6 of its own planes."""
    want = metrics.frame_metrics(org, rec)
    for k in ("Avg", "Y", "U", "V"):
        g, w = entry["PSNR"][k], want["PSNR"][k]
        assert (g == w) if np.isinf(w) else abs(g - w) <= 1e-12 * abs(w), (k, g, w)
    for p, k in enumerate(("Y", "U", "V")):
        n = (org[p].shape[0] // 4 - 1) * (org[p].shape[1] // 4 - 1)
        assert abs(entry["SSIM"][k] - want["SSIM"][k]) <= mean_bound(n), (k, entry["SSIM"][k], want["SSIM"][k])
    s = entry["SSIM"]
    assert abs(s["Avg"] - (4.0 * s["Y"] + s["U"] + s["V"]) / 6.0) <= 1e-15
