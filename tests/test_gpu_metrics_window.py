"""Device-side PSNR / SSIM on a context with a visible size (include/wrenc_gpu.h: wrenc_gpu_download_metrics): the
figures are those of the visible rectangle, in tests/metrics_ref.py's comparison rules -- squared errors and window counts
exact, a plane's SSIM mean within 4 N 2^-53 -- and a context without a visible size still gives the sums of the plain
pass."""
import numpy as np
import pytest

import metrics_ref
from window_stream import SIZE_IDS, SIZES, crop_planes, pad_planes, textured

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("visible,coded", SIZES, ids=SIZE_IDS)
def test_metrics_are_those_of_the_visible_rectangle(built, visible, coded):
    from wrenc_amd import gpu
    (vw, vh), (cw, ch) = visible, coded
    pic = textured(vw, vh, 5)
    enc = gpu.Encoder(cw, ch, qp=32, max_split_depth=2, n_slots=3, visible=visible)
    for slot in (0, 2):
        enc.upload(slot, *pic)
    enc.upload(1, *textured(vw, vh, 6))
    enc.encode(0, 3)
    got = enc.download_metrics(0, 3)
    d = enc.download(0)
    full = (d["rec_y"], d["rec_cb"], d["rec_cr"])
    rec = crop_planes(full, vw, vh)
    raw = got[0]["_raw"]
    # the exact squared error of the cropped pair, the window count of the formula, the SSIM mean of the cropped planes
    for p in range(3):
        ph, pw = pic[p].shape
        diff = pic[p].astype(np.int64) - rec[p].astype(np.int64)
        assert raw["sse"][p] == int(np.sum(diff * diff)), p
        assert raw["ssim_windows"][p] == ((pw >> 2) - 1) * ((ph >> 2) - 1), p
    metrics_ref.check_raw(raw, pic, rec)
    metrics_ref.check_entry(got[0], pic, rec)
    # ... and not the figure of the coded picture, whose margin is coded too
    padded = pad_planes(pic, cw, ch)
    coded_sse = [int(np.sum((a.astype(np.int64) - b.astype(np.int64)) ** 2)) for a, b in zip(padded, full)]
    assert raw["sse"] != coded_sse and all(c >= v for c, v in zip(coded_sse, raw["sse"]))
    # the same picture in another slot and in a call of its own: the same bytes; another picture: other bytes
    assert got[2]["_raw"]["bytes"] == raw["bytes"] != got[1]["_raw"]["bytes"]
    assert enc.download_metrics(2, 1)[0]["_raw"]["bytes"] == raw["bytes"]
    enc.close()


@pytest.mark.parametrize("cw,ch", sorted({c for _, c in SIZES}))
def test_without_a_visible_size_the_sums_are_the_plain_ones(built, cw, ch):
    """A context of the coded size on which no visible size is set -- and one on which it was set back to the coded size --
    reports exactly what wrenc_gpu_test_metrics gives on the same planes at full size."""
    from wrenc_amd import gpu
    pic = textured(cw, ch, 8)
    records = []
    for visible in (None, (cw - 2, ch - 2)):
        enc = gpu.Encoder(cw, ch, qp=32, max_split_depth=2, visible=visible)
        if visible is not None:
            enc.set_visible_size(cw, ch)
        d = enc.encode_picture(*pic)
        rec = (d["rec_y"], d["rec_cb"], d["rec_cr"])
        got = enc.download_metrics(0, 1)[0]
        direct = enc.test_metrics(pic, rec)
        assert got["_raw"]["bytes"] == direct["_raw"]["bytes"]
        metrics_ref.check_raw(got["_raw"], pic, rec)
        records.append(got["_raw"]["bytes"])
        enc.close()
    assert records[0] == records[1]
