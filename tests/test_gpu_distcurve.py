"""The device's distortion curve (include/wrenc_gpu.h: wrenc_gpu_download_dist_curve; the kernel is
wrenc_amd/csrc/dev_distcurve.h) against tests/distcurve_ref.py's numpy restatement of include/wrenc_distcurve.h, bit for
bit: at every seam of the kernel's layout (the rate histogram's: a wave is a strip of 16 CTUs of one CTU row; a lane owns
the luma blocks of rows 0 | 1, then 2 | 3 of that CTU row, then one Cb | Cr pair; here two waves a workgroup), on content
whose every coefficient is at the magnitude bound, on padded, converted and scaled pictures, and the call's behaviour as an
API."""
import numpy as np
import pytest

import distcurve_ref as dr
import format_ref
import ratecurve_ref as rr
import scale_ref
from content import content
from window_stream import pad_planes

pytestmark = pytest.mark.gpu

# one CTU (every block on a picture edge); two; 3 x 2 CTUs; 17 CTUs in a row: one more than a wave's strip
SIZES = [(32, 32), (64, 32), (96, 64), (544, 32)]
KINDS = ["ramp", "stripes30", "checker", "cclm", "extremes"]
ESTATE, EINVAL = -5, -1
KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")


def half_step(w, h):
    """Flat 255 but for columns 0 and 4 of every block at an odd (bx, by), which are 27: such a block is predicted as 255
    from flat neighbours, its residual -228 (1 + (-1)^x)(1 + (-1)^(x >> 1)) / 4 is four equal coefficients, 0 .. 3, of
    -3648: m = 29,184 = T(63) / 2 exactly, the largest error there is, four times in one 32-bit partial of the kernel."""
    def plane(hh, ww):
        p = np.full((hh, ww), 255, np.uint8)
        yy, xx = np.mgrid[0:hh, 0:ww]
        p[((xx >> 3) & 1 == 1) & ((yy >> 3) & 1 == 1) & (xx & 3 == 0)] = 27
        return p
    return plane(h, w), plane(h // 2, w // 2), plane(h // 2, w // 2)


def _pictures(w, h):
    return [content(k, w, h, 3) for k in KINDS] + [rr.flat(w, h), rr.checker8(w, h), rr.noise(w, h, 7), half_step(w, h)]


def _check(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "(plane, qp)", bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("w,h", SIZES)
def test_content_against_numpy(built, w, h):
    """All pictures through slots 0.. in one upload round and ONE call (several workgroups, the last one partly idle when
    the waves are odd in number)."""
    from wrenc_amd import gpu
    pics = _pictures(w, h)
    # (the half-step picture is what it says: block (1, 1) has four coefficients whose errors at QP 63 are the largest)
    c = rr.block_coefficients(pics[-1][0], 1, 1).ravel()
    e = dr.errors(c[:4])[:, 63]
    assert c[:4].tolist() == [-3648] * 4 and not c[4:].any() and np.abs(e).tolist() == [29184] * 4 and 1 << 31 < int((e * e).sum()) < 1 << 32
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=len(pics))
    for k, p in enumerate(pics):
        enc.upload(k, *p)
    got = enc.download_dist_curve(0, len(pics))
    one = enc.download_dist_curve(2, 1)              # (an odd number of waves at 32 x 32: the second wave of the workgroup idles)
    enc.close()
    assert got.shape == (len(pics), 3, 64) and got.dtype == np.uint64
    for k, p in enumerate(pics):
        _check(got[k], dr.dist_curve(*p), k)
    _check(one[0], got[2], "alone")
    flat, checker = got[len(KINDS)], got[len(KINDS) + 1]
    # a flat picture: only its first block (predicted as 128) has a coefficient, the DC 64 x (93 - 128)
    e = dr.errors([64 * 35])[0]
    assert flat.tolist() == [(e * e).tolist()] * 3
    # 0 / 255 squares: every block but the first has the one coefficient 64 x 255, m = 130,560, the bound: a lane's four
    # luma blocks are four such terms at every QP
    big, first = dr.errors([16320])[0], dr.errors([8192])[0]
    assert checker[0].tolist() == ((w * h // 64 - 1) * big * big + first * first).tolist()


@pytest.mark.parametrize("visible,coded", [((34, 30), (64, 32)), ((70, 50), (96, 64))])
def test_padded_pictures_count_their_margin(built, visible, coded):
    from wrenc_amd import gpu
    pics = [content("cclm", *visible, 5), rr.noise(*visible, 9)]
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, n_slots=2, visible=visible)
    for k, p in enumerate(pics):
        enc.upload(k, *p)
    got = enc.download_dist_curve(0, 2)
    enc.close()
    for k, p in enumerate(pics):
        _check(got[k], dr.dist_curve(*rr.padded(p, *coded)), k)


def test_back_to_back_uploads_and_a_replaced_slot(built):
    """Two slots uploaded without a sync between them, then another picture into slot 0: slot 1's table is unchanged; the
    figures do not depend on the slot or on the call's size; the error codes."""
    from wrenc_amd import gpu
    w, h, n = 96, 64, 4
    pics = [content("cclm", w, h, 1), rr.noise(w, h, 2), content("stripes30", w, h, 3)]
    refs = [dr.dist_curve(*p) for p in pics]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=n)
    with pytest.raises(gpu.WrencGpuError) as e:            # nothing uploaded yet
        enc.download_dist_curve(0, 1)
    assert e.value.code == ESTATE
    for first, count in ((-1, 1), (0, 0), (n, 1), (n - 1, 2), (0, n + 1)):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.download_dist_curve(first, count)
        assert e.value.code == EINVAL, (first, count)
    enc.upload(0, *pics[0])
    enc.upload(1, *pics[1])
    both = enc.download_dist_curve(0, 2)
    _check(both[0], refs[0], "slot 0")
    _check(both[1], refs[1], "slot 1")
    with pytest.raises(gpu.WrencGpuError) as e:            # slot 2 of the range is fresh
        enc.download_dist_curve(0, 3)
    assert e.value.code == ESTATE
    enc.upload(0, *pics[2])
    after = enc.download_dist_curve(0, 2)
    _check(after[0], refs[2], "slot 0 replaced")
    _check(after[1], refs[1], "slot 1 after slot 0's upload")
    enc.upload(n - 1, *pics[1])
    _check(enc.download_dist_curve(n - 1, 1)[0], refs[1], "last slot, alone")
    enc.close()


def test_a_converted_scaled_padded_picture(built):
    """yuv422p10le 70x50 -> 34x30 in 64x32: the table is that of the converted, scaled, padded picture."""
    from wrenc_amd import gpu
    fmt, source, visible, coded = format_ref.YUV422P10LE, (70, 50), (34, 30), (64, 32)
    raw = format_ref.picture("textured", fmt, *source)
    want = pad_planes(scale_ref.scale_planes(format_ref.convert(fmt, raw), *visible), *coded)
    enc = gpu.Encoder(coded[0], coded[1], qp=32, max_split_depth=2, source_format=fmt)
    enc.set_visible_size(*visible)
    enc.set_source_size(*source)
    enc.upload_planes(0, raw)
    got = enc.download_dist_curve(0, 1)[0]
    enc.close()
    _check(got, dr.dist_curve(*want), "converted")


def test_the_search_and_the_rate_histogram_do_not_notice_the_call(built):
    """The same record with the call before the search, while it is queued, and after it -- and without any call; the rate
    histogram behind the call is the one without it."""
    from wrenc_amd import gpu
    w, h = 96, 64
    pic = content("cclm", w, h, 4)
    ref = dr.dist_curve(*pic)
    plain = gpu.Encoder(w, h, qp=32, max_split_depth=2)
    want = plain.encode_picture(*pic)
    plain.close()
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=2)
    enc.upload(0, *pic)
    _check(enc.download_dist_curve(0, 1)[0], ref, "before the search")
    enc.encode(0, 1)
    enc.upload(1, *pic)
    _check(enc.download_dist_curve(0, 2)[1], ref, "behind a queued search")
    got = enc.download(0)
    _check(enc.download_dist_curve(0, 1)[0], ref, "after the search")
    hist = enc.download_rate_hist(0, 2)
    assert enc.final_pass_mismatches() == 0
    enc.close()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(hist[0], rr.rate_hist(*pic)) and np.array_equal(hist[1], hist[0])
