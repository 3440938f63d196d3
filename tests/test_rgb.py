"""RGB sources on the host (include/wrenc_rgb.h, exported as wrenc_gpu_rgb_from_name, _rgb_name, _rgb_layout,
_rgb_coefficients and _rgb_convert_host) against their restatement in Python (tests/rgb_ref.py) and against the real-valued
formula, and the --colorspace / --range argument errors of both command lines, which need no device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rgb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
EINVAL = -1
SIZES = [(16, 16), (34, 30), (70, 50)]
COMBO_IDS = ["%s-%s" % (rgb_ref.MATRICES[m], rgb_ref.RANGES[r]) for m, r in rgb_ref.COMBOS]


# ---- tables ----

@pytest.mark.parametrize("matrix,rng", rgb_ref.COMBOS, ids=COMBO_IDS)
def test_coefficients_are_the_table_and_its_derivation(built, matrix, rng):
    from wrenc_amd import gpu
    k = gpu.rgb_coefficients(matrix, rng)
    assert k == rgb_ref.TABLE[(matrix, rng)] == rgb_ref.derive(matrix, rng)
    assert k == gpu.rgb_coefficients(rgb_ref.MATRICES[matrix], rgb_ref.RANGES[rng])
    sy, _ = rgb_ref.scales(rng)
    assert sum(k[0:3]) == int(np.floor(sy * 2 ** 14 + 0.5))         # grey is exact
    assert sum(k[3:6]) == 0 and sum(k[6:9]) == 0                     # grey is exactly 128
    assert k[9] == (16 if rng == rgb_ref.TV else 0)


def test_coefficient_refusals(built):
    from wrenc_amd import gpu
    for m, r in ((-1, 0), (2, 0), (0, -1), (0, 2), ("bt2020", "tv"), ("bt709", "full")):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.rgb_coefficients(m, r)
        assert e.value.code == EINVAL, (m, r)
    assert gpu.load_library().wrenc_gpu_rgb_coefficients(0, 0, None) == EINVAL


@pytest.mark.parametrize("matrix,rng", rgb_ref.COMBOS, ids=COMBO_IDS)
def test_anchors(built, matrix, rng):
    """Flat 16x16 pictures of the five anchor colours, in all five layouts, through the host converter."""
    from wrenc_amd import gpu
    for name, want in rgb_ref.ANCHORS[(matrix, rng)].items():
        for lay in rgb_ref.LAYOUTS:
            y, cb, cr = gpu.rgb_convert_host(lay, matrix, rng, 16, 16, rgb_ref.picture(name, lay, 16, 16))
            got = (set(y.ravel().tolist()), set(cb.ravel().tolist()), set(cr.ravel().tolist()))
            assert got == ({want[0]}, {want[1]}, {want[2]}), (name, rgb_ref.NAMES[lay], got, want)


# ---- the host converter against the numpy restatement ----

@pytest.mark.parametrize("lay", rgb_ref.LAYOUTS, ids=rgb_ref.NAMES)
def test_host_converter_equals_the_reference(built, lay):
    from wrenc_amd import gpu
    for w, h in SIZES:
        for name in rgb_ref.PICTURES:
            raw = rgb_ref.picture(name, lay, w, h)
            wide = rgb_ref.strided(raw, (24, 8, 40))
            for matrix, rng in rgb_ref.COMBOS:
                want = rgb_ref.convert(lay, matrix, rng, raw)
                for planes in (raw, wide):
                    got = gpu.rgb_convert_host(lay, matrix, rng, w, h, planes if len(planes) > 1 else planes[0])
                    for p in range(3):
                        assert got[p].shape == want[p].shape and np.array_equal(got[p], want[p]), (w, h, name, matrix, rng, p)


def test_the_reference_pictures_cover_what_they_claim():
    pic = rgb_ref.rgb_picture("corners", 16, 16).astype(np.int64)
    assert set(np.unique(pic).tolist()) == {0, 255}
    sums = pic[0::2, 0::2] + pic[0::2, 1::2] + pic[1::2, 0::2] + pic[1::2, 1::2]
    assert len({tuple(s) for s in sums.reshape(-1, 3).tolist()}) == 64             # the 4^3 combinations of the sums
    # pc, bt709: an all-blue block reaches 256 before the clip, an all-red one too (Cr)
    k = rgb_ref.TABLE[(rgb_ref.BT709, rgb_ref.PC)]
    assert (k[5] * 1020 + (128 << 16) + (1 << 15)) >> 16 == 256 and (k[6] * 1020 + (128 << 16) + (1 << 15)) >> 16 == 256
    y, cb, cr = rgb_ref.convert(rgb_ref.RGB24, rgb_ref.BT709, rgb_ref.PC, rgb_ref.pack(rgb_ref.RGB24, pic))
    assert int(cb.max()) == 255 and int(cr.max()) == 255
    # junk in the X byte, and convert() does not see it
    a = rgb_ref.pack(rgb_ref.RGB0, pic, np.random.default_rng(1))
    b = rgb_ref.pack(rgb_ref.BGR0, pic, np.random.default_rng(2))
    assert len(np.unique(a[0][:, 3::4])) > 16
    assert all(np.array_equal(p, q) for p, q in zip(rgb_ref.convert(rgb_ref.RGB0, 0, 0, a), rgb_ref.convert(rgb_ref.BGR0, 0, 0, b)))


# ---- against the real-valued formula ----

LUMA_BOUND = 0.5 + 255 * (0.5 + 0.5 + 1.5) / 2 ** 14      # the final rounding; yr and yb off by 0.5 at most, yg by 1.5 (its own rounding and theirs)
CHROMA_BOUND = 0.5 + 1020 * 2 / 2 ** 16                   # ... the outer coefficients off by 0.5 each, the middle one by their sum


def _real_luma(matrix, rng, r, g, b):
    kr, kb = rgb_ref.K[matrix]
    sy, _ = rgb_ref.scales(rng)
    return (16 if rng == rgb_ref.TV else 0) + sy * (kr * r + (1 - kr - kb) * g + kb * b)


def _real_chroma(matrix, rng, r, g, b):
    """(Cb, Cr) of mean colours r, g, b."""
    kr, kb = rgb_ref.K[matrix]
    _, sc = rgb_ref.scales(rng)
    yy = kr * r + (1 - kr - kb) * g + kb * b
    return 128 + sc * (b - yy) / (2 * (1 - kb)), 128 + sc * (r - yy) / (2 * (1 - kr))


def test_luma_of_every_colour_is_within_the_derived_bound(built):
    """bt709 tv, all 2^24 colours, through the host converter, 2^20 at a time: a 4096 x 256 rgb24 picture per value of
    the four high bits of R."""
    from wrenc_amd import gpu
    assert LUMA_BOUND < 0.54
    lo = np.arange(1 << 20, dtype=np.int64)
    g, b = (lo >> 8) & 255, lo & 255
    worst = 0.0
    for hi in range(16):
        r = (hi << 4) | (lo >> 16)
        pic = np.stack([r, g, b], axis=1).astype(np.uint8).reshape(256, 4096 * 3)
        y, _, _ = gpu.rgb_convert_host("rgb24", "bt709", "tv", 4096, 256, pic)
        err = np.abs(y.reshape(-1).astype(np.float64) - _real_luma(rgb_ref.BT709, rgb_ref.TV, r, g, b))
        worst = max(worst, float(err.max()))
    assert worst <= LUMA_BOUND, worst


@pytest.mark.parametrize("matrix,rng", rgb_ref.COMBOS, ids=COMBO_IDS)
def test_random_colours_are_within_the_derived_bounds(built, matrix, rng):
    """2^20 random colours as a 1024 x 1024 picture: luma per pixel, chroma per 2x2 block, except where the clip acts."""
    from wrenc_amd import gpu
    rgb = rgb_ref.rgb_picture("noise", 1024, 1024, seed=5 + 2 * matrix + rng)
    rgb[:64] = rgb_ref.rgb_picture("corners", 1024, 64)                       # with the extremes of every accumulator
    y, cb, cr = gpu.rgb_convert_host("rgb24", matrix, rng, 1024, 1024, rgb_ref.pack(rgb_ref.RGB24, rgb)[0])
    c = rgb.astype(np.float64)
    err = np.abs(y - _real_luma(matrix, rng, c[:, :, 0], c[:, :, 1], c[:, :, 2]))
    assert float(err.max()) <= LUMA_BOUND, float(err.max())
    mean = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]) / 4
    clipped = 0
    for got, real in zip((cb, cr), _real_chroma(matrix, rng, mean[:, :, 0], mean[:, :, 1], mean[:, :, 2])):
        inside = real <= 255.0
        assert float(np.abs(got - real)[inside].max()) <= CHROMA_BOUND
        assert np.all(got[~inside] == 255)                                     # the clip: 255.5 .. 256 would round to 256
        clipped += int((~inside).sum())
    assert (clipped > 0) == (rng == rgb_ref.PC)                                # live only for pc chroma


# ---- layouts and names ----

@pytest.mark.parametrize("w,h", SIZES + [(3840, 2160)], ids=lambda v: str(v))
def test_layout_equals_the_python_layout(built, w, h):
    from wrenc_amd import gpu
    for lay in rgb_ref.LAYOUTS:
        got = gpu.rgb_layout(lay, w, h)
        assert got == rgb_ref.layout(lay, w, h) == gpu.rgb_layout(rgb_ref.NAMES[lay], w, h), lay
        raw = rgb_ref.picture("black", lay, w, h)
        assert [p.shape[0] for p in raw] == got["rows"] and [p.shape[1] for p in raw] == got["row_bytes"], lay
        assert len(rgb_ref.raw_bytes(raw)) == got["frame_bytes"] == w * h * (4 if lay in (rgb_ref.RGB0, rgb_ref.BGR0) else 3)
    assert gpu.rgb_layout("gbrp", w, h)["offset"] == [0, w * h, 2 * w * h]
    assert gpu.rgb_layout("bgr0", w, h)["offset"] == [0]


def test_names_and_aliases(built):
    from wrenc_amd import gpu
    for lay, name in enumerate(rgb_ref.NAMES):
        assert gpu.rgb_from_name(name) == lay and gpu.rgb_name(lay) == name
    for alias, lay in rgb_ref.ALIASES.items():
        assert gpu.rgb_from_name(alias) == lay
    for lay in (-1, 5, 100):
        assert gpu.rgb_name(lay) is None
    for name in ("", "bogus", "RGB24", "rgb24 ", "rgb", "yuv420p", "nv12", "gbrap", None):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.rgb_from_name(name)
        assert e.value.code == EINVAL, name


def test_refusals(built):
    from wrenc_amd import gpu
    gpu.rgb_layout(4, 16, 16)                          # the smallest frame is served
    for lay, w, h in ((-1, 64, 64), (5, 64, 64), (0, 65, 64), (2, 64, 63), (1, 14, 64), (4, 64, 14), (3, 0, 0), (0, -64, 64)):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.rgb_layout(lay, w, h)
        assert e.value.code == EINVAL, (lay, w, h)
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.rgb_convert_host(lay, 0, 0, w, h, np.zeros((16, 64), np.uint8))
        assert e.value.code == EINVAL, (lay, w, h)
    lib = gpu.load_library()
    assert lib.wrenc_gpu_rgb_layout(0, 64, 64, None) == EINVAL       # a null pointer
    # the two id spaces stay apart: the format functions still refuse id 6 and the RGB names
    assert gpu.format_name(6) is None
    for name in ("rgb24", "gbrp", "rgba"):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.format_from_name(name)
        assert e.value.code == EINVAL
    with pytest.raises(gpu.WrencGpuError):
        gpu.format_layout(6, 64, 64)
    # the converter: a short stride, a null plane, a bad matrix or range
    import ctypes as C
    pic = np.zeros((16, 48), np.uint8)
    out = [np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)]
    o = [gpu._p(a) for a in out]

    def call(lay, m, r, ptrs, strides):
        return lib.wrenc_gpu_rgb_convert_host(lay, m, r, 16, 16, (C.c_void_p * 3)(*ptrs), (C.c_size_t * 3)(*strides), *o)

    d = pic.ctypes.data
    assert call(0, 0, 0, [d, None, None], [48, 0, 0]) == 0          # a packed layout reads plane[0] alone
    assert call(0, 0, 0, [d, None, None], [47, 0, 0]) == EINVAL
    assert call(0, 0, 0, [None, d, d], [48, 48, 48]) == EINVAL
    assert call(4, 0, 0, [d, d, None], [16, 16, 16]) == EINVAL      # gbrp reads three
    assert call(4, 0, 0, [d, d, d], [16, 15, 16]) == EINVAL
    assert call(0, 2, 0, [d, None, None], [48, 0, 0]) == EINVAL and call(0, 0, 2, [d, None, None], [48, 0, 0]) == EINVAL


# ---- command line, no device: the options are parsed before anything is opened ----

def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + args, cwd=ROOT, capture_output=True, timeout=120)


@pytest.mark.parametrize("front", ["native", "python"])
def test_colour_option_argument_errors(built, front, tmp_path):
    base = ["-i", str(tmp_path / "missing.rgb"), "-o", str(tmp_path / "out.vvc"), "--num-pictures", "1", "--qp", "32",
            "--input-size", "64x64", "--output-size", "64x64"]
    for args, text in ((["--colorspace", "bt709", "--input-format", "nv12"], b"error: --colorspace needs an RGB --input-format"),
                       (["--colorspace", "bt709"], b"error: --colorspace needs an RGB --input-format"),          # yuv420p, the default
                       (["--input-format", "yuv420p", "--range", "pc"], b"error: --range needs an RGB --input-format"),
                       (["--input-format", "rgb24", "--range", "full"], b"error: Invalid range: full"),
                       (["--input-format", "rgb24", "--colorspace", "bt2020"], b"error: Invalid colorspace: bt2020"),
                       (["--input-format", "rgb24", "--colorspace"], b"error: option --colorspace needs a value"),
                       (["--input-format", "rgb24", "--range"], b"error: option --range needs a value")):
        r = _run(front, base + args)
        assert r.returncode == 0 and text in r.stderr, (args, r.stderr)
    # known names and values get as far as the input file
    for args in (["--input-format", "rgb24"], ["--input-format", "bgra", "--colorspace", "bt601", "--range", "pc"],
                 ["--range", "tv", "--input-format", "gbrp"]):
        r = _run(front, base + args)
        assert r.returncode == 0 and b"error: failed to open input file" in r.stderr, (args, r.stderr)
    assert not (tmp_path / "out.vvc").exists()
