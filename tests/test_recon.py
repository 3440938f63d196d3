"""CPU tests of include/wrenc_recon.h through libwrenc_gpu.so's host-only entries (wrenc_gpu_recon_from_name, _recon_name,
_recon_layout, _recon_coefficients, _recon_convert_host): the library's converter against the numpy restatement
(recon_ref.py), the coefficient table against its rule in exact rationals, the three properties the header states, and the
command line's argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import recon_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
EINVAL = -1
SIZES = ((16, 16), (1030, 18), (1022, 18))
RGB_CASES = [(f, m, r) for f in range(5) for m in (rr.BT709, rr.BT601) for r in (rr.TV, rr.PC)]
CASES = RGB_CASES + [(rr.YUV420P, 0, 0), (rr.NV12, 0, 0)]


def _sentinel_planes(fmt, w, h, extra=7, value=0xA5):
    """Destination planes as views into wider arrays filled with a sentinel: (views, the wide arrays)."""
    wide = [np.full((rows, row_bytes + extra), value, np.uint8) for rows, row_bytes in rr.layout(fmt, w, h)]
    return [a[:, :a.shape[1] - extra] for a in wide], wide


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_host_converter_equals_the_reference(built, size):
    from wrenc_amd import gpu
    w, h = size
    for content in (rr.noise(w, h, 5), rr.corners(w, h)):
        for fmt, matrix, rng in CASES:
            want = rr.convert(fmt, matrix, rng, *content)
            views, wide = _sentinel_planes(fmt, w, h)
            got = gpu.recon_convert_host(fmt, matrix, rng, w, h, *content, out=views)
            assert len(got) == len(want)
            for p, (a, b, big) in enumerate(zip(got, want, wide)):
                assert a.shape == b.shape and np.array_equal(a, b), (fmt, matrix, rng, p, np.argwhere(a != b)[:4].tolist())
                assert np.all(big[:, b.shape[1]:] == 0xA5), (fmt, p)       # the bytes between the rows are untouched
            fresh = gpu.recon_convert_host(rr.NAMES[fmt], ("bt709", "bt601")[matrix], ("tv", "pc")[rng], w, h, *content)
            assert all(np.array_equal(a, b) for a, b in zip(fresh, want))


def test_the_corners_picture_clips_at_both_ends():
    y, cb, cr = rr.corners(64, 32)
    k = rr.coefficients(rr.BT709, rr.TV)
    for a in rr.rgb_unclipped(k, y, rr.chroma16(cb), rr.chroma16(cr)):
        assert a.min() < 0 and a.max() > 255


def test_coefficient_table_equals_the_rule(built):
    from wrenc_amd import gpu
    rows = {}
    for m, mname in ((rr.BT709, "bt709"), (rr.BT601, "bt601")):
        for r, rname in ((rr.TV, "tv"), (rr.PC, "pc")):
            want = rr.coefficients(m, r)
            assert gpu.recon_coefficients(m, r) == want == gpu.recon_coefficients(mname, rname)
            rows[(mname, rname)] = want
    assert rows[("bt709", "tv")] == [19077, 29372, -3494, -8731, 34610, 16]
    assert rows[("bt709", "tv")][4] > 32767                                # bu does not fit a signed 16-bit operand
    header = open(os.path.join(ROOT, "include", "wrenc_recon.h")).read()
    for (mname, rname), k in rows.items():                                 # the comment's rows are the table's
        assert " ".join([mname, rname] + [str(v) for v in k]) in " ".join(header.split()), (mname, rname)
    for bad in ((2, 0), (0, 2), (-1, 0)):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.recon_coefficients(*bad)
        assert e.value.code == EINVAL


@pytest.mark.parametrize("matrix,rng", [(rr.BT709, rr.TV), (rr.BT601, rr.PC)], ids=["bt709-tv", "bt601-pc"])
def test_every_sample_triple_is_near_the_real_formula_and_inside_32_bits(matrix, rng):
    """All 2^24 (Y, Cb, Cr) with flat chroma (C16 = 16 C): the unclipped integer result within 0.5 + 511 / 2^15 of the
    real-valued formula, every accumulator inside int32."""
    k = rr.coefficients(matrix, rng)
    inv_sy, rv, gu, gv, bu, yoff = rr.real_coefficients(matrix, rng)
    bound = 0.5 + 511.0 / (1 << 15)
    cb, cr = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    u, v = (cb - 128).astype(np.float64), (cr - 128).astype(np.float64)
    real_c = (rv * v, gu * u + gv * v, bu * u)
    worst, lo, hi = 0.0, 0, 0
    for y in range(256):
        acc = rr.accumulators(k, y, 16 * cb, 16 * cr)
        lo, hi = min(lo, min(int(a.min()) for a in acc)), max(hi, max(int(a.max()) for a in acc))
        yr = (y - yoff) * inv_sy
        for a, c in zip(acc, real_c):
            worst = max(worst, float(np.abs((a >> 18) - (yr + c)).max()))
    assert -(1 << 31) <= lo and hi < (1 << 31), (lo, hi)
    assert worst <= bound + 1e-9, (worst, bound)                           # (1e-9: the float64 evaluation of the real formula)
    assert worst > 0.5                                                     # the bound is not idle: some triple rounds from beyond a half


def test_bilinear_chroma_is_within_the_bound_too():
    """The same bound on real-valued bilinear chroma (weights 9, 3, 3, 1 over 16) of a noise picture."""
    y, cb, cr = rr.noise(64, 32, 11)
    for matrix, rng in ((rr.BT709, rr.TV), (rr.BT601, rr.PC)):
        k = rr.coefficients(matrix, rng)
        inv_sy, rv, gu, gv, bu, yoff = rr.real_coefficients(matrix, rng)
        cb16, cr16 = rr.chroma16(cb), rr.chroma16(cr)
        u, v = cb16 / 16.0 - 128, cr16 / 16.0 - 128
        yr = (y.astype(np.float64) - yoff) * inv_sy
        for a, real in zip(rr.rgb_unclipped(k, y, cb16, cr16), (yr + rv * v, yr + gu * u + gv * v, yr + bu * u)):
            assert float(np.abs(a - real).max()) <= 0.5 + 511.0 / (1 << 15) + 1e-9


def test_grey_gives_equal_components(built):
    from wrenc_amd import gpu
    y = rr.noise(32, 16, 3)[0]
    grey = np.full((8, 16), 128, np.uint8)
    for matrix in (rr.BT709, rr.BT601):
        for rng in (rr.TV, rr.PC):
            g, b, r = gpu.recon_convert_host("gbrp", matrix, rng, 32, 16, y, grey, grey)
            assert np.array_equal(g, b) and np.array_equal(g, r)
            assert np.array_equal(r, rr.rgb(matrix, rng, y, grey, grey)[:, :, 0])
    assert len(np.unique(r)) > 100


def test_constant_chroma_upsamples_to_sixteen_times_the_constant():
    for c in (0, 1, 77, 128, 255):
        assert np.all(rr.chroma16(np.full((9, 17), c, np.uint8)) == 16 * c)


def test_first_and_last_rows_and_columns_use_the_clamp(built):
    from wrenc_amd import gpu
    rng = np.random.default_rng(8)
    c = rng.integers(0, 256, (8, 8), dtype=np.uint8).astype(np.int64)
    c16 = rr.chroma16(c)
    assert np.array_equal(c16[1:-1, 0], 12 * c[rr_rows(16)[1:-1], 0] + 4 * c[rr_rows2(16, 8)[1:-1], 0])        # x = 0: i' = i
    assert np.array_equal(c16[1:-1, -1], 12 * c[rr_rows(16)[1:-1], -1] + 4 * c[rr_rows2(16, 8)[1:-1], -1])     # x = w - 1
    assert np.array_equal(c16[0, 1:-1], 12 * c[0, rr_rows(16)[1:-1]] + 4 * c[0, rr_rows2(16, 8)[1:-1]])        # y = 0: j' = j
    assert np.array_equal(c16[-1, 1:-1], 12 * c[-1, rr_rows(16)[1:-1]] + 4 * c[-1, rr_rows2(16, 8)[1:-1]])     # y = h - 1
    assert c16[0, 0] == 16 * c[0, 0] and c16[-1, -1] == 16 * c[-1, -1] and c16[0, -1] == 16 * c[0, -1]
    assert c16[1, 1] == 9 * c[0, 0] + 3 * c[0, 1] + 3 * c[1, 0] + c[1, 1]                                      # the interior rule
    # ... and the library agrees at the edges of a picture whose edge chroma differs from its neighbours
    y = np.full((16, 16), 128, np.uint8)
    got = gpu.recon_convert_host("rgb24", "bt709", "pc", 16, 16, y, c.astype(np.uint8), c.astype(np.uint8)[::-1].copy())[0]
    want = rr.convert(rr.RGB24, rr.BT709, rr.PC, y, c.astype(np.uint8), c.astype(np.uint8)[::-1].copy())[0]
    for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), slice(0, 3)), (slice(None), slice(-3, None))):
        assert np.array_equal(got[sl], want[sl])


def rr_rows(n):
    """i = x >> 1 for x < n."""
    return np.arange(n) >> 1


def rr_rows2(n, cn):
    """i' of the rules for x < n on an axis of cn chroma samples."""
    x = np.arange(n)
    return np.clip((x >> 1) + np.where(x & 1, 1, -1), 0, cn - 1)


def test_names_and_aliases(built):
    from wrenc_amd import gpu
    for i, name in enumerate(rr.NAMES):
        assert gpu.recon_from_name(name) == i and gpu.recon_name(i) == name
    for i in range(5):                                                     # the RGB layouts keep wrenc_rgb.h's ids and names
        assert gpu.rgb_name(i) == gpu.recon_name(i) and gpu.rgb_from_name(rr.NAMES[i]) == i
    for alias, i in rr.ALIASES.items():
        assert gpu.recon_from_name(alias) == i
    assert gpu.recon_name(7) is None and gpu.recon_name(-1) is None
    for bad in ("yuv422p", "RGB24", "", None, "p010le"):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.recon_from_name(bad)
        assert e.value.code == EINVAL


def test_layouts(built):
    from wrenc_amd import gpu
    for fmt in range(7):
        for w, h in SIZES:
            lay = gpu.recon_layout(fmt, w, h)
            want = rr.layout(fmt, w, h)
            assert lay["n_planes"] == len(want) and lay["bytes_per_sample"] == 1
            assert list(zip(lay["rows"], lay["row_bytes"])) == want
            assert lay["offset"] == [sum(r * b for r, b in want[:p]) for p in range(len(want))]
            assert lay["frame_bytes"] == sum(r * b for r, b in want)
    assert gpu.recon_layout("rgb24", 64, 32) == gpu.rgb_layout("rgb24", 64, 32)
    assert gpu.recon_layout("nv12", 64, 32) == gpu.format_layout("nv12", 64, 32)
    for bad in ((7, 64, 32), (-1, 64, 32), (0, 63, 32), (5, 64, 31), (6, 14, 32), (0, 64, 14)):
        with pytest.raises(gpu.WrencGpuError) as e:
            gpu.recon_layout(*bad)
        assert e.value.code == EINVAL


def test_converter_refusals(built):
    import ctypes as C
    from wrenc_amd import gpu
    lib = gpu.load_library()
    w, h = 16, 16
    y, cb, cr = rr.noise(w, h, 1)
    out = [np.zeros((h, 4 * w), np.uint8) for _ in range(3)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(fmt, matrix, rng, w_, h_, planes=(y, cb, cr), dst=out, strides=(4 * w, 4 * w, 4 * w), null_list=False):
        ptr = (C.c_void_p * 3)(*[a.ctypes.data if a is not None else None for a in dst])
        st = (C.c_size_t * 3)(*strides)
        return lib.wrenc_gpu_recon_convert_host(fmt, matrix, rng, w_, h_, *[p(a) if a is not None else None for a in planes],
                                                None if null_list else ptr, st)

    assert call(rr.RGB24, 0, 0, w, h) == 0
    assert call(rr.YUV420P, 9, 9, w, h) == 0                               # matrix and range are not read for the YUV outputs
    assert call(7, 0, 0, w, h) == EINVAL and call(-1, 0, 0, w, h) == EINVAL
    assert call(rr.RGB24, 2, 0, w, h) == EINVAL and call(rr.RGB24, 0, 2, w, h) == EINVAL
    assert call(rr.RGB24, 0, 0, 15, h) == EINVAL and call(rr.RGB24, 0, 0, w, 14) == EINVAL
    assert call(rr.RGB24, 0, 0, w, h, planes=(y, None, cr)) == EINVAL
    assert call(rr.RGB24, 0, 0, w, h, dst=[None, out[1], out[2]]) == EINVAL
    assert call(rr.RGB24, 0, 0, w, h, dst=[out[0], None, None]) == 0       # a packed layout writes plane 0 alone
    assert call(rr.GBRP, 0, 0, w, h, dst=[out[0], out[1], None]) == EINVAL
    assert call(rr.NV12, 0, 0, w, h, dst=[out[0], out[1], None]) == 0      # nv12 has two planes
    assert call(rr.NV12, 0, 0, w, h, dst=[out[0], None, out[2]]) == EINVAL
    assert call(rr.RGB24, 0, 0, w, h, strides=(3 * w - 1, 0, 0)) == EINVAL
    assert call(rr.RGB24, 0, 0, w, h, strides=(3 * w, 0, 0)) == 0
    assert call(rr.YUV420P, 0, 0, w, h, strides=(w, w // 2, w // 2 - 1)) == EINVAL
    assert call(rr.RGB24, 0, 0, w, h, null_list=True) == EINVAL
    with pytest.raises(gpu.WrencGpuError):
        gpu.recon_convert_host("rgb24", "bt709", "tv", w, h, y, cb, cr, out=[np.zeros((h, 3 * w + 1), np.uint8)])
    with pytest.raises(gpu.WrencGpuError):
        gpu.recon_convert_host("rgb24", "bt2020", "tv", w, h, y, cb, cr)


def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + args, cwd=ROOT, capture_output=True, timeout=600)


@pytest.mark.parametrize("front", ["native", "python"])
def test_command_line_argument_errors(built, tmp_path, front):
    """Message on stderr, exit status 0, as tests/test_cli.py has it for the other options."""
    out, rec = str(tmp_path / "o.vvc"), str(tmp_path / "r.raw")
    base = ["-i", str(tmp_path / "missing.yuv"), "-o", out, "--num-pictures", "1", "--qp", "32", "--input-size", "64x64", "--output-size", "64x64"]
    r = _run(front, base + ["--reconst-format", "rgb24"])
    assert r.returncode == 0 and b"error: --reconst-format needs --reconst" in r.stderr
    r = _run(front, base + ["-r", rec, "--reconst-format", "yuv422p"])
    assert r.returncode == 0 and b"error: Invalid reconst-format: yuv422p" in r.stderr
    for opt, value in (("--reconst-colorspace", "bt601"), ("--reconst-range", "pc")):
        for fmt in (["--reconst-format", "yuv420p"], ["--reconst-format", "nv12"], []):
            r = _run(front, base + ["-r", rec] + fmt + [opt, value])
            assert r.returncode == 0 and b"error: " + opt.encode() + b" needs an RGB --reconst-format" in r.stderr, (opt, fmt, r.stderr)
    r = _run(front, base + ["-r", rec, "--reconst-format", "rgb24", "--reconst-colorspace", "bt2020"])
    assert r.returncode == 0 and b"error: Invalid reconst-colorspace: bt2020" in r.stderr
    r = _run(front, base + ["-r", rec, "--reconst-format", "rgb24", "--reconst-range", "full"])
    assert r.returncode == 0 and b"error: Invalid reconst-range: full" in r.stderr
    # well-formed options get as far as the input file
    r = _run(front, base + ["-r", rec, "--reconst-format", "bgra", "--reconst-colorspace", "bt601", "--reconst-range", "pc"])
    assert r.returncode == 0 and b"error: failed to open input file" in r.stderr
