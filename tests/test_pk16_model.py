"""The packed 16-bit row helpers (wrenc_amd/csrc/dev_pk16.h) against the scalar formulas they replace, on NumPy models
with explicit i16 wrap-around (tests/pk16_model.py): the range conditions the device code states at each helper."""
import numpy as np

import pk16_model as m

def test_bytes_to_pairs_and_back():
    """pk16_lo / pk16_hi put byte k of a dword into pair lane k & 1, zero-extended; pk16_pack takes the low bytes back:
    exact for every value 0..255 in every position."""
    rng = np.random.default_rng(1602)
    w = np.concatenate([np.array([0, 0xFFFFFFFF, 0x00FF00FF, 0xFF00FF00, 0x01020304, 0x80FF7F00], np.uint32),
                        rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)])
    b = [(w.astype(np.int64) >> (8 * k)) & 255 for k in range(4)]
    lo0, lo1 = m.halves(m.pk_lo(w))
    hi0, hi1 = m.halves(m.pk_hi(w))
    for got, want in zip((lo0, lo1, hi0, hi1), b):
        assert np.array_equal(got, want)
    assert np.array_equal(m.pk_pack(m.pk_lo(w), m.pk_hi(w)), w)
    # all 256 x 256 byte pairs of one pair register, in both halves of the dword
    a, c = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    pair = (a | (c << np.uint32(16))).ravel()
    packed = m.pk_pack(pair, pair[::-1].copy())
    assert np.array_equal(packed & 0xFF, a.ravel()) and np.array_equal((packed >> 8) & 0xFF, c.ravel())
    assert np.array_equal((packed >> 16) & 0xFF, a.ravel()[::-1]) and np.array_equal(packed >> 24, c.ravel()[::-1])


W7 = np.array([0, 1, 2, 4, 8, 16, 32], np.int64)


def test_pdpc_weights_of_position_pairs():
    """pk16_positions and pk16_pdpc_w2 against pdpc_w: every even x of a 32-sample line (and the pair's second position),
    every n_scale; the capped shift count gives 0 where the rule says 0."""
    x = np.arange(0, 32, 2)
    p0, p1 = m.positions(x)
    assert np.array_equal(p0, x) and np.array_equal(p1, x + 1)
    allpos = np.arange(0, 34)
    for n_scale in (0, 1, 2):
        assert np.array_equal(m.pdpc_w_pk(n_scale, allpos), m.pdpc_w(n_scale, allpos))
        assert set(m.pdpc_w(n_scale, allpos).tolist()) <= set(W7.tolist())
        # beyond 3 << n_scale the weight is 0 by the formula itself: the `pdpc` flag of the callers guards reads only
        assert not m.pdpc_w(n_scale, allpos[allpos >= (3 << n_scale)]).any()


def test_pdpc_blend_exhaustive():
    """766 x 7 x 256: rs in -255..510, every weight, every v -- the sum stays inside i16 and the packed blend is the scalar one."""
    rs, w, v = np.meshgrid(np.arange(-255, 511), W7, np.arange(256), indexing="ij")
    total = rs * w + (64 - w) * v + 32
    assert total.min() == -255 * 32 + 32 and total.max() == 510 * 32 + 32 * 255 + 32 < 1 << 15
    assert np.array_equal(m.pdpc_blend_pk(rs, w, v), m.pdpc_blend_scalar(rs, w, v))


def test_pdpc_rs_and_folded_blend_exhaustive():
    """side, corner, v over all bytes, every weight, the three kinds: rs of mode 18 / 50 lies in -255..510 and needs no wrap;
    the blend with the entry's constants folded (rows_per_lane) is the scalar blend of the scalar rs."""
    sv, v = (a.ravel()[None, :] for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    for kind in (1, 2):     # (kind 3 is kind 2 with another side array)
        for w in W7:
            for c0 in range(0, 256, 32):
                corner = np.arange(c0, c0 + 32)[:, None] if kind == 1 else np.array([[c0]])
                rs = m.pdpc_rs_scalar(kind, sv, corner, v)
                assert np.array_equal(rs, m.pdpc_rs_pk(kind, sv, corner, v))
                assert rs.min() >= -255 and rs.max() <= 510
                want = m.pdpc_blend_scalar(rs, w, v)
                assert np.array_equal(m.pdpc_folded_pk(kind, sv, corner, w, v), want)
                assert np.array_equal(m.pdpc_blend_pk(rs, w, v), want)


def _filter_rows():
    import json
    import os
    tabs = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_source_data.json")))["tables"]
    fc = np.array(tabs["f_c"], np.int64).reshape(32, 4)
    fg = np.array([(16 - (p >> 1), 32 - (p >> 1), 16 + (p >> 1), p >> 1) for p in range(32)], np.int64)
    chroma = np.array([(0, 32 - p, p, 0) for p in range(32)], np.int64)
    return fc, fg, chroma


def test_range_after_the_dot_product():
    """All 32 rows of both luma filters and of the chroma filter, tap bytes at {0, 1, 127, 128, 254, 255}^4: the shifted
    sum lies inside i16 (luma: -40..295 at the most), and what goes into a pair -- luma after its 32-bit clamp, chroma
    as it is, a convex combination -- lies in 0..255."""
    fc, fg, chroma = _filter_rows()
    assert (fc.sum(axis=1) == 64).all() and (fg.sum(axis=1) == 64).all() and (chroma.sum(axis=1) == 32).all()
    e = np.array([0, 1, 127, 128, 254, 255], np.int64)
    taps = np.stack([a.ravel() for a in np.meshgrid(e, e, e, e, indexing="ij")], axis=-1)        # (1296, 4)
    for tab, luma in ((fc, True), (fg, True), (chroma, False)):
        v = m.ang_sample_scalar(tab[:, None, :], taps[None, :, :], luma)
        assert -32768 <= v.min() and v.max() <= 32767
        if luma:
            assert np.array_equal(v, (tab[:, None, :] * taps[None, :, :]).sum(axis=-1) + 32 >> 6)   # the XOR 0x80 form is the plain one
        else:
            assert v.min() >= 0 and v.max() <= 255
    v = m.ang_sample_scalar(fg[:, None, :], taps[None, :, :], True)
    assert v.min() >= 0 and v.max() <= 255          # the smoothing filter has no negative tap


def _planar_points():
    """every (x, y) of every block size x all corners of the four references, and 10^6 seeded points"""
    rng = np.random.default_rng(1604)
    out = []
    for lg in (2, 3, 4, 5):
        n = 1 << lg
        e = np.array([0, 255], np.int64)
        y, x, a, lb, l, an = (g.ravel() for g in np.meshgrid(np.arange(n), np.arange(n), e, e, e, e, indexing="ij"))
        r = 250000
        ry, rx = rng.integers(0, n, r), rng.integers(0, n, r)
        ra, rlb, rl, ran = (rng.integers(0, 256, r) for _ in range(4))
        out.append((lg, np.concatenate([x, rx]), np.concatenate([y, ry]), np.concatenate([a, ra]), np.concatenate([lb, rlb]),
                    np.concatenate([l, rl]), np.concatenate([an, ran])))
    return out


def test_planar_pairs():
    for lg, x, y, a, lb, l, an in _planar_points():
        n = 1 << lg
        total = (n - 1 - y) * a + (y + 1) * lb + (n - 1 - x) * l + (x + 1) * an + n
        assert total.min() >= 0 and total.max() <= 2 * 32 * 255 + 32
        got, want = m.planar_pk(lg, x, y, a, lb, l, an), m.planar_scalar(lg, x, y, a, lb, l, an)
        assert np.array_equal(got, want) and want.max() <= 255
        assert np.array_equal(want, total >> (lg + 1))       # `as u8` changes nothing


def test_planar_and_dc_blend_pairs_need_no_clamp():
    """The blend of PLANAR and DC with p = the planar value, and with p = any DC value: the packed form WITHOUT a clamp
    is the scalar form with its clamp, at every corner, every (x, y) of every size and the seeded points."""
    rng = np.random.default_rng(1605)
    for lg, x, y, a, lb, l, an in _planar_points():
        ns = (2 * lg - 2) >> 2
        assert (m.pdpc_w(ns, x) + m.pdpc_w(ns, y)).max() <= 64
        p = m.planar_scalar(lg, x, y, a, lb, l, an)
        for pp in (p, np.where(rng.random(len(p)) < 0.5, rng.integers(0, 256, len(p)), rng.choice([0, 255], len(p)))):
            got, want = m.planar_dc_blend_pk(lg, x, y, a, l, pp), m.planar_dc_blend_scalar(lg, x, y, a, l, pp)
            assert np.array_equal(got, want)
