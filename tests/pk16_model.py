"""NumPy models of the packed 16-bit row helpers (wrenc_amd/csrc/dev_pk16.h) with explicit i16 wrap-around, and the scalar
formulas they replace (copied from dev_predict.h as it stood before the rows were packed).  A packed helper works on
two i16 lanes at once; the lanes do not interact, so a model of one lane over arrays is a model of the helper.

Every model takes and returns int64 arrays; wrap16() is the ONLY place where a value is reduced to 16 bits, and it is
applied after every operation the device performs as a v_pk_*_i16 / _u16 instruction."""
import numpy as np


def wrap16(v):
    """The value an i16 register holds after a 16-bit add, subtract or multiply-low of wider operands."""
    v = np.asarray(v, np.int64)
    return ((v + 32768) & 0xFFFF) - 32768


def sar16(v, s):
    """v_pk_ashrrev_i16: arithmetic shift of an i16."""
    return wrap16(v) >> s


def clamp255(v):
    """v_pk_max_i16 with 0, v_pk_min_i16 with 255: any i16 in."""
    return np.minimum(np.maximum(wrap16(v), 0), 255)


# ---- bytes <-> pairs -------------------------------------------------------------------------------------------------
def perm(s0, s1, sel):
    """v_perm_b32 D = perm(S0, S1, sel) on uint32 arrays: selector byte 0..3 takes that byte of S1, 4..7 of S0, 0x0C is 0."""
    s0, s1 = np.asarray(s0, np.uint64), np.asarray(s1, np.uint64)
    both = s1 | (s0 << np.uint64(32))
    out = np.zeros_like(both)
    for k in range(4):
        b = (sel >> (8 * k)) & 0xFF
        assert b < 8 or b == 0x0C
        if b < 8:
            out |= ((both >> np.uint64(8 * b)) & np.uint64(0xFF)) << np.uint64(8 * k)
    return out.astype(np.uint32)


def pk_lo(w):
    return perm(0, w, 0x0C010C00)


def pk_hi(w):
    return perm(0, w, 0x0C030C02)


def pk_pack(a, b):
    return perm(b, a, 0x06040200)


def halves(w):
    """the two i16 lanes of a dword"""
    w = np.asarray(w, np.uint32).astype(np.int64)
    return wrap16(w & 0xFFFF), wrap16(w >> 16)


# ---- reconstruction (scalar: recon_row4 is not packed) ------------------------------------
def recon_rows(pred, res, org):
    """Rows of four as recon_row4 computes them: pred, org (n, 4) uint8, res (n, 4) int16 (any value) -> (rec (n, 4) uint8,
    ssd (n,) uint32): v = clamp((int16_t)(pred + res)); d = v - org; ssd += d * d."""
    v = wrap16(np.asarray(pred, np.int64) + np.asarray(res, np.int64))
    v = np.minimum(np.maximum(v, 0), 255)
    d = v - np.asarray(org, np.int64)
    return v.astype(np.uint8), ((d * d).sum(axis=1) & 0xFFFFFFFF).astype(np.uint32)


# ---- PDPC weights ------------------------------------------------------------------------------------------------------
def pdpc_w(n_scale, i):
    """dev_predict.h pdpc_w: 32 >> ((2 i) >> n_scale), 0 once that shift exceeds 5"""
    sh = (np.asarray(i, np.int64) << 1) >> n_scale
    return np.where(sh > 5, 0, 32 >> np.minimum(sh, 5))


def positions(x):
    """pk16_positions: x * 0x10001 + 0x10000 as the pair (x, x + 1)"""
    return halves(((np.asarray(x, np.int64) * 0x10001 + 0x10000) & 0xFFFFFFFF).astype(np.uint32))


def pdpc_w_pk(n_scale, pos):
    """pk16_pdpc_w2, one lane: v_pk_lshlrev_b16, v_pk_lshrrev_b16, v_pk_min_u16, v_pk_lshrrev_b16 (four bits of the count)"""
    sh = ((np.asarray(pos, np.int64) << 1) & 0xFFFF) >> n_scale
    return 32 >> (np.minimum(sh, 6) & 15)


# ---- the angular modes' PDPC blend ---------------------------------------------------------------------------------------
def mad16(a, b, c):
    """v_pk_mad_u16 / _i16: the low 16 bits of a * b + c"""
    return wrap16(np.asarray(a, np.int64) * np.asarray(b, np.int64) + np.asarray(c, np.int64))


def pdpc_blend_scalar(rs, w, v):
    """ang_row4 / rows_per_lane as they stood: pv = (int16_t)(mul24(rs, w) + mul24(64 - w, v) + 32) >> 6, clamped"""
    pv = wrap16(np.asarray(rs, np.int64) * w + (64 - np.asarray(w, np.int64)) * v + 32) >> 6
    return np.minimum(np.maximum(pv, 0), 255)


def pdpc_rs_scalar(kind, sv, corner, v):
    """rs = kind == 1 ? (int16_t)(sv - corner + v) : sv"""
    return wrap16(np.asarray(sv, np.int64) - corner + v) if kind == 1 else np.asarray(sv, np.int64) + 0 * np.asarray(v, np.int64)


def pdpc_blend_pk(rs, w, v):
    """pk16_pdpc_blend + pk16_clamp255, one lane"""
    return clamp255(sar16(mad16(64 - np.asarray(w, np.int64), v, mad16(rs, w, 32)), 6))


def pdpc_rs_pk(kind, sv, corner, v):
    """ang_row4: rs = kind == 1 ? pk16_add_wrap(s - corner, v) : s"""
    return wrap16(wrap16(np.asarray(sv, np.int64) - corner) + v) if kind == 1 else np.asarray(sv, np.int64) + 0 * np.asarray(v, np.int64)


def pdpc_folded_pk(kind, sv, corner, w, v):
    """rows_per_lane: wa, wc once per entry, pk16_pdpc_blend_folded + pk16_clamp255 per row"""
    w = np.asarray(w, np.int64)
    wa = 64 + 0 * w if kind == 1 else wrap16(64 - w)
    wc = mad16(w, -np.asarray(corner, np.int64), 32) if kind == 1 else 32 + 0 * w
    return clamp255(sar16(mad16(sv, w, mad16(v, wa, wc)), 6))


# ---- what v_dot4_i32_i8 leaves for the pairs -------------------------------------------------------------------------------
def ang_sample_scalar(coef, taps, luma):
    """(sum c (ref - 128) + 8192 + 32) >> 6 for the luma filters (coefficients sum to 64), (... + 4096 + 16) >> 5 for the
    chroma filter (sum 32): the value before any clamp"""
    s = (np.asarray(coef, np.int64) * (np.asarray(taps, np.int64) - 128)).sum(axis=-1)
    return (s + 8192 + 32) >> 6 if luma else (s + 4096 + 16) >> 5


# ---- PLANAR and DC -------------------------------------------------------------------------------------------------------
def planar_scalar(lg, x, y, a, lb, l, an):
    """planar_dc_row4 as it stood: ((n-1-y) a + (y+1) lb + (n-1-x) l + (x+1) an + n) >> (lg + 1), & 0xFF"""
    n = 1 << lg
    pv = (n - 1 - y) * a + (y + 1) * lb
    ph = (n - 1 - x) * l + (x + 1) * an
    return ((pv + ph + n) >> (lg + 1)) & 0xFF


def planar_pk(lg, x, y, a, lb, l, an):
    """pk16_planar2, one lane: the row's scalars in 32 bits, two v_pk_mad_u16, v_pk_lshrrev_b16"""
    n = 1 << lg
    ny, dl, k = n - 1 - y, an - l, (n - 1) * l + an + (y + 1) * lb + n
    t = mad16(a, wrap16(ny), mad16(x, wrap16(dl), wrap16(k)))
    return (t & 0xFFFF) >> (lg + 1)


def planar_dc_blend_scalar(lg, x, y, a, l, p):
    """p = (int16_t)(l wl + a wt + (64 - wt - wl) p + 32) >> 6, clamped"""
    ns = (2 * lg - 2) >> 2
    wl, wt = pdpc_w(ns, x), pdpc_w(ns, y)
    v = wrap16(l * wl + a * wt + (64 - wt - wl) * p + 32) >> 6
    return np.minimum(np.maximum(v, 0), 255)


def planar_dc_blend_pk(lg, x, y, a, l, p):
    """pk16_planar_dc_blend, one lane: three v_pk_mad_u16, v_pk_sub_i16, v_pk_ashrrev_i16 and NO clamp"""
    ns = (2 * lg - 2) >> 2
    wl, wt = pdpc_w_pk(ns, x), pdpc_w(ns, y)
    t = mad16(a, wt, mad16(wl, l, 32))
    return sar16(mad16(wrap16(64 - wt - wl), p, t), 6)
