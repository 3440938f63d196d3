"""A numpy model of the 8x8 and 16x16 transforms as the device runs them (wrenc_amd/csrc/dev_transform.h fwd_dct_mfma /
inv_dct_mfma): the operand tables as the host fills them (DevConst::fdct_b ...), the digit and byte splits, one matrix
product per MFMA with the lane layout of the hardware instruction, recombination, offsets, shifts and the clamp -- lane by
lane, so an index slip in a table or in a lane's share of an operand shows here, without a device.  `Bounds` records the
largest magnitude of every kind of intermediate that passes through it.  Also the inputs the model test and the GPU test
(tests/test_gpu_dct_mfma.py) share."""
import functools

import numpy as np

from oracle import pyoracle as po

SEL_LO, SEL_HI, SEL_ZERO = "lo", "hi", "zero"


def basis(n):
    return po.dct64()[::64 // n, :n].astype(np.int64)      # T_N[u][x]


def yk(j, h):
    """row of accumulator register j in lane half h (v_mfma_i32_32x32x*: D[8 (w / 4) + 4 h + w % 4][n] in lane n + 32 h)"""
    return 8 * (j // 4) + 4 * h + j % 4


class Bounds:
    def __init__(self):
        self.worst = {}

    def see(self, name, a):
        a = np.asarray(a, np.int64)
        lo, hi = int(a.min()), int(a.max())
        w = self.worst.setdefault(name, [lo, hi])
        w[0], w[1] = min(w[0], lo), max(w[1], hi)

    def mag(self, name):
        return max(-self.worst[name][0], self.worst[name][1])


def basis_abs_row_sum(n):
    return int(np.abs(basis(n)).sum(axis=1).max())


@functools.lru_cache(maxsize=None)
def tables(n):
    """the host's fill of the operand tables (const_block.cpp fill_dev_const), [m][h][j]"""
    T = basis(n)
    s = T.sum(axis=0)                                      # S[y] = sum_i T[i][y]
    t = {"fdct_b": np.zeros((32, 2, 16), np.int64), "idct_b": np.zeros((32, 2, 16), np.int64),
         "fdct_p": np.zeros((32, 2, 8 if n == 16 else 16), np.int64),
         "idct_p": np.zeros((32, 2, 16 if n == 16 else 8), np.int64),
         "k1": np.array([128 * s[m % n] + 64 for m in range(32)], np.int64),
         "k2": np.array([[128 * s[yk(w, h)] + 2048 for w in range(n // 2)] for h in range(2)], np.int64)}
    for m in range(32):
        for h in range(2):
            for j in range(16):
                blk, x = (h, j) if n == 16 else (2 * h + j // 8, j % 8)
                if m // n == blk:
                    t["fdct_b"][m, h, j] = T[m % n, x]
                    t["idct_b"][m, h, j] = T[x, m % n]
                if n == 16:
                    if j < 8 and m < 16:
                        t["fdct_p"][m, h, j] = T[m, yk(j, h)]
                    if j // 8 == m // 16:
                        t["idct_p"][m, h, j] = T[yk(j % 8, h), m % 16]
                else:
                    if j // 4 == m // 8 and m // 8 < 3:
                        t["fdct_p"][m, h, j] = T[m % 8, 4 * h + j % 4]
                    if j < 8 and j // 4 == m // 16 and m % 16 < 8:
                        t["idct_p"][m, h, j] = T[4 * h + j % 4, m % 16]
    for v in t.values():
        assert np.abs(v).max() < 2 ** 31
    for name in ("fdct_b", "idct_b", "fdct_p", "idct_p"):
        assert t[name].min() >= -128 and t[name].max() <= 127, "the basis fits signed bytes"
    return t


def mfma(a, b, c, bounds, name):
    """v_mfma_i32_32x32x(2 * bytes)_i8: a, b (64 lanes, bytes per lane), c (64, 16) -> d (64, 16).  Operand byte j of lane
    m + 32 h is element (m, k = (h, j)) of A / (k, n = m) of B; the same slot order on both sides, whatever k it is."""
    assert a.min() >= -128 and a.max() <= 127 and b.min() >= -128 and b.max() <= 127, "%s: an operand leaves i8" % name
    kb = a.shape[1]
    A = np.concatenate([a[:32], a[32:]], axis=1)           # (32, 2 kb): row m, slots (h, j)
    B = np.concatenate([b[:32], b[32:]], axis=1).T         # (2 kb, 32)
    assert A.shape == (32, 2 * kb)
    # every partial sum of a dot product, in slot order, stays in i32 if the sum of magnitudes does
    bounds.see(name + " sum of |products|", np.abs(A) @ np.abs(B) + np.abs(c).max())
    D = A @ B
    d = np.zeros((64, 16), np.int64)
    for h in range(2):
        for w in range(16):
            d[32 * h:32 * h + 32, w] = D[yk(w, h), :]
    d += c
    bounds.see(name + " accumulator", d)
    return d


def sext8(v):
    return ((np.asarray(v, np.int64) & 255) ^ 128) - 128


def rows_operand(src, b0, nb, n_side, sel, add, xm):
    """mfma_rows: per lane the 16 bytes of its row of the blocks of its half; sel / add / xm per lane as the device picks."""
    per = 32 // n_side
    out = np.zeros((64, 16), np.int64)
    for lane in range(64):
        n, h = lane & 31, lane >> 5
        row = n & (n_side - 1)
        for j in range(16):
            blk = b0 + (h if n_side == 16 else 2 * h + j // 8)
            col = j if n_side == 16 else j % 8
            if blk > nb - 1:
                continue                                    # zero selector
            v = (int(src[blk, row, col]) + add[lane]) & 0xFFFF   # wrapping i16 add
            byte = (v & 255) if sel[lane] == SEL_LO else (v >> 8)
            out[lane, j] = sext8(byte ^ xm[lane])
    assert per in (2, 4)
    return out


def fwd_model(groups, bounds):
    """groups: (nb, n, n) residuals within +-255 -> coefficients, as fwd_dct_mfma<LG>"""
    groups = np.asarray(groups, np.int64)
    nb, n, _ = groups.shape
    lg = n.bit_length() - 1
    t = tables(n)
    nh = n // 2
    out = np.zeros_like(groups)
    lanes = np.arange(64)
    d = (lanes & 31) >> 4
    sel = [SEL_HI if x else SEL_LO for x in d]
    add = [128 if x else 0 for x in d]
    tB = t["fdct_b"].transpose(1, 0, 2).reshape(64, 16)    # lane n + 32 h
    tP = t["fdct_p"].transpose(1, 0, 2).reshape(64, -1)
    z = np.zeros((64, 16), np.int64)
    for b0 in range(0, nb, 32 // n):
        a = rows_operand(groups, b0, nb, n, sel, add, [0] * 64)
        bounds.see("fwd stage-1 digit", a)
        acc = mfma(a, tB, z, bounds, "fwd stage 1")
        H = ((acc[:, 8:8 + nh] << 8) + acc[:, :nh] + (1 << (lg - 2))) >> (lg - 1)
        bounds.see("fwd H", H)
        d0, d1, d2 = sext8(H), sext8((H + 128) >> 8), sext8((H + 32896) >> 16)
        assert np.array_equal(d0 + 256 * d1 + 65536 * d2, H), "three balanced digits rebuild H"
        bounds.see("fwd stage-2 digit 2", d2)
        if n == 16:
            acc = mfma(tP, d2, z, bounds, "fwd stage 2")
            acc[:, :nh] <<= 8
            acc = mfma(tP, d1, acc, bounds, "fwd stage 2")
            acc[:, :nh] = (acc[:, :nh] << 8) + (1 << (lg + 5))
            bounds.see("fwd stage 2 shifted", acc)
            acc = mfma(tP, d0, acc, bounds, "fwd stage 2")
        else:
            b = np.concatenate([d0, d1, d2, np.zeros((64, 4), np.int64)], axis=1)
            acc = mfma(tP, b, z, bounds, "fwd stage 2")
            acc[:, :nh] = (((acc[:, 8:8 + nh] << 8) + acc[:, 4:4 + nh]) << 8) + acc[:, :nh] + (1 << (lg + 5))
            bounds.see("fwd stage 2 shifted", acc)
        for lane in range(64):
            nn, h = lane & 31, lane >> 5
            blk = b0 + (nn >> lg)
            if blk < nb:
                for w in range(nh):
                    out[blk, yk(w, h), nn & (n - 1)] = acc[lane, w] >> (lg + 6)
    assert np.abs(out).max() < 2 ** 15, "the coefficient is stored as i16"
    return out


def inv_model(groups, bounds):
    """groups: (nb, n, n) dequantised coefficients d[i][x], any i16 -> residuals, as inv_dct_mfma<LG> (which reads them
    transposed from r2)"""
    groups = np.asarray(groups, np.int64)
    nb, n, _ = groups.shape
    lg = n.bit_length() - 1
    t = tables(n)
    nh = n // 2
    dT = groups.transpose(0, 2, 1)                          # [blk][x][i]
    out = np.zeros_like(groups)
    lanes = np.arange(64)
    b = (lanes & 31) >> 4
    sel = [SEL_HI if x else SEL_LO for x in b]
    xm = [0 if x else 0x80 for x in b]
    tB = t["idct_b"].transpose(1, 0, 2).reshape(64, 16)
    tP = t["idct_p"].transpose(1, 0, 2).reshape(64, -1)
    k1 = np.concatenate([t["k1"], t["k1"]])[:, None]
    k2 = np.zeros((64, 16), np.int64)
    for h in range(2):
        k2[32 * h:32 * h + 32, :nh] = t["k2"][h]
    z = np.zeros((64, 16), np.int64)
    for b0 in range(0, nb, 32 // n):
        a = rows_operand(dT, b0, nb, n, sel, [0] * 64, xm)
        acc = mfma(a, tB, z, bounds, "inv stage 1")
        pre = (acc[:, 8:8 + nh] << 8) + acc[:, :nh] + k1
        bounds.see("inv stage 1 recombined", pre)
        V = np.clip(pre >> 7, -32768, 32767)
        lo, hi = sext8((V & 255) ^ 0x80), sext8((V >> 8) & 255)
        assert np.array_equal(256 * hi + lo + 128, V)
        acc = mfma(tP, np.concatenate([lo, hi], axis=1), k2, bounds, "inv stage 2")
        r = ((acc[:, 8:8 + nh] << 8) + acc[:, :nh])
        bounds.see("inv stage 2 recombined", r)
        r >>= 12
        for lane in range(64):
            nn, h = lane & 31, lane >> 5
            blk = b0 + (nn >> lg)
            if blk < nb:
                for w in range(nh):
                    out[blk, nn & (n - 1), yk(w, h)] = sext16(r[lane, w])
    return out


def sext16(v):
    return ((int(v) & 0xFFFF) ^ 0x8000) - 0x8000


# ---- inputs ----
def fwd_inputs(n, seed=15):
    """name -> (n, n) residual block, every one within +-255"""
    rng = np.random.default_rng(seed + n)
    yy, xx = np.mgrid[0:n, 0:n]
    d = {"plus": np.full((n, n), 255), "minus": np.full((n, n), -255), "checker": np.where((yy + xx) & 1, -255, 255)}
    for y in range(n):
        for x in range(n):
            for v in (255, -255):
                b = np.zeros((n, n), np.int64)
                b[y, x] = v
                d["impulse%+d@%d,%d" % (v, y, x)] = b
    for i in range(8):
        d["noise%d" % i] = rng.integers(-255, 256, (n, n))
    return {k: v.astype(np.int16) for k, v in d.items()}


def inv_inputs(n, seed=16):
    """name -> (n, n) dequantised block over the whole i16 range"""
    rng = np.random.default_rng(seed + n)
    d = {"max": np.full((n, n), 32767), "min": np.full((n, n), -32768)}
    row = np.zeros((n, n), np.int64)
    row[0, :] = 32767
    d["row"] = row
    for i in range(n):
        for x in range(n):
            for v in (32767, -32768, 1):
                b = np.zeros((n, n), np.int64)
                b[i, x] = v
                d["impulse%+d@%d,%d" % (v, i, x)] = b
    for i in range(8):
        d["normal%d" % i] = np.clip(np.rint(rng.normal(0, 400, (n, n))), -32768, 32767)
        d["full%d" % i] = rng.integers(-32768, 32768, (n, n))
    return {k: v.astype(np.int16) for k, v in d.items()}


def as_groups(blocks, nb):
    """the blocks dealt into groups of nb so that every block of a group is of another kind: block i of group g is
    blocks[(g + i * stride) % len], stride = len // nb (the kinds lie in runs in the input order)"""
    blocks = list(blocks)
    m = len(blocks)
    stride = max(m // nb, 1)
    return np.stack([np.stack([blocks[(g + i * stride) % m] for i in range(nb)]) for g in range(m)])
