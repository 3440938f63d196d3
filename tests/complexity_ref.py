"""Reference side of the device-complexity tests: include/wrenc_gpu.h's wrenc_gpu_complexity restated in numpy, and the
pictures the tests share."""
import numpy as np

_H2 = np.array([[1, 1], [1, -1]], np.int64)
H8 = np.kron(np.kron(_H2, _H2), _H2)      # the unnormalised 8x8 Hadamard matrix (+-1)


def block_act(plane):
    """(h/8, w/8) int64: per picture-aligned 8x8 block, sum |H8 X H8| over the 63 coefficients other than DC."""
    h, w = plane.shape
    x = plane.astype(np.int64).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    coef = H8 @ x @ H8
    return np.abs(coef).sum(axis=(2, 3)) - np.abs(coef[:, :, 0, 0])


def complexity(y, cb, cr):
    """{"satd": [Y, Cb, Cr], "ctu_satd": (h/32, w/32) uint32}: a CTU is 4x4 luma and 2x2 blocks of each chroma plane."""
    acts = [block_act(p) for p in (y, cb, cr)]
    h, w = y.shape

    def ctus(a, n):
        return a.reshape(h // 32, n, w // 32, n).sum(axis=(1, 3))

    ctu = ctus(acts[0], 4) + ctus(acts[1], 2) + ctus(acts[2], 2)
    return {"satd": [int(a.sum()) for a in acts], "ctu_satd": ctu.astype(np.uint32)}


def check(got, y, cb, cr, ref=None):
    ref = ref if ref is not None else complexity(y, cb, cr)
    assert got["satd"] == ref["satd"], (got["satd"], ref["satd"])
    if got["ctu_satd"] is not None:
        bad = np.argwhere(got["ctu_satd"] != ref["ctu_satd"])
        assert bad.size == 0, ("CTU (row, column)", bad[:8].tolist())


def bent_block():
    """An 8x8 0/255 block whose 63 non-DC coefficients all have the magnitude 4 * 255 (a bent function of the six
    index bits: x0 x1 ^ x2 x3 ^ x4 x5): act = 64,260, within 1 % of what Cauchy-Schwarz allows a two-level block
    (255 / 2 * sqrt(63 * 4096) = 64,770), and every stage of the transform at its widest."""
    i = np.arange(64)
    f = ((i & 1) & (i >> 1 & 1)) ^ ((i >> 2 & 1) & (i >> 3 & 1)) ^ ((i >> 4 & 1) & (i >> 5 & 1))
    return (255 * f).astype(np.uint8).reshape(8, 8)


def tiled(block, w, h):
    return (np.tile(block, (h // 8, w // 8)), np.tile(block, (h // 16, w // 16)), np.tile(255 - block, (h // 16, w // 16)))


def checker1(w, h):
    """0 / 255 at period 1: all of a block's energy in one coefficient (|coefficient| = 32 * 255 = 8160)."""
    yy, xx = np.mgrid[0:h, 0:w]
    y = (255 * ((xx + yy) & 1)).astype(np.uint8)
    c = y[:h // 2, :w // 2]
    return y, c.copy(), (255 - c).astype(np.uint8)
