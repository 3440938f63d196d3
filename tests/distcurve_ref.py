"""Reference side of the distortion-curve tests: include/wrenc_distcurve.h restated in numpy.  The coefficients are the rate
histogram's (tests/ratecurve_ref.py: prediction from the neighbours' originals, Hadamard transform); each is quantised with
the step of every QP 0 .. 63 and the squared errors are summed per plane and QP."""
import numpy as np

import ratecurve_ref as rr
from complexity_ref import H8

QPS = 64
G = (40, 45, 51, 57, 64, 72)


def step(q):
    """T(q) in the units of m = 8 |c|."""
    return G[q % 6] << (q // 6)


STEPS = np.array([step(q) for q in range(QPS)], np.int64)


def errors(c):
    """(n, 64) int64: the quantisation error e of every coefficient of c (any shape) at every QP."""
    m = 8 * np.abs(np.asarray(c, np.int64)).reshape(-1, 1)
    level = (m + STEPS // 2) // STEPS
    return m - level * STEPS


def plane_curve(plane):
    """(64,) uint64: sum e e of the plane's coefficients per QP."""
    blk, pred = rr._plane_pred(plane.astype(np.int64))
    e = errors(H8 @ (blk - pred) @ H8)
    return (e * e).sum(axis=0).astype(np.uint64)


def dist_curve(y, cb, cr):
    """(3, 64) uint64: wrenc_dist_curve of a picture."""
    return np.stack([plane_curve(p) for p in (y, cb, cr)])


def predicted_psnr(curve, samples):
    """(64,) float: the PSNR a plane's curve predicts per QP, sse = sse8 / 4096 (infinity for 0)."""
    sse = np.asarray(curve, np.float64) / 4096.0
    with np.errstate(divide="ignore"):
        return np.where(sse > 0, 10.0 * np.log10(255.0 * 255.0 * samples / np.maximum(sse, 1e-300)), np.inf)
