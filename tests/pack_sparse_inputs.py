"""Packs for quantize_pk whose chains are zero, quiet or live in every combination (test_pack_sparse_inputs.py on the CPU,
test_gpu_pack_sparse.py on the device).

The packed quantiser traces a chain only where it has something to trace, and hands back per block whether it holds a
level; the packs here put every mixture of chains with and without levels side by side.  Three kinds of block, built
from the reference's quantiser formulas in quant_inputs.py, never from device code:

    zero    every coefficient 0;
    quiet   non-zero coefficients, each well below half a quantiser step (quotient 0), so that every level is zero: the
            kind of block the head proof of the device's walk disposes of without walking it;
    live    coefficients of levels 2 .. 4 at a few places (significant positions), over the same quiet background.

What the kinds deliver is read off the oracle's output in test_pack_sparse_inputs.py (quiet: coefficients non-zero, levels
all zero; live: levels not all zero), not taken from this description."""
import itertools

import numpy as np

import quant_inputs as qi

KINDS = ("zero", "quiet", "live")
QPS = (22, 32, 42)
PACKS = qi.PACKS   # (3, 1), (3, 2), (3, 3), (4, 1), (4, 2)


def block(kind, qp, n, place):
    """One block of a kind; `place` (the chain's position in the pack) only varies the draw."""
    b = np.zeros((n, n), np.int16)
    if kind == "zero":
        return b
    rng = np.random.default_rng(5100 + 1000 * KINDS.index(kind) + 37 * qp + 11 * n + place)
    small = max(1, qi.coef_below(0, qp, n) // 3)           # a sixth of a level
    for at in rng.choice(n * n, max(3, n * n // 8), replace=False):
        b[at // n, at % n] = small * (1 if rng.integers(0, 2) else -1)
    if kind == "live":
        for at in rng.choice(n * n, max(2, n * n // 32), replace=False):
            neg = bool(rng.integers(0, 2))
            v = qi.coef_for_level(int(rng.integers(2, 5)), qp, n, neg)
            b[at // n, at % n] = -v if neg else v
    return b


def chroma_patterns(nc):
    """The kinds of a pack's 2 nc chroma chains (chain 2 c + plane): all quiet; one chain live, in each position; all live."""
    nch = 2 * nc
    out = [("quiet",) * nch]
    out += [tuple("live" if i == k else "quiet" for i in range(nch)) for k in range(nch)]
    out.append(("live",) * nch)
    return out


def plan(qp, log2n, nc):
    """Every assignment of the three kinds to the pack's nc luma chains crossed with chroma_patterns(nc).
    Returns (kinds, luma, chroma): kinds[p] = (luma kinds, chroma kinds) of pack p, which holds luma[p * nc + c] and
    chroma[(p * nc + c) * 2 + pl] -- the layout of quant_inputs.pack_array."""
    n = 1 << log2n
    kinds, luma, chroma = [], [], []
    for lk in itertools.product(KINDS, repeat=nc):
        for ck in chroma_patterns(nc):
            kinds.append((lk, ck))
            luma += [block(k, qp, n, c) for c, k in enumerate(lk)]
            chroma += [block(k, qp, n // 2, 8 + i) for i, k in enumerate(ck)]
    return kinds, luma, chroma
