"""Groups of blocks for the device functions the search calls on more than one block at a time (test_pair_inputs.py on the
CPU, test_gpu_solo_groups.py on the device): the Cb + Cr pair through quantize_solo's two-block path, and the groups of
two to four blocks the transforms and the dequantiser take at a base offset.

Everything is built from the reference's quantiser formulas in quant_inputs.py and the kinds of pack_sparse_inputs.py,
never from device code.  Five kinds of coefficient block:

    zero, quiet, live   as pack_sparse_inputs.block;
    low     a quiet block with coefficients of levels 2 .. 4 only in the first LOW_K sub-blocks of the scan (the ones
            nearest DC): the walk's head -- the end of the chain it reaches last, the high frequencies -- is long and
            proven zero.  At side 4 a block is a single sub-block: the levels sit in its first eight scan positions;
    stray   a low block with one coefficient of level 2 or more in the LAST sub-block of the scan: no head, the walk covers
            the whole chain.

LOW_K depends on the block's place in the pair where the side allows it, so that two low blocks side by side end their
walks at different sub-blocks.  What the kinds deliver (and where the oracle's model of the head proof ends each walk) is
read off the oracle in test_pair_inputs.py, not taken from this description."""
import itertools

import numpy as np

import pack_sparse_inputs as ps
import quant_inputs as qi

KINDS = ps.KINDS + ("low", "stray")
SIDES = (4, 8, 16)                      # the chroma blocks of an 8x8, 16x16 and 32x32 CU
QPS = ps.QPS
LOW_K = {4: (1, 1), 8: (1, 2), 16: (3, 1)}   # side -> sub-blocks (in scan order) that hold a low block's levels, by place


def low_k(n, place):
    return LOW_K[n][place & 1]


def block(kind, qp, n, place):
    """One block of a kind; `place` is its position in the pair (it varies the draw, and LOW_K)."""
    if kind in ps.KINDS:
        return ps.block(kind, qp, n, place)
    rng = np.random.default_rng(6100 + 1000 * KINDS.index(kind) + 37 * qp + 11 * n + place)
    b = ps.block("quiet", qp, n, 20 + place)
    order = qi.scan(n)
    near_dc = order[:8] if n == 4 else order[:16 * low_k(n, place)]
    for at in rng.choice(len(near_dc), 3, replace=False):
        neg = bool(rng.integers(0, 2))
        v = qi.coef_for_level(int(rng.integers(2, 5)), qp, n, neg)
        b[near_dc[at]] = -v if neg else v
    if kind == "stray":
        last = order[-4:] if n == 4 else order[-16:]
        neg = bool(rng.integers(0, 2))
        v = qi.coef_for_level(int(rng.integers(3, 5)), qp, n, neg)      # level 2 .. 5
        b[last[int(rng.integers(0, len(last)))]] = -v if neg else v
    return b


def mixtures(qp, n):
    """((kind 0, kind 1), (block 0, block 1)) for every ordered pair of the five kinds."""
    return [((k0, k1), (block(k0, qp, n, 0), block(k1, qp, n, 1))) for k0, k1 in itertools.product(KINDS, repeat=2)]


def qp_pairs(qp, n, seeds=qi.CLASS_SEEDS):
    """The blocks of qi.qp_blocks paired with the same list reversed and rotated: (tagged blocks of position 0, tagged
    blocks of position 1); pair i is (first[i], second[i]).  Rotated by one, or by the least amount beyond that at which
    every class (the generator's tag) sits beside another class in both positions: with eight blocks per draw the
    rotation by one leaves class (d) beside (d) only."""
    first = qi.qp_blocks(qp, n, seeds)
    rev = first[::-1]
    tags = {t for t, _ in first}
    for r in range(1, len(first)):
        second = rev[r:] + rev[:r]
        mixed = [(t0, t1) for (t0, _), (t1, _) in zip(first, second) if t0 != t1]
        if {t0 for t0, _ in mixed} == tags and {t1 for _, t1 in mixed} == tags:
            return first, second
    raise AssertionError("no rotation mixes the classes")


def bound_pairs(qp, n):
    """(name, (block 0, block 1)): every bound block beside itself, beside a zero block and beside +-3 noise, in both
    positions."""
    zero = np.zeros((n, n), np.int16)
    out = []
    for i, (name, b) in enumerate(qi.bound_blocks(qp, n)):
        noise = qi.noise3(n, 40 + i)
        out += [(name + "+self", (b, b)), (name + "+zero", (b, zero)), ("zero+" + name, (zero, b)),
                (name + "+noise", (b, noise)), ("noise+" + name, (noise, b))]
    return out


LIMIT_SEEDS = 3


def limit_pairs(qp, n, seed):
    """(pairs at the limit, pairs over it): the block with a coefficient at the tables' last entry (over: one step beyond)
    in position 0 and in position 1, beside a harmless block."""
    at, over, fill = qi.limit_block(qp, n, seed, False), qi.limit_block(qp, n, seed, True), qi.harmless_block(qp, n, seed)
    return [(at, fill), (fill, at)], [(over, fill), (fill, over)]


# ---- transform and dequantiser groups: (log2n, nb, o1) as the search calls them ----
TRANSFORM_SHAPES = ((2, 2, 0), (3, 2, 0), (4, 2, 0),          # the chroma pair of an 8x8 / 16x16 / 32x32 CU
                    (3, 1, 0), (3, 3, 0),                     # luma of an 8x8 pack of one to three candidates (two: above)
                    (4, 1, 0), (3, 2, 256), (3, 4, 512))      # a 16x16 pack: luma (two: above), then chroma behind it
RESIDUAL_KINDS = ("plus255", "minus255", "checker255", "zero", "noise")
COEF_KINDS = ("plus32767", "minus32767", "row32767", "zero", "small")
LEVEL_KINDS = ("plus2046", "minus2046", "checker2046", "zero", "noise")


def _kind_block(kind, n, seed):
    rng = np.random.default_rng(8300 + seed)
    yy, xx = np.indices((n, n))
    odd = ((yy + xx) & 1).astype(bool)
    if kind == "zero":
        return np.zeros((n, n), np.int16)
    if kind == "noise":
        return rng.integers(-255, 256, (n, n)).astype(np.int16)
    if kind == "small":
        return rng.integers(-64, 65, (n, n)).astype(np.int16)
    if kind.startswith("row"):
        b = np.zeros((n, n), np.int16)
        b[int(rng.integers(0, n)), :] = int(kind[3:])
        return b
    for prefix, sign in (("plus", 1), ("minus", -1)):
        if kind.startswith(prefix):
            return np.full((n, n), sign * int(kind[len(prefix):]), np.int16)
    top = int(kind[len("checker"):])
    return np.where(odd, -top, top).astype(np.int16)


def _groups(kinds, log2n, nb):
    """len(kinds) + 1 groups of nb blocks: group r holds the kinds r, r + 1, ... (every kind in every position, never beside
    itself unless nb exceeds the kinds), the last one nb different draws of the last kind (noise)."""
    n = 1 << log2n
    out = [np.stack([_kind_block(kinds[(r + j) % len(kinds)], n, 16 * r + j) for j in range(nb)]) for r in range(len(kinds))]
    out.append(np.stack([_kind_block(kinds[-1], n, 200 + j) for j in range(nb)]))
    return np.stack(out)


def residual_groups(log2n, nb):
    """(groups, nb, n, n): all +255, all -255, the +-255 checkerboard, zero and noise, every block of a group another kind."""
    return _groups(RESIDUAL_KINDS, log2n, nb)


def coef_groups(log2n, nb):
    """Inputs of the inverse transform: all +32767 / -32767 (the first stage's clip), a single row of 32767, zero, and small
    blocks beside them."""
    return _groups(COEF_KINDS, log2n, nb)


def level_groups(log2n, nb):
    """Inputs of the dequantiser: the largest coded level (2 * 1023) with either sign and as a checkerboard, zero, noise."""
    return _groups(LEVEL_KINDS, log2n, nb)


# ---- what a group is compared with ----
class Oracle:
    """po.quantize / level_cost / dequantize of a block, once per block."""

    def __init__(self, qp):
        from oracle import pyoracle as po
        self.po, self.qp, self.seen = po, qp, {}

    def __call__(self, b):
        key = (b.shape[0], b.tobytes())
        if key not in self.seen:
            ref = self.po.quantize(b, self.qp)
            self.seen[key] = (ref, self.po.level_cost(ref), self.po.dequantize(ref, self.qp))
        return self.seen[key]


def expected(pairs, oracle):
    """(levels (count, 2, n, n), cost per pair, any per pair) of pairs of blocks: each block through the oracle alone; the
    cost of a pair is the sum of its blocks' costs, `any` is "some level of the pair is non-zero"."""
    levels = np.stack([np.stack([oracle(b)[0] for b in pair]) for pair in pairs])
    cost = np.array([sum(oracle(b)[1] for b in pair) for pair in pairs], np.int64)
    return levels, cost, levels.reshape(len(pairs), -1).any(axis=1)


def differences(got, want):
    """[(pair, what)] wherever (levels, cost, any) of `got` is not exactly `want`; empty = equal."""
    out = []
    for i in range(len(want[0])):
        for b in range(want[0].shape[1]):
            if not np.array_equal(got[0][i, b], want[0][i, b]):
                out.append((i, "levels of block %d" % b))
        if int(got[1][i]) != int(want[1][i]):
            out.append((i, "cost"))
        if bool(got[2][i]) != bool(want[2][i]):
            out.append((i, "any"))
    return out
