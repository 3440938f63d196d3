"""Coefficient blocks aimed at the quantiser's register paths (wrenc_amd/csrc/dev_quant.h): the parity masks and the
state-0 flag a walker takes from the round's ballots, the three table entries a chunk entry selects by the parity of the
quotient, the table's LDS edge, the head test's two outcomes and the trace's shares of a chain.

As in quant_inputs.py everything comes from the reference's formulas (quotient, level scale, scan), never from device
code; which case a block reaches is read off the oracle (test_quant_regs_inputs.py), not assumed here.  Position p below
is the walk's: p = N - 1 is the DC position, the walk goes from there down to p = 0, and p & 15 == 15 is the first
position of a 4x4 sub-block in coding order.  One QP throughout: at QP 10 a 16-bit coefficient reaches a level of 455 at
4x4 and more at the larger sizes, so every size has coefficients on both sides of the tables' 256 LDS entries, and no
block here holds a level above 258 (the reference panics at 1024).
"""
import numpy as np

import quant_inputs as qi

QP = 10
EDGE = (253, 254, 255, 256, 257, 258)     # a + 3, a = quotient / 2: the largest table entry a chunk entry reads


def place(b, p, v):
    """Coefficient v at walk position p of block b."""
    n = b.shape[0]
    y, x = qi.scan(n)[n * n - 1 - p]
    b[y, x] = v


def at(b, p):
    n = b.shape[0]
    y, x = qi.scan(n)[n * n - 1 - p]
    return int(b[y, x])


def coef(qd, n, neg=False):
    """A coefficient of quotient qd (the largest magnitude there is), negative with neg."""
    v = qi.coef_below(qd, QP, n, neg)
    return -v if neg else v


def quotients(b):
    """Quotient of every walk position p of a block."""
    n = b.shape[0]
    return [qi.quotient(at(b, p), QP, n) for p in range(n * n)]


def parity_block(n, flip):
    """Every position non-zero, the quotient's parity (p + flip) & 1: both blocks together hold both parities at every
    position of every sub-block, the DC position included."""
    b = np.zeros((n, n), np.int16)
    for p in range(n * n):
        place(b, p, coef(2 + ((p + flip) & 1) + 2 * ((p >> 1) % 3), n, neg=bool((p >> 2) & 1)))
    return b


def edge_one_block(n, a3, k):
    """Quotients 3 .. 6 everywhere and ONE coefficient whose chunk entry reads up to table entry a3 (one lane on the slow
    path): of either parity, at the DC position, at p = 0 or inside the block, in turn with k."""
    N = n * n
    rng = np.random.default_rng(8100 + 10 * n + k)
    b = np.zeros((n, n), np.int16)
    for p in range(N):
        place(b, p, coef(int(rng.integers(3, 7)), n, neg=bool(rng.integers(0, 2))))
    p = (N - 1, 0, N // 2 + 5, 15, N - 16, 7)[k % 6]
    place(b, p, coef(2 * (a3 - 3) + (k & 1), n, neg=bool(k & 2)))
    return b


def edge_all_block(n, seed):
    """Every position at the tables' LDS edge: a + 3 in 253 .. 258, both parities, both signs (all lanes on the slow path
    or, where a draw stays below 253, beside it)."""
    rng = np.random.default_rng(8200 + 10 * n + seed)
    b = np.zeros((n, n), np.int16)
    for p in range(n * n):
        place(b, p, coef(int(rng.integers(2 * (EDGE[0] - 3), 2 * (EDGE[-1] - 3) + 2)), n, neg=bool(rng.integers(0, 2))))
    return b


def head_block(n, sbs, amp, seed):
    """Significant coefficients (quotients 4 .. 12) from position 16 sbs up to the DC position, the first of them AT 16 sbs,
    and below it -- the head, sub-blocks 0 .. sbs - 1 -- zeros and coefficients of at most `amp` times the largest magnitude of
    quotient 1.  Whether the head test passes there is the oracle model's to say."""
    N = n * n
    rng = np.random.default_rng(8300 + 1000 * n + 10 * sbs + seed)
    b = np.zeros((n, n), np.int16)
    for p in range(16 * sbs, N):
        place(b, p, coef(int(rng.integers(4, 13)), n, neg=bool(rng.integers(0, 2))))
    top = qi.coef_below(1, QP, n)
    for p in range(16 * sbs):
        if rng.integers(0, 3):
            place(b, p, int(round(amp * top * rng.random())) * (1 if rng.integers(0, 2) else -1))
    return b


def adj_block(n, significant):
    """A chain that is walked from end to end although most of it is zero: the largest coefficient of quotient 1 at p = 2
    ends the proven region inside sub-block 0 (at 4x4 and 8x8; at the larger sizes it is inside the region, and the heads
    that fail their test are the chains walked through zeros: test_quant_regs_inputs.py).  With `significant`, quotients 4 .. 9 in the last eight positions (the first
    significant position is N - 8: every sub-block's first position but the DC sub-block's is a zero kept inside the
    trailing run); without, nothing significant at all (so is the DC position)."""
    N = n * n
    rng = np.random.default_rng(8400 + n + (1 if significant else 0))
    b = np.zeros((n, n), np.int16)
    if significant:
        for p in range(N - 8, N):
            place(b, p, coef(int(rng.integers(4, 10)), n, neg=bool(rng.integers(0, 2))))
    place(b, 2, coef(1, n))
    place(b, min(9, N - 9), coef(1, n, neg=True))
    return b


def single_block(n, first, v):
    """One coefficient v, at the walk's first position (the DC position) or at its last."""
    b = np.zeros((n, n), np.int16)
    place(b, n * n - 1 if first else 0, v)
    return b


# (sub-blocks of head, amplitude, seed) per size, found on the CPU with the oracle's model (test_quant_regs_inputs.py
# asserts each outcome): heads whose test passes -- at 8x8 with every start a trace can have, 16, 32 and 48 -- and heads whose
# test fails, so that the chain is walked to its end and traced from 0.  A 4x4 block is one sub-block and has no head; at
# 32x32, which only the one-block quantiser takes, no block of this recipe fails its test.
HEADS = {
    4: {"pass": (), "fail": ()},
    8: {"pass": ((1, 0.2, 0), (2, 0.2, 0), (3, 0.2, 0)), "fail": ((1, 0.5, 2), (2, 0.5, 1), (3, 0.8, 0))},
    16: {"pass": ((1, 0.2, 0), (5, 0.2, 0), (15, 0.2, 0)), "fail": ((2, 0.9, 1), (5, 0.8, 5), (15, 0.8, 1))},
    32: {"pass": ((1, 0.2, 0), (21, 0.2, 0), (63, 0.2, 0)), "fail": ()},
}


def pool(n):
    """(name, block) of every kind above at side n."""
    out = [("parity0", parity_block(n, 0)), ("parity1", parity_block(n, 1))]
    out += [("edge_one_%d" % a3, edge_one_block(n, a3, k)) for k, a3 in enumerate(EDGE)]
    out += [("edge_all_%d" % s, edge_all_block(n, s)) for s in range(2)]
    for kind in ("pass", "fail"):
        out += [("head_%s_%d" % (kind, sbs), head_block(n, sbs, amp, seed)) for sbs, amp, seed in HEADS[n][kind]]
    out += [("adj_sig", adj_block(n, True)), ("adj_nosig", adj_block(n, False))]
    lvl1 = qi.coef_below(2, QP, n)
    for first in (True, False):
        where = "first" if first else "last"
        out += [("one_%s_%+d" % (where, v), single_block(n, first, v)) for v in (1, -1)]
        out += [("level1_%s_%+d" % (where, s), single_block(n, first, s * lvl1)) for s in (1, -1)]
    return out


def pack_plan(log2n, nc):
    """Packs of quantize_pk: every luma block of pool(n) once (the pool's order puts a passing head beside a failing one in
    a pack of two or three), the blocks of pool(n / 2) as chroma in turn; every fourth pack has all-zero chroma beside its
    luma.  (luma, chroma) lists of (name, block) as quant_inputs.pack_array takes them."""
    n = 1 << log2n
    lsrc, csrc = pool(n), pool(n // 2)
    n_packs = -(-len(lsrc) // nc)
    luma = [lsrc[i % len(lsrc)] for i in range(n_packs * nc)]
    zero = ("zero", np.zeros((n // 2, n // 2), np.int16))
    chroma = [zero if (i // (2 * nc)) % 4 == 3 else csrc[(3 * i) % len(csrc)] for i in range(n_packs * nc * 2)]
    return luma, chroma


def pair_plan(n):
    """Groups of two blocks for the two-block path of the one-block quantiser: every block of pool(n) beside another."""
    src = pool(n)
    return [(src[i], src[(i + 7) % len(src)]) for i in range(len(src))]
