"""Coefficient blocks for the quantiser parity tests (test_quant_inputs.py on the CPU, test_gpu_quant_bounds.py on the device).

Everything here is derived from the reference's quantiser formulas, never from device code:

    level scale  lsc = 16 * LEVEL_SCALE[(qp + 1) % 6] << ((qp + 1) / 6)          (quantizer.rs:8, LEVEL_SCALE from
                                                                                  tests/golden/ref_source_data.json)
    shift        sh  = log2(n) + 4,  offset off = 1 << (sh - 1)                  (quantizer.rs:558-569)
    quotient     qd  = |(tc << sh) - off| / lsc                                  (quantizer.rs:378, :441)
    trellis level a  = qd / 2 or (qd + 1) / 2 by the state's delta, or one more; coded level q = 2 a - delta

"Level" below is the trellis level a, the index of the level-cost table (block_splitter.rs:436-458); the search costs
both candidates of a position with dq_table[a + 1] (quantizer.rs:29-31), so the reference panics once a0 + 2 >= 1024
for a candidate it visits.  The largest quotient that is safe in every state is therefore 2042 (a0 = 1021 in both
delta classes, the tables' last entry 1023 consulted), and 2044 panics in every state.  At 2043 the reference panics
only where its search reaches the position in a state with delta 1 (a lone coefficient is reached in state 0 alone);
the device costs both delta classes at every position and reports the overflow there regardless, one quotient step
early (include/wrenc_gpu.h), so no generator but early_blocks -- which holds exactly that difference -- sends a quotient
of 2043: negative maxima are computed for their own sign (the offset enters a negative coefficient's quotient with the
other sign).  The DC position is exempt on both sides: its a0 is qd / 2 in either delta class.

A coefficient is 16 bits, so the largest level a block can hold at all is reach(qp, n) = quotient(32767) / 2: 1023 and
more only at low QPs (4x4: QP <= 3, 32x32: QP <= 21), 7 at QP 63 and 32x32, 0 at QP 63 and 4x4.  Classes that name a
level range are required where reach allows them (required_classes) -- the class "maximal" (d) everywhere, as the
largest magnitude there is: +-32767 / -32768, or the largest magnitude of quotient 2042 where those would panic.
"""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_TABLES = json.load(open(os.path.join(_HERE, "golden", "ref_source_data.json")))["tables"]
LEVEL_SCALE = [int(v) for v in np.ravel(_TABLES["level_scale"])]
Q_STATE_TRANS = [[int(v) for v in row] for row in np.reshape(_TABLES["q_state_trans"], (4, 2))]

SIZES = (4, 8, 16, 32)
PACKS = ((3, 1), (3, 2), (3, 3), (4, 1), (4, 2))   # (log2 of the luma side, candidates) quantize_pk takes
TOP_QUOTIENT = 2042                                 # the largest quotient no state panics at (module docstring)
OVER_QUOTIENT = 2044                                # the smallest quotient every state panics at


def level_scale(qp):
    return (16 * LEVEL_SCALE[(qp + 1) % 6]) << ((qp + 1) // 6)


def shift(n):
    return n.bit_length() - 1 + 4


def reciprocal(qp):
    """(lsc, m, k - 32): the level scale of a QP and the reciprocal the device divides by it with (DevConst::lsc, div_magic,
    div_shift; const_block.cpp, fill_dev_const): m = floor(2^k / lsc) + 1, k = 26 + ceil(log2 lsc), q = mulhi(n, m) >> (k - 32)."""
    lsc = level_scale(qp)
    lg = 0
    while (1 << lg) < lsc:
        lg += 1
    k = 26 + lg
    return lsc, (1 << k) // lsc + 1, k - 32


def quotient(tc, qp, n):
    sh = shift(n)
    s = (int(tc) << sh) - (1 << (sh - 1))
    return 0 if tc == 0 else (-s if tc < 0 else s) // level_scale(qp)


def coef_below(qd, qp, n, neg=False):
    """The largest magnitude whose quotient is <= qd (as a negative coefficient with neg), within 16 bits."""
    sh, off = shift(n), 1 << (shift(n) - 1)
    m = ((qd + 1) * level_scale(qp) - 1 + (-off if neg else off)) >> sh
    return max(0, min(m, 32768 if neg else 32767))


def reach(qp, n):
    """The largest level a 16-bit coefficient is sure to reach at this QP and block size."""
    return quotient(32767, qp, n) // 2


def top_coef(qp, n, neg=False):
    """The maximum magnitude of class (d): 32767 / 32768, or the largest the reference does not panic at."""
    return coef_below(TOP_QUOTIENT, qp, n, neg)


def coef_for_level(k, qp, n, neg=False):
    """A magnitude whose level is k - 1 .. k + 1 (k or k + 1 wherever one coefficient unit is at most one quotient)."""
    return coef_below(2 * k, qp, n, neg)


def _diag(side):
    return [(d - x, x) for d in range(2 * side - 1) for x in range(d + 1) if x < side and d - x < side]


def scan(n):
    """(y, x) of every position in coding order (ctu.rs:14-81, :827-845): 4x4 sub-blocks along up-right diagonals, the
    same inside each; the quantiser walks it backwards."""
    return [(4 * sy + y, 4 * sx + x) for sy, sx in _diag(n // 4) for y, x in _diag(4)]


def trellis_levels(levels):
    """The level a of every position of a block of coded levels (block_splitter.rs:436-458)."""
    n = levels.shape[0]
    out = np.zeros((n, n), np.int64)
    state = 0
    for y, x in reversed(scan(n)):
        qc = abs(int(levels[y, x]))
        a = (qc + (1 if state > 1 else 0)) // 2 if qc else 0
        out[y, x] = a
        state = Q_STATE_TRANS[state][a & 1]
    return out


def level_cost_model(levels, lv):
    """block_splitter.rs:415-460 from trellis_levels and the level-cost table lv: what ties them to the oracle's walk."""
    a = trellis_levels(levels)
    total, trailing = 0, True
    for y, x in reversed(scan(levels.shape[0])):
        if levels[y, x] != 0:
            total += int(lv[a[y, x]])
            trailing = False
        elif not trailing:
            total += int(lv[0])
    return total


# ---- classes, named by the oracle's output ----
def required_classes(qp, n):
    r = reach(qp, n)
    need = ["a", "d", "e"]
    if r >= 2:
        need += ["b_sparse", "b_dense"]
    if r >= 258:
        need.append("c")
    return need


def classes_of(coef, ref, qp):
    """The classes (a) .. (d) a block belongs to, from its coefficients and the oracle's levels."""
    n = coef.shape[0]
    a = trellis_levels(ref)
    nnz = int((a > 0).sum())
    mag = np.abs(coef.astype(np.int32))
    out = set()
    if nnz == 0 and mag.any():
        out.add("a")
    if nnz and a.max() <= 8:
        if nnz <= n * n // 8:
            out.add("b_sparse")
        if nnz >= n * n // 2:
            out.add("b_dense")
    if ((a >= 200) & (a <= 255)).any() and ((a >= 256) & (a <= 400)).any():
        out.add("c")
    if mag.max() >= top_coef(qp, n) and min(900, reach(qp, n)) <= a.max() <= 1023:
        out.add("d")
    return out


def missing_classes(qp, n, tagged, refs):
    """Required classes that no block of `tagged` ((tag, block) pairs, refs = the oracle's levels) is in; (e) is the
    generator's tag, the others are read off the oracle's output."""
    seen = set()
    for (tag, b), ref in zip(tagged, refs):
        seen |= classes_of(b, ref, qp)
        if tag == "e":
            seen.add("e")
    return [c for c in required_classes(qp, n) if c not in seen]


def class_counts(qp, tagged, refs, into):
    for (tag, b), ref in zip(tagged, refs):
        for c in classes_of(b, ref, qp) | ({"e"} if tag == "e" else set()):
            into[c] = into.get(c, 0) + 1
    return into


# ---- blocks of every class at one QP ----
CLASS_SEEDS = 3   # blocks per class (a) .. (d) and sets of four decaying spectra, each from its own draw
def _signs(rng, shape):
    return rng.integers(0, 2, shape) * 2 - 1


def _decaying(rng, n, sigma, top):
    decay = np.exp(-np.add.outer(np.arange(n), np.arange(n)) / (n / 3.0))
    return (rng.standard_normal((n, n)) * sigma * decay).clip(-top, top).astype(np.int16)   # (top: safe with either sign)


def qp_blocks(qp, n, seeds=CLASS_SEEDS):
    """(tag, block) pairs holding every class required_classes(qp, n) names, `seeds` independent draws of each; the tag is
    the class the block was built for (the tests read the classes off the oracle's output, not off the tag -- except (e),
    the decaying spectra)."""
    rng = np.random.default_rng(7000 + 100 * qp + n)
    N, r, top = n * n, reach(qp, n), top_coef(qp, n)
    both = min(top, top_coef(qp, n, neg=True))
    unit = 2.0 * level_scale(qp) / (1 << shift(n))       # coefficient units per level
    out = []

    def put(b, k, lo, hi):
        for at in rng.choice(N, k, replace=False):
            neg = bool(rng.integers(0, 2))
            v = coef_for_level(int(rng.integers(lo, hi + 1)), qp, n, neg)
            b[at // n, at % n] = -v if neg else v

    for seed in range(seeds):
        b = np.zeros((n, n), np.int16)                   # (a): a sixth of a level at three places
        for at in rng.choice(N, 3, replace=False):
            b[at // n, at % n] = max(1, coef_below(0, qp, n) // 3) * int(_signs(rng, ()))
        out.append(("a", b))
        if r >= 2:
            hi = min(7, r)
            b = np.zeros((n, n), np.int16)
            put(b, max(2, N // 16), 2, hi)
            out.append(("b_sparse", b))
            b = np.zeros((n, n), np.int16)
            put(b, N, 2, min(4, hi))
            out.append(("b_dense", b))
        if r >= 258:
            b = _decaying(rng, n, 2 * unit, both)
            put(b, 3, 202, 254)
            put(b, 3, 258, min(398, r - 1))
            out.append(("c", b))
        b = (rng.integers(-1, 2, (n, n)) * (unit / 2)).astype(np.int16)    # (d): the maximum, both signs, over half-level noise
        ats = rng.choice(N, 3, replace=False)
        b[ats[0] // n, ats[0] % n] = top
        b[ats[1] // n, ats[1] % n] = -top_coef(qp, n, neg=True)
        corner = [0, n - 1][(qp + seed) & 1]             # the DC or the walk's first position, in turn
        b[corner, corner] = top if rng.integers(0, 2) else -top_coef(qp, n, neg=True)
        out.append(("d", b))
        for sigma in (0.5, 3.0, 20.0, 150.0):            # (e): the decaying spectra of test_gpu_blocks.py, in levels
            out.append(("e", _decaying(rng, n, sigma * unit, both)))
    return out


def pack_plan(qp, log2n, nc):
    """Packs of quantize_pk at one QP: every luma block of qp_blocks(qp, n) once, the chroma blocks of qp_blocks(qp, n / 2)
    in turn.  Returns (luma, chroma) lists of (tag, block): pack p holds luma[p * nc + c] and chroma[(p * nc + c) * 2 + pl]."""
    n = 1 << log2n
    lsrc, csrc = qp_blocks(qp, n), qp_blocks(qp, n // 2)
    n_packs = -(-len(lsrc) // nc)
    luma = [lsrc[i % len(lsrc)] for i in range(n_packs * nc)]
    chroma = [csrc[i % len(csrc)] for i in range(n_packs * nc * 2)]
    return luma, chroma


def pack_array(luma, chroma, nc):
    """The (n_packs, nc * 1.5 * n * n) array quantize_pk takes: per pack nc luma blocks, then per candidate Cb and Cr."""
    n_packs = len(luma) // nc
    return np.stack([np.concatenate([b.ravel() for b in luma[p * nc:(p + 1) * nc] + chroma[p * 2 * nc:(p + 1) * 2 * nc]])
                     for p in range(n_packs)])


# ---- blocks built against the stated bounds ----
# (qp, extra_params): the ends of the QP range (the step-cost bound is stated for QP 63), the two rate models at the edge
# of what wrenc_gpu_create accepts, and three QPs at which the maximum magnitude really is a level of 900 and more, which
# no 16-bit coefficient is at QP 57 or 63 -- QP 22: +-32767 themselves at 32x32; QP 16: 16x16 and 32x32; QP 4: every
# size, so that the 4x4 blocks of quantize_p16 and the 8x8 / 4x4 members of the quantize_pk packs sit at the tables' end
BOUND_MODELS = ((63, None), (57, None), (32, "quant_lambda_mul_trellis=86"), (37, "quant_lambda_mul_trellis=44"),
                (22, None), (16, None), (4, None))


def bound_blocks(qp, n):
    """(name, block): every position at the maximum magnitude; the same with alternating signs; checkerboards of the maximum
    against 0 and against +-1; 16 maximal positions in scan order before zeros and 16 zeros before maximal positions, at
    either end of the scan; a lone maximum at the first and at the last scan position."""
    top, topn = top_coef(qp, n), top_coef(qp, n, neg=True)
    order = scan(n)
    yy, xx = np.indices((n, n))
    odd = ((yy + xx) & 1).astype(bool)
    out = [("all_max", np.full((n, n), top, np.int16)),
           ("alternating_signs", np.where(odd, -topn, top).astype(np.int16)),
           ("checker_max_0", np.where(odd, 0, top).astype(np.int16)),
           ("checker_max_pm1", np.where(odd, np.where(yy & 1, 1, -1), np.where(xx & 2, -topn, top)).astype(np.int16))]

    def along(first, rest, count):
        b = np.full((n, n), rest, np.int16)
        for y, x in order[:count] if count > 0 else order[count:]:
            b[y, x] = first
        return b
    if n > 4:   # 16 positions are one sub-block and one period of the walk's renormalisation
        out += [("first16_max", along(top, 0, 16)), ("first16_zero", along(0, top, 16)),
                ("last16_max", along(-topn, 0, -16)), ("last16_zero", along(0, -topn, -16))]
    out += [("lone_first", along(top, 0, 1)), ("lone_last", along(-topn, 0, -1))]
    return out


def bound_level_floor(qp, n):
    """What the largest level of a bound block must reach: 900, or all that 16 bits give at this QP and size."""
    return min(900, reach(qp, n))


def noise3(n, seed):
    return np.random.default_rng(seed).integers(-3, 4, (n, n)).astype(np.int16)


# ---- the DC wrap ----
WRAP_QPS = (22, 32, 45)
WRAP_COUNT = 36
WRAP_SEED = 9400   # chosen on the CPU: at least four wraps per size and QP in the oracle's output


def dc_wrap_blocks(qp, n):
    """Sparse blocks with a small DC and one to three coefficients of level 1 or 2 elsewhere: where the walk arrives at the
    DC position in a state with delta 1 and keeps a = 0 there, the reference's usize wrap codes the level -1 * sign
    (quantizer.rs:378-391).  That costs the distortion of a whole level more than level 1 of the right sign and saves
    lambda_q * (dq_table[2] - dq_table[1]), so it wins only for a DC of a few hundredths of a quotient step: the DC is
    drawn from 1 .. 1/32 of a step.  The seed is fixed so that the oracle alone shows at least one such block per size."""
    rng = np.random.default_rng(WRAP_SEED + 10 * qp + n)
    out = []
    for _ in range(WRAP_COUNT):
        b = np.zeros((n, n), np.int16)
        b[0, 0] = int(rng.integers(1, max(1, coef_below(1, qp, n) // 32) + 1)) * int(_signs(rng, ()))
        for at in rng.choice(np.arange(1, n * n), int(rng.integers(1, 4)), replace=False):
            neg = bool(rng.integers(0, 2))
            v = coef_for_level(int(rng.integers(1, 3)), qp, n, neg)
            b[at // n, at % n] = -v if neg else v
        out.append(b)
    return out


def dc_wrapped(coef, ref):
    return coef[0, 0] != 0 and ref[0, 0] != 0 and (coef[0, 0] < 0) != (ref[0, 0] < 0)


# ---- the level limit ----
def limit_qps(n):
    """The two largest QPs at which a 16-bit coefficient of a block of side n passes the tables' end (they are
    neighbours, so of different (qp + 1) % 6 classes)."""
    ok = [qp for qp in range(64) if coef_below(OVER_QUOTIENT - 1, qp, n) < 32767]
    return ok[-2], ok[-1]


def limit_block(qp, n, seed, over):
    """An ordinary block (levels 0 .. 2) with one coefficient at the last table entry (quotient 2042: dq_table[1023] is
    consulted, nothing beyond), or with `over` one step beyond it (quotient 2044: every state asks for dq_table[1024])."""
    rng = np.random.default_rng(seed)
    unit = 2.0 * level_scale(qp) / (1 << shift(n))
    b = (rng.integers(-2, 3, (n, n)) * unit).astype(np.int16)
    at = int(rng.integers(0, n * n))
    neg = bool(seed & 1)
    v = coef_below(OVER_QUOTIENT - 1, qp, n, neg) + 1 if over else coef_below(TOP_QUOTIENT, qp, n, neg)
    b[at // n, at % n] = -v if neg else v
    return b


def harmless_block(qp, n, seed=1):
    rng = np.random.default_rng(9900 + seed)
    return _decaying(rng, n, 3.0 * 2.0 * level_scale(qp) / (1 << shift(n)), top_coef(qp, n, neg=True) - 1)


def early_blocks(qp, n):
    """(name, block, oracle quantises, device quantises): the quotient between TOP_QUOTIENT and OVER_QUOTIENT, 2043, where
    the reference's answer depends on the states its search visits and the device's does not (include/wrenc_gpu.h).
    Alone at the walk's first position -- the last in scan order, reached in state 0 only -- the reference quantises and
    the device reports the overflow, one step early; in every position of a block the reference panics too; at the DC
    position, beside small coefficients that bring the walk there in every state, both quantise (a0 = qd / 2 in either
    delta class)."""
    v = coef_below(OVER_QUOTIENT - 1, qp, n)
    assert quotient(v, qp, n) == OVER_QUOTIENT - 1
    lone = np.zeros((n, n), np.int16)
    lone[n - 1, n - 1] = v
    dc = harmless_block(qp, n, 2)
    dc[0, 0] = v
    return [("lone_first_walked", lone, True, False), ("everywhere", np.full((n, n), v, np.int16), False, False),
            ("dc_beside_others", dc, True, True)]
