"""The quantiser kernels (wrenc_amd/csrc/dev_quant.h) against the oracle's literal DFS at every QP and at the ends of the
32-bit cost range: every entry point, blocks of every class the 16-bit coefficient range allows at that QP
(tests/quant_inputs.py), the DC position's usize wrap, and the level limit with the test entries' own overflow word.
Nothing expected here comes from device code; test_quant_inputs.py holds the generators against the oracle on the CPU."""
import numpy as np
import pytest

import quant_inputs as qi

pytestmark = pytest.mark.gpu

ELEVEL = -6   # WRENC_GPU_ELEVEL


class _Oracle:
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


def _check_solo(e, oracle, blocks, what, packed=False):
    """quantize (or quantize_p16) and dequantize of a list of equal-sized blocks; returns the blocks compared."""
    arr = np.stack(blocks)
    got, cost = e.quantize_p16(arr) if packed else e.quantize(arr)
    deq = e.dequantize(got)
    for i, b in enumerate(blocks):
        ref, ref_cost, ref_deq = oracle(b)
        assert np.array_equal(got[i], ref), (what, i)
        assert int(cost[i]) == ref_cost, (what, i)
        assert np.array_equal(deq[i], ref_deq), (what, i)
    return len(blocks)


def _check_packs(e, oracle, luma, chroma, log2n, nc, what):
    """quantize_pk of packs holding luma[p * nc + c] and chroma[(p * nc + c) * 2 + pl]; returns the blocks compared."""
    n, nch = 1 << log2n, 1 << (log2n - 1)
    levels, cost = e.quantize_pk(qi.pack_array(luma, chroma, nc), log2n, nc)
    for p in range(len(luma) // nc):
        at = 0
        for c in range(nc):
            ref, ref_cost, ref_deq = oracle(luma[p * nc + c])
            got = levels[p, at:at + n * n].reshape(n, n)
            assert np.array_equal(got, ref), (what, p, c, "luma")
            assert int(cost[p, c, 0]) == ref_cost, (what, p, c, "luma cost")
            at += n * n
        pair = []
        for c in range(nc):
            want = 0
            for pl in range(2):
                ref, ref_cost, ref_deq = oracle(chroma[(p * nc + c) * 2 + pl])
                got = levels[p, at:at + nch * nch].reshape(nch, nch)
                assert np.array_equal(got, ref), (what, p, c, pl)
                pair.append((got, ref_deq))
                want += ref_cost
                at += nch * nch
            assert int(cost[p, c, 1]) == want, (what, p, c, "chroma cost")
        deq = e.dequantize(np.stack([g for g, _ in pair]))
        for i, (_, ref_deq) in enumerate(pair):
            assert np.array_equal(deq[i], ref_deq), (what, p, i, "chroma dequantised")
    return 3 * len(luma)


@pytest.mark.parametrize("qp", range(64))
def test_every_entry_point_at_every_qp(built, qp):
    """quantize at 4 .. 32, quantize_p16 and the five quantize_pk shapes at one QP: levels, level cost and the
    dequantised levels of every block equal the oracle's, over blocks that quantise to nothing, to levels 1 .. 8 sparse
    and dense, to levels on both sides of the LDS tables' 256 entries, to the largest level there is, and over decaying
    spectra -- each class wherever 16-bit coefficients reach it at that QP and size (quant_inputs.required_classes), which
    this test asserts of what it sent."""
    from wrenc_amd import gpu
    oracle = _Oracle(qp)
    counts, compared = {}, 0
    e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
    try:
        for n in qi.SIZES:
            tagged = qi.qp_blocks(qp, n)
            refs = [oracle(b)[0] for _, b in tagged]
            assert qi.missing_classes(qp, n, tagged, refs) == [], (qp, n)
            qi.class_counts(qp, tagged, refs, counts)
            compared += _check_solo(e, oracle, [b for _, b in tagged], (qp, n))
        four = [b for _, b in qi.qp_blocks(qp, 4)]
        compared += _check_solo(e, oracle, four + four[::-1][1:], (qp, "p16"), packed=True)   # an odd count: a partial last group
        for log2n, nc in qi.PACKS:
            luma, chroma = qi.pack_plan(qp, log2n, nc)
            for side, part in ((1 << log2n, luma), (1 << (log2n - 1), chroma)):
                assert qi.missing_classes(qp, side, part, [oracle(b)[0] for _, b in part]) == [], (qp, log2n, nc, side)
            compared += _check_packs(e, oracle, [b for _, b in luma], [b for _, b in chroma], log2n, nc, (qp, log2n, nc))
    finally:
        e.close()
    print("qp %d: %d blocks compared, classes %s" % (qp, compared, sorted(counts.items())))


@pytest.mark.parametrize("qp,extra", qi.BOUND_MODELS)
def test_blocks_built_against_the_stated_bounds(built, qp, extra):
    """Blocks of nothing but the maximum magnitude and its relatives (alternating signs, checkerboards with 0 and
    +-1 -- the no-branch cost next to maximal step costs --, 16 maximal positions before or behind zeros at either end of
    the scan -- one period of the renormalisation --, a lone maximum at either end) at both ends of the QP range, under the
    two rate models at the edge of what wrenc_gpu_create accepts (lambda_q * dq_table[1023] = 24.9 M and 24.75 M of the
    25.17 M a step may cost) and at three QPs where the maximum is a level of 900 and more (QP 22 at 32x32, QP 16 from
    16x16, QP 4 at every size, the 4x4 blocks of quantize_p16 and every member of a quantize_pk pack included): 16x16
    and 32x32 through quantize, 4x4 through quantize_p16, and in quantize_pk packs beside all-zero and +-3 noise
    candidates.  Every block holds a level of at least quant_inputs.bound_level_floor: 900, or all that 16 bits give."""
    from wrenc_amd import gpu
    oracle = _Oracle(qp)
    oracle.po.set_extra_params(extra)
    e = None
    compared, top_levels = 0, {}
    try:
        e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0, extra_params=extra)
        named = {n: qi.bound_blocks(qp, n) for n in qi.SIZES}
        for n in qi.SIZES:
            for name, b in named[n]:
                a = int(qi.trellis_levels(oracle(b)[0]).max())
                assert qi.bound_level_floor(qp, n) <= a <= 1023, (qp, extra, n, name, a)
                top_levels[n] = min(top_levels.get(n, a), a)
        for n in (16, 32):
            compared += _check_solo(e, oracle, [b for _, b in named[n]], (qp, extra, n))
        compared += _check_solo(e, oracle, [b for _, b in named[4]], (qp, extra, "p16"), packed=True)
        for log2n in (3, 4):
            n, nch = 1 << log2n, 1 << (log2n - 1)
            big, bigc = [b for _, b in named[n]], [b for _, b in named[nch]]
            # every bound block as a candidate of its own, its chroma pair two bound blocks of half the side
            compared += _check_packs(e, oracle, big, [bigc[i % len(bigc)] for i in range(2 * len(big))], log2n, 1,
                                     (qp, extra, log2n, 1))
            # a maximal candidate beside an all-zero one and beside +-3 noise, in either place
            zero, zeroc = np.zeros((n, n), np.int16), np.zeros((nch, nch), np.int16)
            noise, noisec = qi.noise3(n, 1), [qi.noise3(nch, 2), qi.noise3(nch, 3)]
            luma, chroma = [], []
            for other, otherc in ((zero, [zeroc, zeroc]), (noise, noisec)):
                for k in (0, 1, 4):
                    mx, mxc = big[k], [bigc[k], bigc[(k + 1) % len(bigc)]]
                    luma += [mx, other, other, mx]
                    chroma += mxc + otherc + otherc + mxc
            compared += _check_packs(e, oracle, luma, chroma, log2n, 2, (qp, extra, log2n, 2))
            if log2n == 3:
                compared += _check_packs(e, oracle, [big[0], zero, noise, noise, big[1], zero],
                                         bigc[:2] + [zeroc, zeroc] + noisec + noisec + bigc[1:3] + [zeroc, zeroc], 3, 3,
                                         (qp, extra, 3, 3))
    finally:
        if e is not None:
            e.close()
        oracle.po.set_extra_params(None)
    print("qp %d %s: %d blocks compared, smallest top level per size %s" % (qp, extra, compared, sorted(top_levels.items())))


@pytest.mark.parametrize("qp", qi.WRAP_QPS)
def test_the_dc_wrap(built, qp):
    """The reference computes the DC position's level in usize and casts it to i16 (quantizer.rs:378-391): a = 0 in
    a state with delta 1 gives the level -1 * sign.  The oracle's output shows at least one such block per size among the
    blocks sent (asserted here from the oracle alone), and every block equals the oracle through every entry point."""
    from wrenc_amd import gpu
    oracle = _Oracle(qp)
    wraps, compared = {}, 0
    e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
    try:
        blocks = {n: qi.dc_wrap_blocks(qp, n) for n in qi.SIZES}
        for n in qi.SIZES:
            wraps[n] = sum(bool(qi.dc_wrapped(b, oracle(b)[0])) for b in blocks[n])
            assert wraps[n] >= 1, (qp, n)
            compared += _check_solo(e, oracle, blocks[n], (qp, n))
        compared += _check_solo(e, oracle, blocks[4], (qp, "p16"), packed=True)
        for log2n, nc in qi.PACKS:
            n_packs = qi.WRAP_COUNT // (2 * nc)
            compared += _check_packs(e, oracle, blocks[1 << log2n][:n_packs * nc], blocks[1 << (log2n - 1)][:n_packs * nc * 2],
                                     log2n, nc, (qp, log2n, nc))
    finally:
        e.close()
    print("qp %d: %d blocks compared, DC wraps per size %s" % (qp, compared, sorted(wraps.items())))


def _limit_cases():
    cases = [("quantize", n, 0) for n in qi.SIZES] + [("p16", 4, 0)]
    return cases + [("pk", log2n, nc) for log2n, nc in qi.PACKS]


@pytest.mark.parametrize("entry,size,nc", _limit_cases())
def test_the_level_limit(built, entry, size, nc):
    """A coefficient at the last table entry (the oracle consults dq_table[1023] and nothing beyond) compares equal;
    the same block with that coefficient one step larger makes the oracle raise and the entry return WRENC_GPU_ELEVEL --
    beside ordinary blocks in a quantize_p16 group of four and in a quantize_pk pack, as a luma and as a chroma block --;
    the next call on the same context succeeds and compares equal (include/wrenc_gpu.h: the test entries keep a word of
    their own and never poison a context).  At the two largest QPs at which 16 bits pass the limit at that size."""
    from wrenc_amd import gpu
    n = size if entry != "pk" else 1 << size
    sides = (n,) if entry != "pk" else (n, n // 2)      # the side whose block sits at the limit
    compared = 0
    for side in sides:
        for qp in qi.limit_qps(side):
            oracle = _Oracle(qp)
            po = oracle.po
            e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
            try:
                for seed in range(3):
                    at_limit, over = qi.limit_block(qp, side, seed, False), qi.limit_block(qp, side, seed, True)
                    po.quantize(at_limit, qp)
                    assert po.last_table_index() == 1023, (entry, side, qp, seed)
                    with pytest.raises(OverflowError):
                        po.quantize(over, qp)
                    if entry == "pk":
                        nch = n // 2
                        fill = [qi.harmless_block(qp, n, k) for k in range(nc)]
                        fillc = [qi.harmless_block(qp, nch, 10 + k) for k in range(2 * nc)]
                        c = seed % nc

                        def run(special):
                            luma, chroma = list(fill), list(fillc)
                            if side == n:
                                luma[c] = special
                            else:
                                chroma[2 * c + (seed & 1)] = special
                            return _check_packs(e, oracle, luma, chroma, size, nc, (entry, size, nc, side, qp, seed))
                        harmless = lambda: _check_packs(e, oracle, fill, fillc, size, nc, (entry, "after", qp, seed))
                    else:
                        fill = [qi.harmless_block(qp, n, k) for k in range(3)]

                        def run(special):
                            group = fill[:seed] + [special] + fill[seed:]
                            return _check_solo(e, oracle, group, (entry, side, qp, seed), packed=entry == "p16")
                        harmless = lambda: _check_solo(e, oracle, fill, (entry, "after", qp, seed), packed=entry == "p16")
                    compared += run(at_limit)
                    with pytest.raises(gpu.WrencGpuError) as err:
                        run(over)
                    assert err.value.code == ELEVEL, (entry, side, qp, seed, err.value)
                    compared += harmless()
            finally:
                e.close()
    print("%s %s %s: %d blocks compared" % (entry, size, nc, compared))


@pytest.mark.parametrize("n", qi.SIZES)
def test_the_quotient_below_the_limit(built, n):
    """The one known difference between the device and the reference (include/wrenc_gpu.h, WRENC_GPU_ELEVEL), held from
    both sides so that neither can move unseen: at a quotient of 2043 a coefficient alone at the walk's first position
    quantises in the oracle (its search reaches it in state 0 only) and returns WRENC_GPU_ELEVEL from the device, which
    costs both delta classes everywhere; in every position of a block the oracle raises as well; at the DC position,
    whose level is qd / 2 in either delta class, both quantise and agree.  Through quantize, and at 4x4 through
    quantize_p16 beside ordinary blocks; a harmless call follows every refusal."""
    from wrenc_amd import gpu
    compared = 0
    for qp in qi.limit_qps(n):
        oracle = _Oracle(qp)
        po = oracle.po
        fill = [qi.harmless_block(qp, n, k) for k in range(3)]
        e = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
        try:
            for name, b, oracle_ok, device_ok in qi.early_blocks(qp, n):
                if oracle_ok:
                    po.quantize(b, qp)
                    assert po.last_table_index() == 1023, (n, qp, name)
                else:
                    with pytest.raises(OverflowError):
                        po.quantize(b, qp)
                for packed in ((False, True) if n == 4 else (False,)):
                    group = [b] if not packed else fill[:1] + [b] + fill[1:]
                    if device_ok:
                        compared += _check_solo(e, oracle, group, (n, qp, name, packed), packed=packed)
                        continue
                    with pytest.raises(gpu.WrencGpuError) as err:
                        e.quantize_p16(np.stack(group)) if packed else e.quantize(np.stack(group))
                    assert err.value.code == ELEVEL, (n, qp, name, packed, err.value)
                    compared += _check_solo(e, oracle, fill, (n, qp, name, "after"), packed=packed)
        finally:
            e.close()
    print("%d: %d blocks compared" % (n, compared))
