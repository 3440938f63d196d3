"""The 4x4 passes of the leaf searches keep a block in registers (wrenc_amd/csrc/dev_transform.h fwd_dct4_reg /
inv_dct4_reg, dev_quant.h dequantize4_lane): four blocks per wavefront, one sample per lane, the two stages of a transform
exchanging their operands by DPP (quad_perm broadcasts, row_ror:4/8/12).

  * The two test entries against the oracle's transforms, bit for bit, at block counts that leave idle rows (1, 2, 3), fill
    one wavefront (4), spill one block into a second (5) and run many wavefronts with a partial last one (203).  An
    impulse at each of the 16 positions pins the whole lane mapping -- which lane feeds which, the basis element that goes
    with each rotated value, and thereby the direction row_ror rotates; the constant and sign-pattern blocks give the
    largest intermediates; levels up to +-32767 at QP 18, 32 and 51 make both clamps to 16 bits fire (after the
    dequantiser and after the inverse transform's first stage).
  * One end-to-end case: small pictures whose CTUs split down to 4x4 at max-split-depth 3, wave schedule and team
    schedule, every plane of the record and the f32 CTU costs against the oracle, and the final pass (which re-makes
    every 4x4 CU with the LDS transforms) agreeing with the search's reconstruction."""
import numpy as np
import pytest

from content import content

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 4, 5, 203)
QPS = (18, 32, 51)
T4 = np.array([[64, 64, 64, 64], [83, 36, -36, -83], [64, -64, -64, 64], [36, -83, 83, -36]], np.int64)
KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr",
        "ctu_cost")


@pytest.fixture(scope="module")
def enc_at(built):
    from wrenc_amd import gpu
    made = {}

    def get(qp):
        if qp not in made:
            made[qp] = gpu.Encoder(64, 64, qp=qp, max_split_depth=0)
        return made[qp]
    yield get
    for e in made.values():
        e.close()


def _patterns(a):
    """Impulses of +-a at each position, the two constant blocks, row / column / checkerboard signs: 37 blocks."""
    out = []
    for p in range(16):
        for s in (a, -a):
            b = np.zeros(16, np.int64)
            b[p] = s
            out.append(b.reshape(4, 4))
    yy, xx = np.indices((4, 4))
    out += [np.full((4, 4), a), np.full((4, 4), -a)]
    out += [np.where(m & 1, -a, a) for m in (yy, xx, yy + xx)]
    return out


def _take(blocks, count):
    """`count` blocks: the fixed ones first, cycled where the count asks for more."""
    return np.stack([blocks[i % len(blocks)] for i in range(count)]).astype(np.int16)


_fwd_cases = {}


def _fwd_case(count):
    """(residual blocks, the oracle's coefficients), made once per count."""
    if count not in _fwd_cases:
        from oracle import pyoracle as po
        rng = np.random.default_rng(700 + count)
        fixed = _patterns(255)
        # a small count cannot hold every pattern: rotate through them so that 1..5 together still start at different ones
        start = {1: 0, 2: 5, 3: 30, 4: 32, 5: 34}.get(count, 0)
        fixed = fixed[start:] + fixed[:start]
        blocks = _take(fixed, count)
        if count > len(fixed):
            blocks[len(fixed):] = rng.integers(-255, 256, (count - len(fixed), 4, 4))
        _fwd_cases[count] = (blocks, np.stack([po.fwd_dct(b) for b in blocks]))
    return _fwd_cases[count]


@pytest.mark.parametrize("count", COUNTS)
def test_forward_equals_the_oracle(enc_at, count):
    blocks, want = _fwd_case(count)
    got = enc_at(32).fwd_dct4_reg(blocks)
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), "count %d: %d coefficients differ, first at (block, v, x) %s" % (count, len(bad), bad[0])


def _level_blocks(rng):
    """203 blocks of levels: impulses of both signs at three sizes and the constant / sign-pattern blocks (111 fixed
    blocks), then random levels, small and over the whole 16-bit range in turn."""
    fixed = _patterns(32767) + _patterns(1) + _patterns(40)
    blocks = _take(fixed, 203)
    n = 203 - len(fixed)
    wide = rng.integers(-32768, 32768, (n, 4, 4))
    small = rng.integers(-60, 61, (n, 4, 4))
    blocks[len(fixed):] = np.where((np.arange(n) % 2 == 0)[:, None, None], small, wide)
    return blocks, len(fixed)


@pytest.mark.parametrize("qp", QPS)
def test_inverse_equals_the_oracle(enc_at, qp):
    from oracle import pyoracle as po
    rng = np.random.default_rng(800 + qp)
    e = enc_at(qp)
    clamp_deq = clamp_v = False
    every, n_fixed = _level_blocks(rng)
    for count in COUNTS:
        # 203 holds every block; the small counts start at different fixed ones
        blocks = every if count == 203 else np.roll(every[:n_fixed], -17 * count, axis=0)[:count]
        deq = [po.dequantize(b, qp) for b in blocks]
        want = np.stack([po.inv_dct(d) for d in deq])
        got = e.inv_dct4_reg(blocks)
        bad = np.argwhere(got != want)
        assert np.array_equal(got, want), "QP %d count %d: %d residuals differ, first at (block, y, x) %s" % (qp, count, len(bad), bad[0])
        for d in deq:
            if d.max() == 32767 or d.min() == -32768:  # the dequantiser's clamp
                clamp_deq = True
            v = (T4.T @ d.astype(np.int64) + 64) >> 7   # the first stage before its clamp
            if v.max() > 32767 or v.min() < -32768:
                clamp_v = True
    assert clamp_deq and clamp_v, "the inputs must reach both clamps (dequantiser %s, first stage %s)" % (clamp_deq, clamp_v)


def _frame(kind, w, h):
    from wrenc_amd import synth
    return synth.synth_textured_frame(w, h, 0) if kind == "textured" else content(kind, w, h, 60)


@pytest.mark.parametrize("w,h", ((64, 64), (96, 64)))
def test_records_equal_the_oracle(built, w, h):
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    cases = [(kind, qp) for kind in ("textured", "noise") for qp in (22, 32, 51)]
    frames = {kind: _frame(kind, w, h) for kind in ("textured", "noise")}
    refs = [po.encode_picture(*frames[kind], qp, 3) for kind, qp in cases]
    assert any((r["cu_log2_size"] == 2).any() for r in refs), "no CU of the inputs is split down to 4x4"
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=3, n_slots=len(cases), schedule=gpu.Encoder.SCHEDULE_WAVE)
    for s, (kind, qp) in enumerate(cases):
        enc.upload(s, *frames[kind])
        enc.set_qp(s, qp)
    for schedule, ran in ((gpu.Encoder.SCHEDULE_WAVE, 1), (gpu.Encoder.SCHEDULE_TEAM, 2)):
        enc.set_schedule(schedule)
        enc.encode(0, len(cases))
        enc.sync()
        assert enc.last_schedule() == ran
        assert enc.final_pass_mismatches() == 0
        for s, (kind, qp) in enumerate(cases):
            got = enc.download(s)
            for k in KEYS:
                if not np.array_equal(got[k], refs[s][k]):
                    bad = np.argwhere(got[k] != refs[s][k])
                    raise AssertionError("%s %dx%d QP %d schedule %d: %s differs at %d positions, first %s"
                                         % (kind, w, h, qp, schedule, k, len(bad), bad[0]))
    enc.close()
