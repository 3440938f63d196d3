"""The 8x8 and 16x16 transforms of the leaf packs as i8 MFMAs (wrenc_amd/csrc/dev_transform.h fwd_dct_mfma /
inv_dct_mfma; the search runs them at 16x16) and the v_dot2 templates (the search's 8x8), on the inputs of
tests/test_dct_mfma_model.py dealt into groups whose blocks are all different: both arms equal the oracle block by block, the one-block entry and each
other, bit for bit.  The impulse blocks pin the operand-to-lane mapping (a transposed or rotated layout moves every
off-diagonal value); a neighbour that leaks into a block shows because no two blocks of a group are alike."""
import numpy as np
import pytest

import dct_mfma_model as mm

pytestmark = pytest.mark.gpu

# (log2n, nb, o1): what the search hands over (a pack's luma at 0, its chroma behind it) and one-off neighbours
SHAPES = [(3, 1, 0), (3, 2, 0), (3, 3, 0), (3, 4, 0), (3, 2, 256), (3, 4, 512), (4, 1, 0), (4, 2, 0), (4, 4, 0)]


@pytest.fixture(scope="module")
def enc(built):
    from wrenc_amd import gpu
    e = gpu.Encoder(64, 64, qp=32, max_split_depth=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(enc):
    """per (direction, n): the blocks, the oracle's answers and the one-block entry's answers, computed once"""
    from oracle import pyoracle as po
    out = {}
    for n in (8, 16):
        for direction, inputs, oracle, solo in (("fwd", mm.fwd_inputs(n), po.fwd_dct, enc.fwd_dct),
                                                ("inv", mm.inv_inputs(n), po.inv_dct, enc.inv_dct)):
            blocks = np.stack(list(inputs.values()))
            want = np.stack([oracle(b) for b in blocks])
            out[direction, n] = (list(inputs), blocks, want, solo(blocks))
    for v in out.values():
        for a in v[1:]:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("direction", ["fwd", "inv"])
@pytest.mark.parametrize("log2n,nb,o1", SHAPES)
def test_groups_equal_the_oracle_on_both_arms(enc, cases, direction, log2n, nb, o1):
    n = 1 << log2n
    names, blocks, want, solo = cases[direction, n]
    assert np.array_equal(solo, want), "the one-block entry against the oracle"
    groups = mm.as_groups(blocks, nb)
    want_g = mm.as_groups(want, nb)
    assert groups.shape == (len(names), nb, n, n)
    for g in groups[:: max(len(groups) // 16, 1)]:          # (the dealing itself: no group holds a block twice)
        assert len({b.tobytes() for b in g}) == nb
    fn = enc.fwd_dct_groups_arm if direction == "fwd" else enc.inv_dct_groups_arm
    got = {}
    for use_mfma in (1, 0):
        got[use_mfma], ms = fn(groups, use_mfma, o1)
        assert ms > 0
        bad = np.argwhere((got[use_mfma] != want_g).any(axis=(2, 3)))
        assert bad.size == 0, "use_mfma=%d: %d blocks differ from the oracle, first group %d block %d (%s)" % (
            use_mfma, len(bad), bad[0][0], bad[0][1], names[(bad[0][0] + bad[0][1] * max(len(names) // nb, 1)) % len(names)])
    assert np.array_equal(got[0], got[1])
    # the plain group entry runs what the search runs at this size: the same answer
    plain = (enc.fwd_dct_groups if direction == "fwd" else enc.inv_dct_groups)(groups, o1)
    assert np.array_equal(plain, want_g)
    # ... and the one-block entry's, block by block
    assert np.array_equal(got[1], mm.as_groups(solo, nb))


@pytest.mark.parametrize("n", [8, 16])
def test_a_residual_of_256_takes_the_v_dot2_arm_and_the_context_stays_usable(enc, cases, n):
    """The digit scheme is exact within +-255, which is all the search forms.  The plain entries inspect the input on the
    host: a group with a residual outside runs the v_dot2 templates (at 16x16, where the search runs the MFMA version, a
    choice the host makes; at 8x8 what the search runs anyway) and returns the oracle's coefficients; asked for the MFMA
    arm by name, the entry refuses it before anything is launched, and the next call is served."""
    from wrenc_amd import gpu
    from oracle import pyoracle as po
    _, blocks, want, _ = cases["fwd", n]
    group = np.stack([blocks[0], blocks[5], blocks[-1]])[None].copy()
    group[0, 1, 2, 3] = 256
    ref = np.stack([po.fwd_dct(b) for b in group[0]])
    assert np.array_equal(enc.fwd_dct_groups(group)[0], ref)
    assert np.array_equal(enc.fwd_dct(group[0])[1], ref[1])
    with pytest.raises(gpu.WrencGpuError) as e:
        enc.fwd_dct_groups_arm(group, 1)
    assert e.value.code == -1          # WRENC_GPU_EINVAL
    got, _ = enc.fwd_dct_groups_arm(group, 0)
    assert np.array_equal(got[0], ref)
    # an o1 the 16-byte row reads cannot take: the host picks the v_dot2 arm as well
    assert np.array_equal(enc.fwd_dct_groups(blocks[None, :2], 2)[0], want[:2])
    # the context after the refusal: the MFMA arm on a clean group, and a whole picture
    got, _ = enc.fwd_dct_groups_arm(blocks[None, :3], 1)
    assert np.array_equal(got[0], want[:3])
    from wrenc_amd import synth
    y, cb, cr = synth.synth_textured_frame(64, 64, 0)
    rec = enc.encode_picture(y, cb, cr)
    assert enc.final_pass_mismatches() == 0
    ref_pic = po.encode_picture(y, cb, cr, 32, 0)
    for k in ("rec_y", "lev_y", "lev_cb", "lev_cr"):
        assert np.array_equal(rec[k], ref_pic[k]), k
