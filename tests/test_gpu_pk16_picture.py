"""Records of a 64x64 picture (2x2 CTUs: every availability pattern, and the 32x32, 16x16, 8x8 and 4x4 paths at
max-split-depth 3) against the oracle, bit for bit in all ten planes, on the content that drives the packed 16-bit rows
(dev_pk16.h) to their range limits: 0 / 255 patches (clamps in prediction and reconstruction, residuals of +-255) and
noise (many levels, large reconstructed residuals), at QP 4, 32 and 51, both schedules.  At QP 4 both contents make the
reference panic (a level reaches 1024) and the device must report the same; noise at half contrast is added as the QP 4
picture whose records compare."""
import functools

import numpy as np
import pytest

from content import content as _content

pytestmark = pytest.mark.gpu

KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr", "rec_y", "rec_cb", "rec_cr",
        "ctu_cost")
W = H = 64
DEPTH = 3


ELEVEL = -6   # WRENC_GPU_ELEVEL


@functools.lru_cache(maxsize=None)
def _picture_and_reference(kind, qp):
    """The oracle's record: computed once, shared by the two schedules, never written to.  None where the oracle reports
    the reference's panic (a quantised level reached 1024, block_splitter.rs:453): at QP 4 full-contrast content does."""
    from oracle import pyoracle as po
    y, cb, cr = _content(kind.split("_")[0], W, H, 1600 + qp)
    if kind.endswith("_half"):      # half the contrast around 128: levels stay inside the reference's tables at QP 4
        y, cb, cr = (np.ascontiguousarray(128 + (a.astype(np.int32) - 128) // 2, np.uint8) for a in (y, cb, cr))
    try:
        ref = po.encode_picture(y, cb, cr, qp, DEPTH)
    except ValueError:
        ref = None
    for a in (y, cb, cr) + (tuple(ref[k] for k in KEYS) if ref else ()):
        a.setflags(write=False)
    return (y, cb, cr), ref


# 0 / 255 patches and noise at QP 4, 32 and 51.  At QP 4 both make the reference panic, and the device must say so too;
# noise at half contrast is the QP 4 picture whose records compare (levels up to 296).
@pytest.mark.parametrize("schedule", [1, 2])    # one wave per CTU / a team of four waves per CTU
@pytest.mark.parametrize("kind,qp", [(k, q) for k in ("extremes", "noise") for q in (4, 32, 51)] + [("noise_half", 4)])
def test_picture_matches_oracle(built, kind, qp, schedule):
    from wrenc_amd import gpu
    (y, cb, cr), ref = _picture_and_reference(kind, qp)
    assert (ref is None) == (qp == 4 and kind != "noise_half")
    enc = gpu.Encoder(W, H, qp=qp, max_split_depth=DEPTH, schedule=schedule)
    try:
        if ref is None:
            with pytest.raises(gpu.WrencGpuError) as err:
                enc.encode_picture(y, cb, cr)
            assert err.value.code == ELEVEL
            return
        got = enc.encode_picture(y, cb, cr)
        assert enc.final_pass_mismatches() == 0
    finally:
        enc.close()
    for k in KEYS:
        if not np.array_equal(got[k], ref[k]):
            bad = np.argwhere(got[k] != ref[k])
            raise AssertionError("%s qp%d schedule %d: %s differs at %d positions, first %s (got %s want %s)" % (
                kind, qp, schedule, k, len(bad), bad[0], got[k][tuple(bad[0])], ref[k][tuple(bad[0])]))
