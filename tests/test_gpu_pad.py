"""Pictures of any even size on the device (include/wrenc_gpu.h: wrenc_gpu_set_visible_size; the kernel is
wrenc_amd/csrc/dev_pad.h): the upload of visible-size planes leaves the slot holding the edge-padded picture of the
coded size, and everything behind it -- search, final pass, read-backs -- is that of a plain context given the padded
picture."""
import numpy as np
import pytest

from window_stream import SIZE_IDS, SIZES, pad_planes, strided, textured

pytestmark = pytest.mark.gpu

KEYS = ("rec_y", "rec_cb", "rec_cr", "lev_y", "lev_cb", "lev_cr", "cu_log2_size", "luma_mode", "chroma_mode", "ctu_cost")
EINVAL, ESTATE = -1, -5


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("visible,coded", SIZES, ids=SIZE_IDS)
def test_upload_pads_every_plane_in_every_slot(built, visible, coded):
    """Planes whose rows are further apart than they are long, into both slots of a two-slot context: the slot holds
    np.pad(mode="edge"); a second picture into a slot that held another one leaves no stale margin."""
    from wrenc_amd import gpu
    (vw, vh), (cw, ch) = visible, coded
    enc = gpu.Encoder(cw, ch, qp=32, max_split_depth=3, n_slots=2, visible=visible)
    assert enc.visible_size() == visible
    pics = [textured(vw, vh, s) for s in (1, 2, 3)]
    for slot in (0, 1):
        enc.upload_strided(slot, *strided(pics[slot]))
    for slot in (0, 1):
        got, want = enc.download_originals(slot), pad_planes(pics[slot], cw, ch)
        for p in range(3):
            assert got[p].shape == want[p].shape and np.array_equal(got[p], want[p]), (slot, p)
    enc.upload_strided(0, *strided(pics[2], extra=(8, 40, 40)))
    assert _same(enc.download_originals(0), pad_planes(pics[2], cw, ch))
    assert _same(enc.download_originals(1), pad_planes(pics[1], cw, ch))
    inverted = tuple(255 - p for p in pics[2])       # every margin sample changes
    enc.upload(0, *inverted)
    assert _same(enc.download_originals(0), pad_planes(inverted, cw, ch))
    enc.close()


@pytest.mark.parametrize("visible,coded", SIZES, ids=SIZE_IDS)
def test_encode_is_that_of_the_padded_picture(built, visible, coded):
    """Depth 3, QP 32: the whole record -- reconstruction, levels, maps, CTU costs, all at the coded size -- is bit for bit
    that of a plain context of the coded size given the numpy-padded planes."""
    from wrenc_amd import gpu
    (vw, vh), (cw, ch) = visible, coded
    pic = textured(vw, vh, 7)
    enc = gpu.Encoder(cw, ch, qp=32, max_split_depth=3, n_slots=2, visible=visible)
    enc.upload_strided(1, *strided(pic))
    enc.encode(1, 1)
    got = enc.download(1)
    assert enc.final_pass_mismatches() == 0
    enc.close()
    plain = gpu.Encoder(cw, ch, qp=32, max_split_depth=3)
    want = plain.encode_picture(*pad_planes(pic, cw, ch))
    assert plain.final_pass_mismatches() == 0
    plain.close()
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert np.any(want["lev_y"] != 0)


def test_visible_size_rules(built):
    from wrenc_amd import gpu
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=2)
    assert enc.visible_size() == (64, 64)

    def refused(w, h, code):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.set_visible_size(w, h)
        assert e.value.code == code
        assert enc.visible_size() == (enc.vis_width, enc.vis_height)

    refused(33, 62, EINVAL)      # odd
    refused(34, 61, EINVAL)
    refused(14, 16, EINVAL)      # below 16 (and not this context's size)
    refused(34, 30, EINVAL)      # rounds up to 64x32, not 64x64
    refused(94, 64, EINVAL)      # ... to 96x64
    refused(66, 62, EINVAL)
    enc.set_visible_size(34, 62)
    assert enc.visible_size() == (34, 62)
    enc.set_visible_size(62, 34)
    pic = textured(62, 34, 4)
    enc.upload(0, *pic)
    refused(34, 62, ESTATE)      # a slot has been uploaded into
    refused(64, 64, ESTATE)
    assert enc.visible_size() == (62, 34)
    enc.close()
    small = gpu.Encoder(32, 32, qp=32, max_split_depth=2)
    with pytest.raises(gpu.WrencGpuError) as e:   # a slot never uploaded into has no originals
        small.download_originals(0)
    assert e.value.code == ESTATE
    with pytest.raises(gpu.WrencGpuError) as e:
        small.set_visible_size(14, 16)
    assert e.value.code == EINVAL
    small.close()


def test_the_coded_size_restores_the_plain_behaviour(built):
    from wrenc_amd import gpu
    pic = textured(64, 64, 9)
    fresh = gpu.Encoder(64, 64, qp=32, max_split_depth=3)
    want = fresh.encode_picture(*pic)
    fresh.close()
    enc = gpu.Encoder(64, 64, qp=32, max_split_depth=3, visible=(34, 62))
    enc.set_visible_size(64, 64)
    got = enc.encode_picture(*pic)
    assert _same(enc.download_originals(0), pic)
    enc.close()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
