"""wrenc_bs_write_parameter_sets_window (include/wrenc_bitstream_window.h): the parameter sets of a picture coded at the next
multiple of the CTU size with a conformance window in the SPS.  The repository's parser accepts only
sps_conformance_window_flag == 0, so nothing here hands it a windowed SPS: the windowed sets are shown to differ from
the plain sets of the coded size -- which the parser and decoder tests cover -- in the SPS alone and by exactly the window
fields."""
import ctypes as C

import pytest

from window_stream import NAL_PPS, NAL_SPS, NAL_VPS, SIZE_IDS, SIZES, check_window_sps, split_nals


@pytest.mark.parametrize("qp", [22, 32])
@pytest.mark.parametrize("visible,coded", SIZES, ids=SIZE_IDS)
def test_window_differs_from_plain_in_the_sps_alone(built, visible, coded, qp):
    from wrenc_amd import bitstream as bs
    plain = split_nals(bs.write_parameter_sets(coded[0], coded[1], qp))
    win = split_nals(bs.write_parameter_sets_window(coded[0], coded[1], visible[0], visible[1], qp))
    assert [t for t, _ in plain] == [t for t, _ in win] == [NAL_VPS, NAL_SPS, NAL_PPS]
    assert win[0] == plain[0] and win[2] == plain[2]
    assert win[1][1] != plain[1][1]
    check_window_sps(plain[1][1], win[1][1], coded, visible)


@pytest.mark.parametrize("w,h", [(32, 32), (64, 64), (96, 32), (1920, 1088)])
def test_visible_equal_to_coded_gives_the_plain_bytes(built, w, h):
    from wrenc_amd import bitstream as bs
    for qp in (22, 32):
        assert bs.write_parameter_sets_window(w, h, w, h, qp) == bs.write_parameter_sets(w, h, qp)


def test_1080p(built):
    from wrenc_amd import bitstream as bs
    plain = split_nals(bs.write_parameter_sets(1920, 1088, 32))
    win = split_nals(bs.write_parameter_sets_window(1920, 1088, 1920, 1080, 32))
    check_window_sps(plain[1][1], win[1][1], (1920, 1088), (1920, 1080))


def test_refused_geometries(built):
    from wrenc_amd import bitstream as bs
    lib = bs.load_library()
    fn = lib.wrenc_bs_write_parameter_sets_window
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    buf = (C.c_uint8 * 4096)()
    n = C.c_size_t()

    def rc(cw, ch, vw, vh, qp=32):
        return fn(cw, ch, vw, vh, qp, buf, len(buf), C.byref(n))

    assert rc(64, 64, 34, 62) == bs.OK
    assert rc(64, 64, 33, 62) == bs.EINVAL and rc(64, 64, 34, 61) == bs.EINVAL        # odd
    assert rc(32, 32, 14, 16) == bs.EINVAL and rc(32, 32, 16, 14) == bs.EINVAL        # below 16
    assert rc(32, 32, 16, 16) == bs.OK
    assert rc(96, 64, 34, 62) == bs.EINVAL and rc(64, 96, 34, 62) == bs.EINVAL        # coded size too large by 32
    assert rc(32, 64, 34, 62) == bs.EINVAL and rc(64, 32, 34, 62) == bs.EINVAL        # ... smaller than the visible size
    assert rc(100, 64, 98, 64) == bs.EINVAL                                            # coded size not whole CTUs
    assert rc(64, 64, 34, 62, qp=64) == bs.EINVAL
    with pytest.raises(bs.BitstreamError) as e:
        bs.write_parameter_sets_window(64, 64, 35, 62, 32)
    assert e.value.code == bs.EINVAL
    # the existing entry keeps refusing what is not whole CTUs
    assert lib.wrenc_bs_write_parameter_sets(100, 64, 32, buf, len(buf), C.byref(n)) == bs.EINVAL
