"""wrenc_gpu_test_predict_layout (host only, no device): the one owner of what an item of wrenc_gpu_test_predict may be and
of how many bytes it puts out (wrenc_amd/csrc/predict_items.h).  Sizes as include/wrenc_gpu_test.h states them, and the
refusal of every kind of bad item -- "a bad item must never reach the kernel"."""
import numpy as np
import pytest

W = H = 64
LIST = 2 | 1 << 8 | 1 << 16          # a SAD list: first mode 2, one entry, stride 1


def pack(*modes):
    word = len(modes) << 24
    for j, m in enumerate(modes):
        word |= m << (8 * j)
    return word


def layout(items):
    """(status, offsets) of the library's layout of (n, 5) items on a W x H picture."""
    from wrenc_amd import gpu
    lib = gpu.load_library()
    it = np.ascontiguousarray(items, np.int32).reshape(-1, 5)
    at = np.full(len(it) + 1, 12345, np.uintp)
    rc = lib.wrenc_gpu_test_predict_layout(W, H, len(it), it.ctypes.data, at.ctypes.data)
    return rc, [int(v) for v in at]


# one item of every kind at its smallest legal size: (x, y, log2 size, kind, mode word) -> bytes
SMALLEST = [
    ((0, 0, 2, 0, 0), 16), ((8, 8, 3, 1, 0), 32), ((4, 60, 2, 2, 66), 16),
    ((0, 0, 2, 4, LIST), 64), ((0, 0, 3, 5, LIST), 64), ((0, 0, 3, 6, LIST), 64), ((0, 0, 3, 7, 0), 64),
    ((0, 0, 3, 8, 0), 192), ((0, 0, 3, 9, 81), 96),
    ((0, 0, 3, 10, pack(0)), 192), ((8, 0, 3, 10, pack(0, 255, 66)), 576),
    ((0, 0, 4, 11, pack(50)), 1152), ((48, 48, 4, 11, pack(255, 1)), 2304),
]


def test_sizes_of_every_kind(built):
    for item, size in SMALLEST:
        assert layout([item]) == (0, [0, size]), item
    rc, at = layout([item for item, _ in SMALLEST])
    assert rc == 0 and at == [int(v) for v in np.cumsum([0] + [size for _, size in SMALLEST])]
    # sizes follow the block: luma n^2, pair n^2 / 2, full candidates three bytes per sample, lists 64 whatever the size
    assert layout([(32, 32, 5, 0, 66), (32, 0, 5, 1, 83), (0, 32, 5, 8, 1), (0, 0, 5, 9, 82), (0, 0, 5, 6, LIST)])[1] == \
        [0, 1024, 1536, 4608, 6144, 6208]


REFUSED = {
    "x not a multiple of the size": (4, 0, 3, 0, 0),
    "y not a multiple of the size": (0, 12, 4, 0, 0),
    "crosses the right edge": (64, 0, 3, 0, 0),
    "crosses the bottom edge": (0, 64, 2, 0, 0),
    "negative x": (-8, 0, 3, 0, 0),
    "log2 size 1": (0, 0, 1, 0, 0),
    "log2 size 6": (0, 0, 6, 0, 0),
    "kind 1 at 4x4": (0, 0, 2, 1, 0),
    "kind 2 at 8x8": (0, 0, 3, 2, 0),
    "kind 5 at 4x4": (0, 0, 2, 5, LIST),
    "kind 9 at 4x4": (0, 0, 2, 9, 0),
    "mode 67": (0, 0, 3, 0, 67),
    "mode 67, full candidate": (0, 0, 3, 8, 67),
    "a CCLM mode on kind 0": (0, 0, 3, 0, 81),
    "a CCLM mode on kind 8": (0, 0, 3, 8, 82),
    "mode 84 on kind 1": (0, 0, 3, 1, 84),
    "a list of 0 entries": (0, 0, 3, 4, 2 | 0 << 8 | 1 << 16),
    "a list of 17 entries": (0, 0, 3, 4, 2 | 17 << 8 | 1 << 16),
    "stride 0": (0, 0, 3, 4, 2 | 1 << 8 | 0 << 16),
    "stride 65": (0, 0, 3, 4, 2 | 1 << 8 | 65 << 16),
    "a first mode below 2": (0, 0, 3, 6, 1 | 1 << 8 | 1 << 16),
    "a first mode of 67": (0, 0, 3, 6, 67 | 1 << 8 | 1 << 16),
    "kind 7 with a mode": (0, 0, 3, 7, 1),
    "a pack of 0 candidates": (0, 0, 3, 10, pack()),
    "a pack of 4 candidates (kind 10)": (0, 0, 3, 10, 4 << 24),
    "a pack of 3 candidates (kind 11)": (0, 0, 4, 11, pack(0, 0, 0)),
    "kind 10 at 16x16": (0, 0, 4, 10, pack(0)),
    "kind 11 at 8x8": (0, 0, 3, 11, pack(0)),
    "a pack mode of 67": (0, 0, 3, 10, pack(0, 67)),
    "a pack mode of 254": (0, 0, 4, 11, pack(254)),
    "a negative mode word": (0, 0, 3, 0, -1),
    "a negative pack word": (0, 0, 3, 10, -(1 << 31) | pack(0)),
    "kind 3": (0, 0, 3, 3, 0),
    "kind 12": (0, 0, 3, 12, 0),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_bad_item_is_refused(built, why):
    good = SMALLEST[0][0]
    assert layout([REFUSED[why]])[0] == -1, why          # WRENC_GPU_EINVAL
    assert layout([good, REFUSED[why], good])[0] == -1, why
    assert layout([good, good, REFUSED[why]])[0] == -1, why


def test_layout_refuses_missing_arguments(built):
    from wrenc_amd import gpu
    lib = gpu.load_library()
    it = np.array([SMALLEST[0][0]], np.int32)
    at = np.zeros(2, np.uintp)
    assert lib.wrenc_gpu_test_predict_layout(W, H, 0, it.ctypes.data, at.ctypes.data) == -1
    assert lib.wrenc_gpu_test_predict_layout(W, H, 1, None, at.ctypes.data) == -1
    assert lib.wrenc_gpu_test_predict_layout(W, H, 1, it.ctypes.data, None) == -1
    # a picture smaller than the block
    assert lib.wrenc_gpu_test_predict_layout(16, 16, 1, np.array([(0, 0, 5, 0, 0)], np.int32).ctypes.data, at.ctypes.data) == -1
