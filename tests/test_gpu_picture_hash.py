"""The decoded picture hash on the device (include/wrenc_gpu.h: wrenc_gpu_download_hashes, wrenc_gpu_test_hash; the kernels
are wrenc_amd/csrc/dev_hash.h) against the host library's wrenc_bs_picture_hash and the Python statement of
picture_hash_ref.py: the kernels alone on arbitrary pictures, one byte flipped at every boundary of the kernels' layout,
and the hashes of what a real search reconstructed."""
import os
import re

import numpy as np
import pytest

import picture_hash_ref as ref
from content import content

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -5
KINDS = ("cclm", "stripes20", "noise", "flat", "ramp", "checker", "extremes", "stripes70", "cclm")


def _layout():
    """The constants of dev_hash.h's layout: 16 bytes per lane and load, 1 KiB per wave and load, kHashLoads loads per piece."""
    src = open(os.path.join(ROOT, "wrenc_amd", "csrc", "dev_hash.h")).read()
    loads = int(re.search(r"constexpr int kHashLoads = (\d+);", src).group(1))
    assert re.search(r"constexpr int kHashPiece = kHashLoads \* 1024;", src)
    return 16, 1024, loads * 1024


def _check(bitstream, w, h, planes, got, tname, t):
    want = ref.picture_values(t, planes)
    assert got.values(tname) == want, (tname, [v.hex() for v in got.values(tname)], [v.hex() for v in want])
    assert got.values(tname) == bitstream.picture_hash(w, h, tname, *planes)
    raw = bytes(got)
    n = ref.VALUE_BYTES[t]
    assert all(raw[16 * p + n:16 * p + 16] == bytes(16 - n) for p in range(3))


@pytest.mark.parametrize("size", ref.SIZES, ids=ref.SIZE_IDS)
def test_kernels_against_the_host_and_python(built, size):
    from wrenc_amd import bitstream, gpu
    w, h = size
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2)
    for name, planes in ref.pictures(w, h).items():
        for tname, t in ref.TYPES:
            _check(bitstream, w, h, planes, enc.test_hash(planes, tname), tname, t)
    enc.close()


def test_checksum_wrap_at_7680x4320(built):
    """All 255, and the mask's complement whose luma checksum passes 2^32 (picture_hash_ref.py): 8100 partials per luma
    plane and 2025 per chroma plane go through the finish."""
    from wrenc_amd import gpu
    w, h = ref.WRAP_SIZE
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2)
    planes = ref.filled(w, h)
    for tname, t in ref.TYPES:
        assert enc.test_hash(planes, tname).values(tname) == ref.picture_values(t, planes), tname
    planes = ref.complement(w, h)
    assert int(np.sum(planes[0] ^ ref.checksum_mask(w, h), dtype=np.int64)) >= 1 << 32
    for tname, t in (("checksum", ref.CHECKSUM), ("crc", ref.CRC)):
        assert enc.test_hash(planes, tname).values(tname) == ref.picture_values(t, planes), tname
    enc.close()


def test_one_flipped_byte_at_every_boundary(built):
    """96x64 noise: the first and last byte of each plane, and both sides of every boundary of the layout -- between two
    lanes' 16 bytes, between two loads of a wave (1 KiB), between two pieces (two waves, two partials of the finish).  The
    pieces are counted from the plane's end."""
    from wrenc_amd import gpu
    w, h = 96, 64
    lane, load, piece = _layout()
    base = ref.pictures(w, h)["noise"]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2)
    before = {t: enc.test_hash(base, tname).values(tname) for tname, t in ref.TYPES}
    for p in range(3):
        n = base[p].size
        first_piece = n % piece or piece           # bytes of the plane's first (short) piece
        at = {0, n - 1}
        for edge in (first_piece % load or load, first_piece, n - piece, n - load, n - lane, lane):
            for o in (edge - 1, edge):
                if 0 <= o < n:
                    at.add(o)
        if p == 0:
            assert n > piece and 0 < first_piece < n   # the luma plane has two pieces: a boundary of the finish
        assert len(at) >= 8
        for o in sorted(at):
            planes = [a.copy() for a in base]
            planes[p].reshape(-1)[o] ^= 0x40
            for tname, t in ref.TYPES:
                got = enc.test_hash(planes, tname).values(tname)
                want = ref.picture_values(t, planes)
                assert got == want, (p, o, tname)
                assert got[p] != before[t][p] and all(got[q] == before[t][q] for q in range(3) if q != p), (p, o, tname)
    enc.close()


def _frames(w, h):
    return [content(k, w, h, i) for i, k in enumerate(KINDS)]


def test_after_a_real_search(built):
    """9 pictures of different kinds in one encode call: each slot's hash is the reference hash of the slot's downloaded
    reconstruction, the same in calls of 4 + 5, and asking changes nothing in the slots."""
    from wrenc_amd import bitstream, gpu
    w, h = 96, 64
    frames = _frames(w, h)
    enc = gpu.Encoder(w, h, qp=30, max_split_depth=2, n_slots=len(frames))
    for s, f in enumerate(frames):
        enc.upload(s, *f)
    enc.encode(0, len(frames))
    before = [enc.download(s) for s in range(len(frames))]
    for tname, t in ref.TYPES:
        got = enc.download_hashes(0, len(frames), tname)
        assert len(got) == len(frames)
        for s in range(len(frames)):
            rec = (before[s]["rec_y"], before[s]["rec_cb"], before[s]["rec_cr"])
            _check(bitstream, w, h, rec, got[s], tname, t)
        assert len({bytes(g) for g in got}) > 4
        split = enc.download_hashes(0, 4, tname) + enc.download_hashes(4, 5, tname)
        assert [bytes(g) for g in split] == [bytes(g) for g in got]
    after = [enc.download(s) for s in range(len(frames))]
    for s in range(len(frames)):
        for k in before[s]:
            assert np.array_equal(after[s][k], before[s][k]), (s, k)
    assert enc.final_pass_mismatches() == 0
    enc.close()


def test_slot_states_and_types(built):
    from wrenc_amd import gpu
    w, h = 64, 64
    frames = _frames(w, h)[:2]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=2)

    def refused(first, n, hash_type, code):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.download_hashes(first, n, hash_type)
        assert e.value.code == code

    enc.upload(0, *frames[0])
    refused(0, 1, "crc", ESTATE)             # uploaded into, not encoded
    enc.upload(1, *frames[1])
    enc.encode(0, 2)
    refused(0, 2, 3, EINVAL)
    refused(0, 2, -1, EINVAL)
    for first, n in ((2, 1), (-1, 1), (1, 2), (0, 0)):
        refused(first, n, "md5", EINVAL)
    with pytest.raises(gpu.WrencGpuError) as e:
        enc.test_hash(frames[0], 3)
    assert e.value.code == EINVAL
    got = enc.download_hashes(0, 2, "checksum")
    with pytest.raises(gpu.WrencGpuError) as e:      # timed only in measurement mode
        enc.last_hash_ms()
    assert e.value.code == ESTATE
    enc.stats_enable()
    assert [bytes(g) for g in enc.download_hashes(0, 2, "checksum")] == [bytes(g) for g in got]
    assert 0.0 < enc.last_hash_ms() < 1000.0
    enc.stats_enable(False)
    enc.upload(1, *frames[0])
    refused(0, 2, "checksum", ESTATE)        # encoded, then uploaded into again
    assert bytes(enc.download_hashes(0, 1, "checksum")[0]) == bytes(got[0])
    d = enc.download(0)
    assert got[0].values("checksum") == ref.picture_values(ref.CHECKSUM, (d["rec_y"], d["rec_cb"], d["rec_cr"]))
    enc.close()
