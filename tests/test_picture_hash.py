"""The decoded picture hash on the host (include/wrenc_bitstream_hash.h: wrenc_bs_picture_hash, wrenc_bs_write_hash_sei)
against the Python statement of picture_hash_ref.py, and the --hash option's argument handling: nothing here needs a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import picture_hash_ref as ref
from window_stream import split_nals, split_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")


def test_crc_loop_is_crc_hqx():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 3, 16, 255, 256, 1000, 4097):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert ref.crc_bitwise(data) == ref.crc_fast(data), n
    assert ref.crc_bitwise(b"") == 0x1D0F


def test_symbols_and_headers(built):
    from wrenc_amd import bitstream
    lib = C.CDLL(bitstream.LIB_PATH)
    assert sorted(bitstream.EXPORTED_HASH_SYMBOLS) == ["wrenc_bs_picture_hash", "wrenc_bs_write_hash_sei"]
    header = open(os.path.join(ROOT, "include", "wrenc_bitstream_hash.h")).read()
    for name in bitstream.EXPORTED_HASH_SYMBOLS:
        assert getattr(lib, name) and name + "(" in header
    shared = open(os.path.join(ROOT, "include", "wrenc_hash.h")).read()
    assert "WRENC_HASH_MD5 = 0, WRENC_HASH_CRC = 1, WRENC_HASH_CHECKSUM = 2" in shared and "uint8_t value[3][16];" in shared
    for h in ("wrenc_gpu.h", "wrenc_bitstream_hash.h"):
        assert '#include "wrenc_hash.h"' in open(os.path.join(ROOT, "include", h)).read()


@pytest.mark.parametrize("size", ref.SIZES, ids=ref.SIZE_IDS)
def test_picture_hash_is_the_python_statement(built, size):
    from wrenc_amd import bitstream
    w, h = size
    for name, planes in ref.pictures(w, h).items():
        for tname, t in ref.TYPES:
            got = bitstream.picture_hash(w, h, tname, *planes)
            assert got == ref.picture_values(t, planes), (name, tname)
            assert got == bitstream.picture_hash(w, h, t, *planes)
        if w * h <= 96 * 64:   # the bit loop itself, where it is quick
            assert bitstream.picture_hash(w, h, "crc", *planes) == [ref.crc_bitwise(p.tobytes()).to_bytes(2, "big") for p in planes]


def test_checksum_wraps_at_2_to_32(built):
    """7680x4320: all 255 (the luma sum stops 1.5 % short of 2^32: picture_hash_ref.py) and the mask's complement, whose
    luma sum of 255 per sample passes 2^32; 3840x2176 all 255 stays far below."""
    from wrenc_amd import bitstream
    w, h = ref.WRAP_SIZE
    cases = [(w, h, ref.filled(w, h), False), (w, h, ref.complement(w, h), True), ref.BELOW_WRAP_SIZE + (ref.filled(*ref.BELOW_WRAP_SIZE), False)]
    for w, h, planes, wraps in cases:
        full = int(np.sum(planes[0] ^ ref.checksum_mask(w, h), dtype=np.int64))
        assert (full >= 1 << 32) == wraps
        for tname, t in ref.TYPES if planes is cases[0][2] else ref.TYPES[2:]:   # (MD5 and the CRC's bit loop once at this size)
            assert bitstream.picture_hash(w, h, tname, *planes) == ref.picture_values(t, planes), (w, h, tname)
        assert bitstream.picture_hash(w, h, "checksum", *planes)[0] == (full & 0xFFFFFFFF).to_bytes(4, "big")


# values that need emulation prevention, and ones that must not get any
SEI_CASES = [
    ("md5", [bytes([1]) + bytes(range(20, 35)), bytes(range(40, 56)), bytes(range(60, 76))]),      # payload starts .. 00 00 01
    ("md5", [bytes(16), bytes(16), bytes(16)]),
    ("md5", [bytes(range(1, 15)) + b"\x00\x00", b"\x02" + bytes(range(1, 16)), bytes(range(1, 15)) + b"\x00\x00"]),
    ("checksum", [b"\x00\x00\x00\x02", b"\x12\x34\x56\x78", b"\xff\xff\xff\xff"]),
    ("checksum", [b"\x01\x00\x00\x00", b"\x00\x00\x03\x00", b"\x00\x01\x00\x00"]),                  # ends 00 00 in front of 0x80
    ("checksum", [b"\x00\x00\x00\x00"] * 3),
    ("crc", [b"\x00\x00", b"\x03\x21", b"\xab\xcd"]),
    ("crc", [b"\x12\x00", b"\x00\x01", b"\x00\x00"]),
    ("crc", [b"\x00\x00"] * 3),
    ("crc", [b"\xff\xff", b"\x80\x00", b"\x00\x03"]),
]


@pytest.mark.parametrize("case", range(len(SEI_CASES)))
def test_hash_sei_is_the_hand_built_unit(built, case):
    from wrenc_amd import bitstream
    tname, values = SEI_CASES[case]
    t = dict(ref.TYPES)[tname]
    got = bitstream.write_hash_sei(tname, values)
    want = ref.sei_nal(t, values)
    assert got == want
    assert got[:8] == ref.PREFIX + b"\x00\xc1"
    payload = ref.sei_payload(t, values)
    assert payload[1] == {"md5": 50, "crc": 8, "checksum": 14}[tname]
    # no start code inside the unit, and the unit reads back as the payload
    assert got.count(b"\x00\x00\x01") == 1 and b"\x00\x00\x00" not in got[6:] and b"\x00\x00\x02" not in got[6:]
    assert split_nals(got) == [(ref.NAL_SUFFIX_SEI, payload)]
    assert ref.parse_sei(payload) == (t, values)
    assert len(split_raw(got)) == 1


def test_emulation_prevention_cases_are_what_they_claim(built):
    """The cases above do hold the byte patterns the writer must escape."""
    from wrenc_amd import bitstream
    md5_first = ref.sei_payload(ref.MD5, SEI_CASES[0][1])
    assert md5_first[2:5] == b"\x00\x00\x01"                      # hash_type 0, the flag byte, digest byte 0x01
    assert ref.sei_payload(ref.CHECKSUM, SEI_CASES[3][1])[4:8] == b"\x00\x00\x00\x02"
    assert ref.sei_payload(ref.CRC, SEI_CASES[6][1])[4:7] == b"\x00\x00\x03"
    assert ref.sei_payload(ref.CHECKSUM, SEI_CASES[4][1])[-3:] == b"\x00\x00\x80"
    for tname, values in SEI_CASES[:1] + SEI_CASES[3:5] + SEI_CASES[6:7]:
        t = dict(ref.TYPES)[tname]
        assert len(bitstream.write_hash_sei(tname, values)) > 8 + len(ref.sei_payload(t, values))
    # ... and a value ending 00 00 in front of the trailing 0x80 gets no byte there
    tail = [b"\x11\x22\x00\x00", b"\x33\x44\x55\x66", b"\x77\x88\x00\x00"]
    assert bitstream.write_hash_sei("checksum", tail) == ref.PREFIX + b"\x00\xc1" + ref.sei_payload(ref.CHECKSUM, tail)


def _raw_calls():
    from wrenc_amd import bitstream
    lib = bitstream.load_library()
    lib.wrenc_bs_picture_hash.restype = C.c_int
    lib.wrenc_bs_picture_hash.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wrenc_bs_write_hash_sei.restype = C.c_int
    lib.wrenc_bs_write_hash_sei.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    return bitstream, lib


def test_picture_hash_rejects_bad_arguments(built):
    bitstream, lib = _raw_calls()
    y, cb, cr = ref.pictures(64, 64)["noise"]
    out = (C.c_uint8 * 48)()
    ptr = lambda a: a.ctypes.data
    assert lib.wrenc_bs_picture_hash(64, 64, 0, ptr(y), ptr(cb), ptr(cr), out) == bitstream.OK
    for t in (-1, 3, 132):
        assert lib.wrenc_bs_picture_hash(64, 64, t, ptr(y), ptr(cb), ptr(cr), out) == bitstream.EINVAL
    for w, h in ((60, 64), (64, 48), (0, 64), (64, -32), (70, 50)):
        assert lib.wrenc_bs_picture_hash(w, h, 0, ptr(y), ptr(cb), ptr(cr), out) == bitstream.EINVAL
    for args in ((None, ptr(cb), ptr(cr), out), (ptr(y), None, ptr(cr), out), (ptr(y), ptr(cb), None, out), (ptr(y), ptr(cb), ptr(cr), None)):
        assert lib.wrenc_bs_picture_hash(64, 64, 0, *args) == bitstream.EINVAL
    with pytest.raises(bitstream.BitstreamError):
        bitstream.picture_hash(64, 64, 3, y, cb, cr)


def test_hash_sei_enospc_and_einval(built):
    bitstream, lib = _raw_calls()
    rec = (C.c_uint8 * 48)(*range(16, 64))   # (no byte that needs emulation prevention)
    for t, size in ((0, 8 + 53), (1, 8 + 11), (2, 8 + 17)):
        n = C.c_size_t(0)
        assert lib.wrenc_bs_write_hash_sei(t, rec, None, 0, C.byref(n)) == bitstream.ENOSPC and n.value == size
        buf = np.full(size + 4, 0xEE, np.uint8)
        n = C.c_size_t(0)
        assert lib.wrenc_bs_write_hash_sei(t, rec, buf.ctypes.data, size - 1, C.byref(n)) == bitstream.ENOSPC and n.value == size
        assert np.all(buf == 0xEE)
        assert lib.wrenc_bs_write_hash_sei(t, rec, buf.ctypes.data, size, C.byref(n)) == bitstream.OK and n.value == size
        assert np.all(buf[size:] == 0xEE) and buf[:size].tobytes() == bitstream.write_hash_sei(t, bytes(rec))
    n = C.c_size_t(0)
    buf = np.zeros(128, np.uint8)
    for t in (-1, 3):
        assert lib.wrenc_bs_write_hash_sei(t, rec, buf.ctypes.data, buf.size, C.byref(n)) == bitstream.EINVAL
    assert lib.wrenc_bs_write_hash_sei(0, None, buf.ctypes.data, buf.size, C.byref(n)) == bitstream.EINVAL


@pytest.mark.parametrize("front", ["native", "python"])
def test_unknown_hash_name_is_an_argument_error(built, tmp_path, front):
    """Refused before any context is made: the same answer with and without a device."""
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    out = tmp_path / "o.vvc"
    base = cmd + ["-i", str(tmp_path / "missing.yuv"), "-o", str(out), "--input-size", "64x64", "--output-size", "64x64",
                  "--num-pictures", "1", "--qp", "32"]
    r = subprocess.run(base + ["--hash", "bogus"], cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0 and b"error: Invalid hash: bogus (md5, crc, checksum)" in r.stderr, r.stderr
    assert not out.exists()
    r = subprocess.run(base + ["--hash"], cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0 and b"error: option --hash needs a value" in r.stderr, r.stderr
    assert not out.exists()
