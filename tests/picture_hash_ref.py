"""Reference side of the decoded-picture-hash tests: the three hashes of H.274's decoded picture hash SEI restated in Python
(include/wrenc_hash.h has the definitions), the SEI's NAL unit built by hand, and the pictures the tests share."""
import binascii
import hashlib

import numpy as np

MD5, CRC, CHECKSUM = 0, 1, 2
TYPES = [("md5", MD5), ("crc", CRC), ("checksum", CHECKSUM)]
TYPE_IDS = [name for name, _ in TYPES]
VALUE_BYTES = {MD5: 16, CRC: 2, CHECKSUM: 4}
NAL_SUFFIX_SEI = 24
PREFIX = b"\x00\x00\x00\x00\x00\x01"

# 544x32 and 32x544: the smallest sizes where x >> 8 and y >> 8 of the checksum's mask are non-zero in luma and chroma
SIZES = [(32, 32), (96, 64), (352, 288), (544, 32), (32, 544)]
SIZE_IDS = ["%dx%d" % s for s in SIZES]
# The checksum is a sum modulo 2^32.  A plane of one value sums to about 127.5 per sample whatever the value (the mask
# takes every 8-bit value equally often), so all 255 at 7680x4320 reaches 4,230,144,000 in luma, 1.5 % short of 2^32, and
# at 3840x2176 a quarter of it.  The sum that does pass 2^32 is that of the mask's complement (`complement` below), 255
# per sample: 8,460,288,000 in luma at 7680x4320.  The tests run both at that size.
WRAP_SIZE = (7680, 4320)
BELOW_WRAP_SIZE = (3840, 2176)


def crc_bitwise(data):
    """The definition, bit by bit: register 0xFFFF, polynomial 0x1021, MSB first, 16 zero bits behind the data."""
    crc = 0xFFFF
    for byte in bytes(data) + b"\x00\x00":
        for k in range(7, -1, -1):
            bit = (byte >> k) & 1
            msb = (crc >> 15) & 1
            crc = ((crc << 1 | bit) & 0xFFFF) ^ (0x1021 if msb else 0)
    return crc


def crc_fast(data):
    """The same value from the C library's table: crc_hqx shifts the 16 zero bits in as it goes; the register 0xFFFF in
    front of 16 zero bits is crc_hqx's start value 0x1D0F."""
    return binascii.crc_hqx(bytes(data), 0x1D0F)


def checksum(plane):
    h, w = plane.shape
    return int(np.sum(plane ^ checksum_mask(w, h), dtype=np.int64)) & 0xFFFFFFFF


def plane_value(hash_type, plane):
    """The bytes the SEI carries for one component."""
    plane = np.ascontiguousarray(plane, np.uint8)
    if hash_type == MD5:
        return hashlib.md5(plane.tobytes()).digest()
    if hash_type == CRC:
        return crc_fast(plane.tobytes()).to_bytes(2, "big")
    return checksum(plane).to_bytes(4, "big")


def picture_values(hash_type, planes):
    return [plane_value(hash_type, p) for p in planes]


def sei_payload(hash_type, values):
    """The RBSP of the SEI NAL unit: the message and rbsp_trailing_bits."""
    body = b"".join(values)
    assert len(body) == 3 * VALUE_BYTES[hash_type]
    return bytes([132, 2 + len(body), hash_type, 0]) + body + b"\x80"


def escape(rbsp):
    """Emulation prevention as H.266 7.4.2 words it: a 0x03 in front of every byte <= 3 that follows two zero bytes."""
    out, zeros = bytearray(), 0
    for b in rbsp:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def sei_nal(hash_type, values):
    """The whole unit: prefix, header 00 C1 (SUFFIX_SEI_NUT = 24, layer 0, temporal id 0), escaped payload."""
    return PREFIX + bytes([0x00, (NAL_SUFFIX_SEI << 3) | 1]) + escape(sei_payload(hash_type, values))


def parse_sei(rbsp):
    """(hash_type, [Y, Cb, Cr values]) of a SUFFIX_SEI RBSP as this encoder writes it."""
    assert rbsp[0] == 132 and rbsp[-1] == 0x80 and rbsp[1] == len(rbsp) - 3
    hash_type, n = rbsp[2], VALUE_BYTES[rbsp[2]]
    assert rbsp[3] == 0 and rbsp[1] == 2 + 3 * n
    return hash_type, [bytes(rbsp[4 + n * p:4 + n * (p + 1)]) for p in range(3)]


def pictures(w, h):
    """{name: (y, cb, cr)}: zeros, 255 and seeded noise."""
    rng = np.random.default_rng(w * 31 + h)
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    return {"zeros": tuple(np.zeros(s, np.uint8) for s in shapes), "ones": tuple(np.full(s, 255, np.uint8) for s in shapes),
            "noise": tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in shapes)}


def filled(w, h, v=255):
    return tuple(np.full(s, v, np.uint8) for s in [(h, w), (h // 2, w // 2), (h // 2, w // 2)])


def checksum_mask(w, h):
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    return ((x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)).astype(np.uint8)


def complement(w, h):
    """The picture whose every sample is 255 ^ mask: each term of the checksum is 255."""
    return tuple(np.uint8(255) ^ checksum_mask(ww, hh) for ww, hh in ((w, h), (w // 2, h // 2), (w // 2, h // 2)))


def strip_sei(stream):
    """(the stream without its type-24 units, [(index of the unit in front, raw unit)] of the removed ones); units as
    window_stream.split_raw gives them."""
    units = stream.split(PREFIX)[1:]
    assert stream.startswith(PREFIX)
    kept, sei = [], []
    for u in units:
        if u[1] >> 3 == NAL_SUFFIX_SEI:
            sei.append((len(kept) - 1, u))
        else:
            kept.append(u)
    return b"".join(PREFIX + u for u in kept), sei
