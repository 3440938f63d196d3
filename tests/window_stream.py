"""Shared by the conformance-window tests (test_bitstream_window.py, test_gpu_pad.py, test_gpu_metrics_window.py,
test_gpu_cli_pad.py): the sizes they cover, edge padding in numpy, and a reader of just enough of the SPS to find
sps_conformance_window_flag (H.266 7.3.2.4)."""
import numpy as np

from content import content

# visible -> coded: margins of 30 (the maximum), 2 (the minimum) and 0, in both directions, more than one CTU per row and per
# column, chroma widths that are no multiple of 4 (17, 31, 33, 47)
SIZES = [((34, 62), (64, 64)), ((62, 34), (64, 64)), ((66, 30), (96, 32)), ((16, 16), (32, 32)), ((94, 64), (96, 64))]
SIZE_IDS = ["%dx%d" % v for v, _ in SIZES]
NAL_VPS, NAL_SPS, NAL_PPS = 14, 15, 16
PREFIX = b"\x00\x00\x00\x00\x00\x01"


def coded_size(w, h):
    return (w + 31) // 32 * 32, (h + 31) // 32 * 32


def textured(w, h, seed):
    """Content whose margin matters: smooth texture plus noise, chroma following luma."""
    return content("cclm", w, h, seed)


def pad_planes(planes, cw, ch):
    """(y, cb, cr) of the visible size -> the coded size, last column and row replicated."""
    out = []
    for p, (pw, ph) in zip(planes, ((cw, ch), (cw // 2, ch // 2), (cw // 2, ch // 2))):
        out.append(np.ascontiguousarray(np.pad(p, ((0, ph - p.shape[0]), (0, pw - p.shape[1])), mode="edge")))
    return tuple(out)


def crop_planes(planes, w, h):
    return tuple(np.ascontiguousarray(p[:hh, :ww]) for p, (ww, hh) in zip(planes, ((w, h), (w // 2, h // 2), (w // 2, h // 2))))


def strided(planes, extra=(24, 8, 8)):
    """Views of the planes inside wider arrays filled with another value: rows further apart than they are long (the two
    chroma planes with the same stride)."""
    out = []
    for p, e in zip(planes, extra):
        wide = np.full((p.shape[0], p.shape[1] + e), 0xA5, np.uint8)
        wide[:, :p.shape[1]] = p
        out.append(wide[:, :p.shape[1]])
    return tuple(out)


def split_nals(stream):
    """[(nal_unit_type, RBSP bytes)] of a byte stream with the six-byte prefix, emulation prevention bytes removed."""
    assert stream.startswith(PREFIX)
    nals = []
    for unit in stream.split(PREFIX)[1:]:
        body, zeros = bytearray(), 0
        for b in unit[2:]:
            if zeros >= 2 and b == 3:
                zeros = 0
                continue
            body.append(b)
            zeros = zeros + 1 if b == 0 else 0
        nals.append((unit[1] >> 3, bytes(body)))
    return nals


def split_raw(stream):
    """The NAL units as they are in the stream (prefix removed, nothing else touched)."""
    assert stream.startswith(PREFIX)
    return stream.split(PREFIX)[1:]


class Bits:
    def __init__(self, data):
        self.s = "".join(format(b, "08b") for b in data)
        self.at = 0

    def u(self, n):
        v = int(self.s[self.at:self.at + n], 2)
        self.at += n
        return v

    def ue(self):
        zeros = 0
        while self.s[self.at] == "0":
            zeros += 1
            self.at += 1
        return self.u(zeros + 1) - 1

    def align(self):
        self.at = (self.at + 7) // 8 * 8


def sps_to_window_flag(rbsp):
    """(Bits positioned at sps_conformance_window_flag, pic_width_max, pic_height_max) of an SPS RBSP as this encoder writes
    it: one sub-layer, a profile_tier_level without GCI or sub-profiles."""
    b = Bits(rbsp)
    b.u(4), b.u(4)                     # sps id, vps id
    assert b.u(3) == 0                 # max_sublayers - 1
    assert b.u(2) == 1                 # 4:2:0
    assert b.u(2) == 0                 # CTU 32
    assert b.u(1) == 1                 # ptl_dpb_hrd_params_present_flag
    b.u(7), b.u(1), b.u(8), b.u(1), b.u(1)
    assert b.u(1) == 0                 # gci_present_flag
    b.align()
    assert b.u(8) == 0                 # ptl_num_sub_profiles
    b.u(1)                             # gdr_enabled_flag
    assert b.u(1) == 0                 # ref_pic_resampling_enabled_flag
    w, h = b.ue(), b.ue()
    return b, w, h


def payload_bits(bits):
    """An RBSP's bits without rbsp_trailing_bits."""
    stop = bits.rindex("1")
    assert len(bits) % 8 == 0 and len(bits) - stop <= 8
    return bits[:stop]


def check_window_sps(plain, windowed, coded, visible):
    """`windowed` is the SPS `plain` with the window fields and nothing else: equal up to and including
    sps_pic_height_max; then 1, ue(0), ue(right), ue(0), ue(bottom); then the plain SPS's bits after its own flag; then the
    trailing bits re-aligned."""
    (cw, ch), (vw, vh) = coded, visible
    p, pw, ph = sps_to_window_flag(plain)
    q, qw, qh = sps_to_window_flag(windowed)
    assert (pw, ph) == (qw, qh) == (cw, ch)
    assert p.at == q.at and p.s[:p.at] == q.s[:q.at]
    assert p.u(1) == 0 and q.u(1) == 1
    assert [q.ue() for _ in range(4)] == [0, (cw - vw) // 2, 0, (ch - vh) // 2]
    rest = payload_bits(p.s)[p.at:]
    assert len(rest) > 100
    want = q.s[:q.at] + rest + "1"
    want += "0" * (-len(want) % 8)
    assert q.s == want
