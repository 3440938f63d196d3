"""Per-picture QP on the CPU: the writer entries of include/wrenc_bitstream_qp.h (a slice QP apart from the parameter
sets' QP) against the test-side parser and spec decoder, and the argument errors of --qp-file."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from content import content

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "wrenc_amd", "csrc", "host", "wrenc")
REC_KEYS = ("cu_log2_size", "luma_mode", "chroma_mode", "lev_y", "lev_cb", "lev_cr")


def test_qp_entries_are_exported(built):
    from wrenc_amd import bitstream as bs
    lib = C.CDLL(bs.LIB_PATH)
    for name in bs.EXPORTED_QP_SYMBOLS:
        assert hasattr(lib, name), name
    txt = open(os.path.join(ROOT, "include", "wrenc_bitstream_qp.h")).read()
    for name in bs.EXPORTED_QP_SYMBOLS:
        assert name + "(" in txt


@pytest.mark.parametrize("q", [0, 22, 26, 37, 63])
def test_slice_qp_apart_from_the_parameter_sets(built, q):
    """A picture searched at q written into a sequence whose PPS carries QP 32: the slice header's delta and the CABAC
    initialisation follow q, and the stream decodes to the oracle's record and reconstruction at q."""
    from wrenc_amd import bitstream as bs
    from oracle import pyoracle as po
    w, h, depth = (64, 64, 2) if q >= 4 else (32, 32, 3)
    y, cb, cr = content("noise", w, h, 7)
    # (the oracle's search does not run at QP 0: there the record of QP 4 stands in, reconstructed at QP 0)
    rec = po.encode_picture(y, cb, cr, max(q, 4), depth)
    if q < 4:
        rec["rec_y"], rec["rec_cb"], rec["rec_cr"] = po.reconstruct_from_record(rec, q)
    stream = bs.write_parameter_sets(w, h, 32) + bs.write_picture_qp(w, h, 32, q, 3, rec)
    assert po.parse_stream_info(stream)["init_qp"] == 32
    back = po.parse_picture(stream, 0)
    assert back["slice_qp"] == q and back["poc_lsb"] == 3
    for k in REC_KEYS:
        assert np.array_equal(back[k], rec[k]), k
    sy, scb, scr = po.spec_decode_record(back, q)
    assert np.array_equal(sy, rec["rec_y"]) and np.array_equal(scb, rec["rec_cb"]) and np.array_equal(scr, rec["rec_cr"])


@pytest.mark.parametrize("qp", [0, 22, 26, 32, 63])
def test_equal_qps_write_the_bytes_of_the_single_qp_writer(built, qp):
    from wrenc_amd import bitstream as bs
    from oracle import pyoracle as po
    y, cb, cr = content("cclm", 64, 64, 3)
    rec = po.encode_picture(y, cb, cr, max(qp, 4), 3)
    assert bs.write_picture_qp(64, 64, qp, qp, 9, rec) == bs.write_picture(64, 64, qp, 9, rec)


def test_slice_qp_outside_the_range_is_refused(built):
    from wrenc_amd import bitstream as bs
    from oracle import pyoracle as po
    y, cb, cr = content("flat", 32, 32, 0)
    rec = po.encode_picture(y, cb, cr, 32, 1)
    for bad in (-1, 64):
        with pytest.raises(bs.BitstreamError) as e:
            bs.write_picture_qp(32, 32, 32, bad, 0, rec)
        assert e.value.code == bs.EINVAL


def _run(front, args):
    cmd = [NATIVE] if front == "native" else [sys.executable, "-m", "wrenc_amd.cli"]
    return subprocess.run(cmd + args, cwd=ROOT, capture_output=True, timeout=600)


@pytest.mark.parametrize("front", ["native", "python"])
def test_qp_file_argument_errors(built, tmp_path, front):
    """Every --qp-file error is an argument error (message, exit status 0) reported before the input is opened or a
    device is touched: the input named here does not exist, so a later failure would say so instead."""
    out = str(tmp_path / "o.vvc")
    base = ["-i", str(tmp_path / "missing.yuv"), "-o", out, "--input-size", "64x64", "--output-size", "64x64",
            "--num-pictures", "3", "--qp", "32"]
    cases = [(None, b"error: failed to open qp file"), ("22 27", b"fewer than --num-pictures 3"),
             ("22 x7 30", b"error: Invalid qp-file entry 1: x7"), ("22 27 3.5", b"error: Invalid qp-file entry 2: 3.5"),
             ("22 64 30", b"entry 1 is 64: qp must be 0..63"), ("-1 22 30", b"entry 0 is -1: qp must be 0..63")]
    for i, (text, want) in enumerate(cases):
        path = tmp_path / ("q%d.txt" % i)
        if text is not None:
            path.write_text(text)
        r = _run(front, base + ["--qp-file", str(path)])
        assert r.returncode == 0 and want in r.stderr, (text, r.stderr)
        assert b"failed to open input file" not in r.stderr
    # a good file gets past the option checks (and fails at the missing input as usual)
    path = tmp_path / "good.txt"
    path.write_text("22\n27 32\t37\n")
    r = _run(front, base + ["--qp-file", str(path)])
    assert r.returncode == 0 and b"error: failed to open input file" in r.stderr
