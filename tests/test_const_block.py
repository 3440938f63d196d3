"""The constant block the device is given (wrenc_amd/csrc/dev_const.h; filled on the host by const_block.cpp, fill_dev_const)
against the Python statements of its parts that the tests and tools already work with, on the CPU: every member is read
through wrenc_gpu_test_const_field, which builds the block for a config and needs no device.  All comparisons are exact:
integers by value, the float floors bit by bit.  (head_rng and avail_tab are held against the device functions they
restate, on the device: tests/test_gpu_blocks.py.)"""
import json
import math
import os

import numpy as np
import pytest

import candidate_floors as cf
import dct_mfma_model as dm
import quant_inputs as qi
import split_floors as sf

HERE = os.path.dirname(os.path.abspath(__file__))
QPS = (0, 22, 32, 51, 63)
DEPTHS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def gpu(built):
    from wrenc_amd import gpu
    return gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _floors(gpu, cfg):
    return (gpu.const_field(cfg, "split_floor", np.float32), gpu.const_field(cfg, "cand_floor", np.float32),
            gpu.const_field(cfg, "cand_floor_ang", np.float32))


def _assert_floors_equal_the_models(gpu, cfg):
    split, cand, ang = _floors(gpu, cfg)
    fl = sf.floors_of_config(cfg)
    assert split.shape == (5,) and cand.shape == (67,) and ang.shape == (1,)
    assert np.array_equal(_bits(split), _bits([fl.leaf4, fl.leafc4] + fl.node))
    cl = cf.floors_of_config(cfg)
    assert np.array_equal(_bits(cand), _bits(cl.cls))
    assert np.array_equal(_bits(ang), _bits([cl.ang]))
    return split, cand, ang


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("qp", QPS)
def test_floors_equal_the_models(gpu, qp, depth):
    split, cand, _ = _assert_floors_equal_the_models(gpu, gpu.default_config(64, 64, qp, depth))
    assert (split > 0).all() and np.isfinite(cand).all()      # the default tables prove every floor


@pytest.mark.parametrize("depth", DEPTHS)
def test_floors_where_a_split_is_cheaper_than_its_node(gpu, depth):
    """With the default tables four children always cost more than the unsplit block and the cheapest angular class is a
    remainder, so neither the depth nor the first angular class shows in the floors.  Here the single-tree header bits
    are sixteen times their defaults and class 2 (mpm_idx 1) is the cheapest dual-tree class.  At depth 3 an 8x8 node's
    children are 4x4 leaves and a chroma leaf, cheaper together than the node, and so on upwards: all three node floors
    are sums of children.  At a smaller depth an 8x8 node is a leaf, four of which cost more than their parent: every
    node floor is the unsplit one.  The angular minimum lies at the first class it may look at."""
    cfg = gpu.default_config(64, 64, 32, depth)
    for cc in range(4):
        for cls in range(67):
            cfg.header_bits_luma[0][cc][cls] *= 16
    cfg.header_bits_luma[1][0][2] = 3
    split, cand, ang = _assert_floors_equal_the_models(gpu, cfg)
    single = sf.floors_of_config(cfg).single
    for level in range(3):
        if depth == 3:
            assert 0 < split[2 + level] < single, level
        else:
            assert _bits(split[2 + level:3 + level]) == _bits([single]), (level, depth)
    assert _bits(ang) == _bits(cand[2:3]) and (cand[3:] > ang[0]).all() and (cand[:2] > ang[0]).all()


def _unproven_configs(gpu):
    out = {}
    out["negative lv_table entry"] = cfg = gpu.default_config(64, 64, 32, 3)
    cfg.lv_table[517] = -1
    out["negative luma header-bit minimum"] = cfg = gpu.default_config(64, 64, 32, 3)
    cfg.header_bits_luma[0][2][40] = -5
    out["negative dual-tree header-bit minimum"] = cfg = gpu.default_config(64, 64, 32, 3)
    cfg.header_bits_luma[1][0][0] = -1
    out["negative chroma header-bit minimum"] = cfg = gpu.default_config(64, 64, 32, 3)
    cfg.header_bits_chroma[3] = -1
    out["negative lambda_rd"] = cfg = gpu.default_config(64, 64, 32, 3)
    cfg.lambda_rd = -0.5
    out["NaN lambda_rd"] = cfg = gpu.default_config(64, 64, 32, 3)
    cfg.lambda_rd = math.nan
    return out


def test_floors_prove_nothing_from_tables_that_prove_nothing(gpu):
    for what, cfg in _unproven_configs(gpu).items():
        split, cand, ang = _floors(gpu, cfg)
        assert np.array_equal(_bits(split), _bits(np.zeros(5))), what
        assert np.array_equal(_bits(cand), _bits(np.full(67, -np.inf))), what
        assert np.array_equal(_bits(ang), _bits([-np.inf])), what
        _assert_floors_equal_the_models(gpu, cfg)


def test_mfma_operand_tables_equal_the_model(gpu):
    cfg = gpu.default_config(64, 64, 32, 2)
    t8, t16 = dm.tables(8), dm.tables(16)
    f = lambda name, dtype, shape: gpu.const_field(cfg, name, dtype).reshape(shape).astype(np.int64)
    for name in ("fdct_b", "idct_b"):
        got = f(name, np.int8, (2, 32, 2, 16))
        assert np.array_equal(got[0], t8[name]) and np.array_equal(got[1], t16[name]), name
    assert np.array_equal(f("fdct16_p", np.int8, (32, 2, 8)), t16["fdct_p"])
    assert np.array_equal(f("fdct8_p", np.int8, (32, 2, 16)), t8["fdct_p"])
    assert np.array_equal(f("idct16_p", np.int8, (32, 2, 16)), t16["idct_p"])
    assert np.array_equal(f("idct8_p", np.int8, (32, 2, 8)), t8["idct_p"])
    k1 = f("idct_k1", np.int32, (2, 32))
    assert np.array_equal(k1[0], t8["k1"]) and np.array_equal(k1[1], t16["k1"])
    assert np.array_equal(f("idct16_k2", np.int32, (2, 8)), t16["k2"])
    assert np.array_equal(f("idct8_k2", np.int32, (2, 4)), t8["k2"])


def test_reciprocal_of_the_level_scale_at_every_qp(gpu):
    for qp in range(64):
        cfg = gpu.default_config(64, 64, qp, 2)
        got = (int(gpu.const_field(cfg, "lsc", np.int32)[0]), int(gpu.const_field(cfg, "div_magic", np.uint32)[0]),
               int(gpu.const_field(cfg, "div_shift", np.uint32)[0]))
        assert got == qi.reciprocal(qp), qp


def test_source_tables_equal_the_reference_data(gpu):
    """The tables the reference's source holds (tests/golden/ref_source_data.json, what tests/test_oracle.py reads)."""
    ref = json.load(open(os.path.join(HERE, "golden", "ref_source_data.json")))["tables"]
    cfg = gpu.default_config(64, 64, 32, 2)
    m64 = np.array(ref["trans_matrix_0"], np.int64).reshape(64, 32)
    dct = gpu.const_field(cfg, "dct", np.int16).reshape(4, 32, 32).astype(np.int64)
    dct_t = gpu.const_field(cfg, "dct_t", np.int16).reshape(4, 32, 32).astype(np.int64)
    for idx in range(4):
        n = 4 << idx
        want = np.zeros((32, 32), np.int64)
        want[:n, :n] = m64[::64 // n, :n][:n]          # T_N[u][x] = row u * 64 / N of the 64-point matrix
        assert np.array_equal(dct[idx], want), n
        assert np.array_equal(dct_t[idx], want.T), n
    assert np.array_equal(gpu.const_field(cfg, "fc", np.int8).astype(np.int64), np.array(ref["f_c"], np.int64))
    angle = [int(v) for v in ref["intra_angle"]]
    assert gpu.const_field(cfg, "intra_angle", np.int16).tolist() == angle
    tab = gpu.const_field(cfg, "ang_tab", np.int32).view(np.int16).reshape(67, 2)    # (low half, high half) of each dword
    for mode in range(67):
        a = angle[14 + mode] if mode >= 2 else 0      # intraPredAngle of mode 2 .. 66 (Table 24 starts at mode -14)
        # invAngle = Round(512 * 32 / intraPredAngle), away from zero at a half; 0 where there is no angle
        inv = 0 if a == 0 else (1 if a > 0 else -1) * ((512 * 32 + abs(a) // 2) // abs(a))
        want_inv = ((inv + 0x8000) & 0xFFFF) - 0x8000    # (the high half keeps 16 bits of it)
        assert tab[mode].tolist() == [a, want_inv], mode


def test_scan_table_equals_the_diagonal_scan(gpu):
    scan = gpu.const_field(gpu.default_config(64, 64, 32, 2), "scan_idx", np.uint16).reshape(4, 1024)
    for idx, n in enumerate(qi.SIZES):
        want = [y * n + x for y, x in reversed(qi.scan(n))]      # position p = 0 is the last in coding order
        assert scan[idx, :n * n].tolist() == want, n
        assert not scan[idx, n * n:].any()


@pytest.mark.parametrize("extra", [None, "quant_lambda_mul_trellis=0.02,lv_pow_dq_trellis=0.52,header_bits_dq_trellis=1.0,a=0.9"])
def test_copied_tables_equal_the_config(gpu, extra):
    for qp in QPS:
        cfg = gpu.default_config(64, 64, qp, 2, extra_params=extra)
        dq = np.array(cfg.dq_table, np.int64)
        assert np.array_equal(gpu.const_field(cfg, "ldq", np.int64), cfg.lambda_q * dq)
        assert np.array_equal(gpu.const_field(cfg, "lv", np.int64), np.array(cfg.lv_table, np.int64))
        assert np.array_equal(gpu.const_field(cfg, "hb_luma", np.int64), np.array(cfg.header_bits_luma, np.int64).ravel())
        assert np.array_equal(gpu.const_field(cfg, "hb_chroma", np.int64), np.array(cfg.header_bits_chroma, np.int64))
        for name, want in (("W", 64), ("H", 64), ("qp", qp), ("max_depth", 2), ("ctu_cols", 2), ("ctu_rows", 2)):
            assert gpu.const_field(cfg, name, np.int32).tolist() == [want], name
        assert gpu.const_field(cfg, "lambda_q", np.int64).tolist() == [cfg.lambda_q]
        assert np.array_equal(_bits(gpu.const_field(cfg, "lambda_rd", np.float32)), _bits([cfg.lambda_rd]))
        assert np.array_equal(_bits(gpu.const_field(cfg, "lambda_rd_chroma", np.float32)), _bits([cfg.lambda_rd_chroma]))


def test_const_field_refuses_what_it_cannot_answer(gpu):
    import ctypes as C
    lib = gpu.load_library()
    cfg = gpu.default_config(64, 64, 32, 2)
    buf = (C.c_uint8 * 64)()
    assert lib.wrenc_gpu_test_const_field(C.byref(cfg), b"split_floor", buf, 64) == 20
    assert lib.wrenc_gpu_test_const_field(C.byref(cfg), b"split_floor", buf, 19) == -1        # WRENC_GPU_EINVAL: short cap
    assert lib.wrenc_gpu_test_const_field(C.byref(cfg), b"no_such_member", buf, 64) == -1
    assert lib.wrenc_gpu_test_const_field(C.byref(cfg), b"", buf, 64) == -1
    assert lib.wrenc_gpu_test_const_field(None, b"split_floor", buf, 64) == -1
    assert lib.wrenc_gpu_test_const_field(C.byref(cfg), None, buf, 64) == -1
    assert lib.wrenc_gpu_test_const_field(C.byref(cfg), b"split_floor", None, 64) == -1
    with pytest.raises(gpu.WrencGpuError):
        gpu.const_field(cfg, "no_such_member", np.uint8)
