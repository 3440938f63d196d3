#!/usr/bin/env python3
"""Extract what three CPU tests check against the reference's source into tests/golden/ref_source_data.json, so that
the tests need nothing outside this repository.  Data only; run once where a checkout of the reference exists:

    python tests/golden/make_ref_source_data.py REFERENCE_CHECKOUT

tables        (tests/test_oracle.py) TRANS_MATRIX_0_ (transformer.rs:934), INTRA_ANGLE_TABLE / F_C / F_G
              (common.rs:145 / 153 / 188), LEVEL_SCALE (quantizer.rs), q_state_trans_table (encoder_context.rs:339),
              as the numbers the reference's source holds
ps_defaults   (tests/test_bitstream.py) for every default headers.cpp relies on (PS_DEFAULTS below), the 1-based
              lines of the reference's source file at which it was found; the script fails if one is not found"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_source_data.json")

# The parameter-set writer (wrenc_amd/csrc/host/headers.cpp) writes from the defaults of the reference's constructors.
# Every default that decides a written value or a taken branch, by the reference's source file that sets it.
PS_DEFAULTS = {
    "main.rs": ["VideoParameterSet::new(8,", "SequenceParameterSet::new(1, 8,", "PictureParameterSet::new(1, &sps",
                "write_byte_stream_nal_unit_bits(1, NALUnitType::VPS_NUT, 0", "write_byte_stream_nal_unit_bits(9, NALUnitType::SPS_NUT, 0",
                "write_byte_stream_nal_unit_bits(9, NALUnitType::PPS_NUT, 0", "let nuh_layer_id = 9;", "NALUnitType::IDR_W_RADL"],
    "vps.rs": ["max_layers: 1,", "max_sublayers: 1,", "VpsLayer::new(9)", "each_layer_is_an_ols: false,", "num_ptls: 1,",
               "default_ptl_dpb_hrd_max_tid_flag: true,", "general_timing_hrd_parameters: None,", "ptl_max_tids: vec![1, 2],",
               "extension_data: vec![],"],
    "ptl.rs": ["general_level_idc: 0,", "general_profile_idc: 0,", "general_constraints_info: None,", "ptl_num_sub_profiles: 0,"],
    "dpb.rs": ["max_tid: 1,", "max_dec_pic_buffering: 8,", "max_num_reorder_pics: 4,", "max_latency_increase: 1,"],
    "reference_picture.rs": ["num_ref_entries: 3,", "abs_delta_poc_st: vec![0, 2, 3],", "strp_entry_sign_flag: vec![lx == 0; 3],",
                             "num_ref_pic_list: 1,", "st_ref_pic_flag: vec![true; 3],"],
    "sps.rs": ["max_sublayers: 1,", "chroma_format: ChromaFormat::YCbCr420,", "log2_ctu_size: 5,", "ptl_dpb_hrd_params_present_flag: true,",
               "conformance_window: None,", "subpic_info: None,", "bitdepth: 8,", "log2_max_pic_order_cnt_lsb: 4,",
               "log2_min_luma_coding_block_size: 2,", "transform_skip_enabled_flag: true,", "log2_transform_skip_max_size: 5,",
               "bdpcm_enabled_flag: false,", "mts_enabled_flag: true,", "explicit_mts_intra_enabled_flag: true,",
               "explicit_mts_inter_enabled_flag: true,", "lfnst_enabled_flag: false,", "joint_cbcr_enabled_flag: false,",
               "same_qp_table_for_chroma_flag: true,", "QpTable::new(bit_depth, 63, 0)", "sao_enabled_flag: false,",
               "alf_enabled_flag: false,", "idr_rpl_present_flag: false,", "rpl1_same_as_rpl0_flag: false,",
               "six_minus_max_num_merge_cand: 0,", "log2_parallel_merge_level: 2,", "cclm_enabled_flag: true,",
               "palette_enabled_flag: false,", "min_qp_prime_ts: 0,", "ibc_enabled_flag: false,", "ladf_parameters: None,",
               "dep_quant_enabled_flag: true,", "sign_data_hiding_enabled_flag: false,", "vui_parameters_present_flag: false,"],
    "partition.rs": ["log2_diff_min_qt_min_cb_intra_slice_luma: 0,", "max_mtt_hierarchy_depth_intra_slice_luma: 0,",
                     "qtbtt_dual_tree_intra_flag: false,", "max_mtt_hierarchy_depth_inter_slice: 0,"],
    "pps.rs": ["no_pic_partition_flag: true,", "cabac_init_present_flag: false,", "num_ref_idx_default_active: [3, 3],",
               "qp.max(26)", "cu_qp_delta_enabled_flag: true,", "chroma_tool_offsets_present_flag: false,",
               "deblocking_filter_control_present_flag: true,", "deblocking_filter_override_enabled_flag: false,",
               "deblocking_filter_disabled_flag: true,", "picture_header_extension_present_flag: false,"],
    "picture_header.rs": ["gdr_or_irap_pic_flag: true,", "non_ref_pic_flag: false,", "gdr_pic_flag: false,", "inter_slice_allowed_flag: !intra,",
                          "pic_order_cnt_lsb: poc & 0b1111,", "cu_qp_delta_subdiv_intra_slice: 0,"],
    "slice_header.rs": ["ph_in_sh: None,", "slice_type: SliceType::I,", "no_output_of_prior_pics_flag: false,", "qp - ectx.slice_qp_y",
                        "dep_quant_used_flag: true,"],
    "nal.rs": ["let header_bytes: [u8; 3] = [0, 0, 0];", "let start_code_prefix_one_3bytes: [u8; 3] = [0, 0, 1];",
               "while idx + 3 < bytes.len()", "bytes[idx + 2] <= 3"],
}


def _ints(text):
    return [int(x) for x in re.findall(r"-?\d+", text)]


def tables(src):
    txt = open(os.path.join(src, "transformer.rs")).read()
    i = txt.index("const TRANS_MATRIX_0_")
    body = txt[i:txt.index("lazy_static!", i)]
    body = body[body.index("= [") + 2:]
    trans = _ints(body)[:64 * 32]
    txt = open(os.path.join(src, "common.rs")).read()

    def rs_table(name):
        i = txt.index("pub const %s" % name)
        i = txt.index("= [", i)
        return _ints(txt[i:txt.index("];", i)])

    ls = open(os.path.join(src, "quantizer.rs")).read()
    i = ls.index("=", ls.index("const LEVEL_SCALE"))
    ec = open(os.path.join(src, "encoder_context.rs")).read()
    j = ec.index("q_state_trans_table: [[0")
    return {"trans_matrix_0": trans, "intra_angle": rs_table("INTRA_ANGLE_TABLE"), "f_c": rs_table("F_C"),
            "f_g": rs_table("F_G"), "level_scale": _ints(ls[i:ls.index("];", i)])[:6],
            "q_state_trans": _ints(ec[j + len("q_state_trans_table:"):ec.index("]],", j)])}


def ps_defaults(src):
    out = {}
    for name, items in PS_DEFAULTS.items():
        lines = open(os.path.join(src, name)).read().split("\n")
        out[name] = []
        for item in items:
            found = [n + 1 for n, line in enumerate(lines) if item in line]
            if not found:
                raise SystemExit("%s no longer says %r" % (name, item))
            out[name].append(found)
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    src = os.path.join(sys.argv[1], "src")
    out = {"tables": tables(src), "ps_defaults": ps_defaults(src)}
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
