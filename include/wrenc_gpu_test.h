/* wrenc_gpu_test.h -- test entries of libwrenc_gpu.so that run device code on data of their own: the building blocks of
 * the search on blocks the caller brings, and device passes on pictures that are no slot of a context.  For the test
 * suite and the measurement tools; an integrator needs wrenc_gpu.h alone.  (The test hooks that only read or set a
 * context's state -- wrenc_gpu_test_plan, _test_load_record, ... -- are declared there, next to what they belong to.) */
#ifndef WRENC_GPU_TEST_H
#define WRENC_GPU_TEST_H

#include "wrenc_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* wrenc_gpu_download_metrics' kernel on two arbitrary pictures of the context's size (host planes), no search involved;
 * ssim_map[p] (may be NULL) receives the plane's per-window f32 values in raster order. */
int wrenc_gpu_test_metrics(wrenc_gpu_ctx* ctx, const uint8_t* const org[3], const uint8_t* const rec[3],
                           wrenc_gpu_metrics* out, float* const ssim_map[3]);

/* wrenc_gpu_download_hashes' kernels on an arbitrary picture of the context's size (host planes Y, Cb, Cr), no search involved. */
int wrenc_gpu_test_hash(wrenc_gpu_ctx* ctx, const uint8_t* const rec[3], int hash_type, wrenc_picture_hash* out);

/* Test entry: the dependent quantiser's head proof decides "this coefficient ends the region" and "quotient >= 2" by range
 * tests whose bounds the host derives per context (QP) and block size; this holds them against the device's own
 * formulas over every 16-bit coefficient, 4 block sizes, DC and other positions.  counts[0]: coefficients a range admits
 * that the formula does not (must be 0: results depend on it); counts[1]: the opposite (allowed, costs speed; 0
 * expected); counts[2]: quotient differences (must be 0); counts[3]: differences of the two alpha formulas (must be 0).
 * ranges (may be NULL): the 4 x 6 bounds.  Waits for the device. */
int wrenc_gpu_test_head_ranges(wrenc_gpu_ctx* ctx, int counts[4], int ranges[24]);
/* Test entry: which reference segments of a block are available (below-left, left, corner, above, above-right) comes
 * from a table of the block's place in its CTU plus the picture's edges; this counts the blocks -- every CTU of the
 * context's picture, every size and position, luma and chroma spacing -- at which that differs from the reference's rules
 * (ctu.rs:2083-2188, encoder_context.rs:918-956) evaluated directly.  Must be 0.  Waits for the device. */
int wrenc_gpu_test_avail_tab(wrenc_gpu_ctx* ctx, int* differences);

/* ---- kernel-level entry points (parity tests of the building blocks) ----
 * Each runs `count` independent square blocks of side 1<<log2n (2..5), row-major
 * int16, host pointers.  Same arithmetic as the picture path.
 * Precondition of the 32x32 forward transform (log2n = 5, and wrenc_gpu_test_fwd_dct32 with use_mfma = 1): every
 * residual lies within +-255, as original minus prediction always does -- the i8-MFMA code splits it into two
 * base-256 digits.  Inputs outside that range return WRENC_GPU_EINVAL (nothing is computed). */
int wrenc_gpu_test_fwd_dct(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int count,
                           int16_t* coef);                              /* transformer.rs:2040 */
/* The 32x32 forward transform of `count` blocks (residuals within +-255), by the v_dot2 code the search kernel used
 * until round 2 (use_mfma = 0) or by the i8-MFMA version it runs now (use_mfma = 1; wrenc_amd/csrc/dev_transform.h); the kernel repeats the
 * transform `reps` times per block and *kernel_ms receives its HIP-event duration: parity gate and micro-benchmark
 * of north_star's MFMA question in one entry point (transformer.rs:2040-2378). */
int wrenc_gpu_test_fwd_dct32(wrenc_gpu_ctx* ctx, const int16_t* res, int count, int16_t* coef,
                             int use_mfma, int reps, float* kernel_ms);
/* The same for the inverse 32x32 transform (transformer.rs:2380-2737): `count` dequantised blocks in, residuals out;
 * use_mfma = 1 is what the search kernel runs (four v_mfma_i32_32x32x32_i8), 0 the v_dot2 version it replaced. */
int wrenc_gpu_test_inv_dct32(wrenc_gpu_ctx* ctx, const int16_t* deq, int count, int16_t* res,
                             int use_mfma, int reps, float* kernel_ms);
/* The packed quantiser of the 8x8 / 16x16 leaf searches (quantize_pk, wrenc_amd/csrc/dev_quant.h): `n_packs` packs of
 * `nc` candidates (log2n = 3: nc 1..3, log2n = 4: nc 1..2); a pack is nc luma blocks of side 1 << log2n, then per candidate
 * its Cb and Cr block of half that side, all row-major int16 coefficients back to back (nc * 1.5 * 4^log2n values).
 * levels: the same layout; level_cost: per pack and candidate {luma block, chroma pair} (block_splitter.rs:436-458). */
int wrenc_gpu_test_quantize_pk(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int nc, int n_packs, int16_t* levels,
                               int64_t* level_cost);
int wrenc_gpu_test_inv_dct(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int count,
                           int16_t* res);                               /* transformer.rs:2380 */
int wrenc_gpu_test_quantize(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int count,
                            int16_t* levels, int64_t* level_cost);      /* quantizer.rs:519 +
                                                                           block_splitter.rs:415-460 */
/* The same quantiser as the packed 4x4 leaf search runs it: `count` 4x4 blocks, up to four per wavefront at once
 * (quantizer.rs:519 + block_splitter.rs:415-460; wrenc_amd/csrc/dev_quant.h quantize_p16). */
int wrenc_gpu_test_quantize_p16(wrenc_gpu_ctx* ctx, const int16_t* coef, int count, int16_t* levels,
                                int64_t* level_cost);
int wrenc_gpu_test_dequantize(wrenc_gpu_ctx* ctx, const int16_t* levels, int log2n, int count,
                              int16_t* deq);                            /* quantizer.rs:761 */
/* The same device functions as the search calls them: on GROUPS of blocks.  Each entry runs `count` groups, one wavefront
 * per group; a group is `nb` blocks of side 1 << log2n back to back, [blk][y][x] row-major int16, and the outputs have the
 * same layout.  The one-block entries above are these with nb = 1, o1 = 0 (one kernel per device function).
 *   _quantize_nb: nb = 1 (a luma block) or 2 (the Cb + Cr pair of a CU: quantize_solo's two-block path) at r1[0 ..];
 *       level_cost[g]: the summed level cost of group g's blocks, any_level[g]: 1 where the device function reported a
 *       non-zero level in the group (what decides whether its caller dequantises and inverts at all), else 0; may be null.
 *       Its own overflow word, WRENC_GPU_ELEVEL and the clean next call exactly as wrenc_gpu_test_quantize.
 *   _fwd_dct_nb / _inv_dct_nb / _dequantize_nb: the group's blocks sit at r1[o1 ..] (i16 units), where the search puts a
 *       pack's chroma behind its luma; the inverse transform's input goes to r2 transposed block by block, and the
 *       dequantiser's output is read back from there the same way.
 * Refused with WRENC_GPU_EINVAL before anything is launched -- the device functions are not written for these, or the
 * group would leave the wavefront's buffers (r1 and r2: 1024 int16 each): nb < 1, nb > 2 for the quantiser; log2n = 5
 * with nb > 1; o1 odd or negative; o1 + nb * 4^log2n > 1024; nb * 4^log2n > 1024; and a 32x32 residual outside +-255
 * for the forward transform. */
int wrenc_gpu_test_quantize_nb(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int nb, int count, int16_t* levels,
                               int64_t* level_cost, int32_t* any_level);
int wrenc_gpu_test_fwd_dct_nb(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int nb, int o1, int count, int16_t* coef);
int wrenc_gpu_test_inv_dct_nb(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int nb, int o1, int count, int16_t* res);
int wrenc_gpu_test_dequantize_nb(wrenc_gpu_ctx* ctx, const int16_t* levels, int log2n, int nb, int o1, int count,
                                 int16_t* deq);
/* The 16x16 transforms (log2n = 4) run as i8 MFMAs in the search (wrenc_amd/csrc/dev_transform.h fwd_dct_mfma /
 * inv_dct_mfma): exact for forward residuals within +-255 and any int16 inverse input, with the group at an o1 that is a
 * multiple of 8 -- all of which the search has by construction.  The same code exists for 8x8 (log2n = 3), where the
 * search keeps the v_dot2 templates.  wrenc_gpu_test_fwd_dct(_nb) and _inv_dct(_nb) inspect the group on the host before
 * the launch: a 16x16 forward group with a residual outside +-255, or a 16x16 group at another o1, runs the retained
 * v_dot2 templates and still returns the reference's answer; every other group runs the code the search runs.  The two
 * entries below choose the arm themselves at log2n = 3 or 4, for the parity tests and tools/dct_bench.py: arguments of
 * _fwd_dct_nb / _inv_dct_nb, then use_mfma (1: the MFMA version, WRENC_GPU_EINVAL where the group does not meet the
 * preconditions above; 0: the v_dot2 templates), reps >= 1 (the transform of the same group repeated in place of
 * itself; the last repetition's result comes back) and kernel_ms (may be null: HIP-event duration of the kernel). */
int wrenc_gpu_test_fwd_dct_mfma(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int nb, int o1, int count, int16_t* coef,
                                int use_mfma, int reps, float* kernel_ms);
int wrenc_gpu_test_inv_dct_mfma(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int nb, int o1, int count, int16_t* res,
                                int use_mfma, int reps, float* kernel_ms);
/* The register transforms of the search's 4x4 passes (wrenc_amd/csrc/dev_transform.h fwd_dct4_reg / inv_dct4_reg): `count`
 * 4x4 blocks, row-major int16, four per wavefront with one sample per lane, a last wavefront of fewer included.
 * fwd: residuals -> coefficients (transformer.rs:2040).  inv: LEVELS -> residuals, dequantised in the lane at the
 * context's QP (quantizer.rs:761) and inverted (transformer.rs:2380). */
int wrenc_gpu_test_fwd_dct4_reg(wrenc_gpu_ctx* ctx, const int16_t* res, int count, int16_t* coef);
int wrenc_gpu_test_inv_dct4_reg(wrenc_gpu_ctx* ctx, const int16_t* levels, int count, int16_t* res);

/* The row reconstruction of the full candidates and the 16x16 packs (wrenc_amd/csrc/dev_predict.h recon_row4): `count`
 * rows of four samples, one per lane.  pred, org: 4 bytes per row; res: 4 int16 per row, any value.  rec: the four
 * reconstructed bytes of each row, clamp((int16)(pred + res)); ssd[row]: the row's squared error against org. */
int wrenc_gpu_test_recon_rows(wrenc_gpu_ctx* ctx, const uint8_t* pred, const int16_t* res, const uint8_t* org, int count,
                              uint8_t* rec, uint32_t* ssd);

/* Intra prediction of single blocks (intra_predictor.rs:56-144: reference-sample build :146-353, PLANAR
 * :759-1146, DC :1148-1285, ANGULAR 2..66 :1287-1602, PDPC :355-757, CCLM :1604-2055) in the environment of
 * given reconstruction planes of the context's picture size.  items: n_items x 5 int32 {x, y (luma, picture
 * coordinates, multiples of the size), log2 luma size 2..5, comp (0 = luma block, 1 = Cb+Cr pair of the block,
 * log2 size >= 3, 2 = the 4x4 luma block through the row-parallel predictor of the packed 4x4 leaf search, log2 size 2),
 * mode (0..66, or 81..83 for comp 1)}.  out: the predicted samples, item after item (luma
 * n x n; pair: Cb (n/2)^2 then Cr (n/2)^2); out_bytes must equal their total.
 * comp 4 / 5 / 6: not a prediction but a SAD LIST of the search (get_intra_pred_aux_cost, block_splitter.rs:64-108, of each
 * entry) over the luma block / the chroma pair (log2 size >= 3) / both, against the block's own samples in the planes as
 * originals: mode = first mode (2..66) | entries (1..16) << 8 | stride (1..64) << 16, entry j = first mode + j * stride (an
 * entry beyond 66 is not evaluated and reads 0).  comp 7 (log2 size >= 3, mode 0): the CCLM SAD list of the chroma pair,
 * entries LT_CCLM, T_CCLM, L_CCLM (get_chroma_intra_pred_aux_cost, :476-522).  A list item's output is 16 uint32 (64 bytes):
 * the SAD of entry j at index j.
 * comp 8 / 9: the search's FULL-candidate predictor on the luma block / the Cb+Cr pair (log2 size >= 3; mode as for comp 0 /
 * 1) into the recon tile, with the block's own samples in the planes as originals (staged as the search stages them).
 * comp 10 (log2 size 3): the luma blocks of an 8x8 pack of 1..3 candidates, predicted side by side into the pack's LDS
 * park; comp 11 (log2 size 4): a 16x16 pack of 1..2 candidates, luma block and chroma pair, into its park; their mode =
 * m0 | m1 << 8 | m2 << 16 | candidates << 24, each m 0..66 or 255 (a candidate that is not evaluated and rides along as
 * zeros).  Output of 8..11: the prediction bytes read back from the destination (comp 10: [candidate][64]; comp 11: luma
 * [candidate][256], then chroma [candidate][Cb | Cr][64]), then as many int16 residuals (original - prediction) in the
 * same order: 3 bytes per sample. */
int wrenc_gpu_test_predict(wrenc_gpu_ctx* ctx, const uint8_t* rec_y, const uint8_t* rec_cb,
                           const uint8_t* rec_cr, int n_items, const int32_t* items, uint8_t* out,
                           size_t out_bytes);
/* Host only, needs no context and no device: where the output of each item of such a call on a width x height picture
 * starts -- offsets[i] for item i, offsets[n_items] = the out_bytes the call takes (offsets: n_items + 1 values).
 * WRENC_GPU_EINVAL at the first item wrenc_gpu_test_predict would refuse (offsets then holds no layout). */
int wrenc_gpu_test_predict_layout(int width, int height, int n_items, const int32_t* items, size_t* offsets);

/* Host only, needs no context and no device: the constant block the device would be given for `cfg` (wrenc_amd/csrc/dev_const.h,
 * DevConst) is built, and the bytes of its member `name` ("split_floor", "scan_idx", "fdct_b", ...: the member's name, arrays
 * as they lie in memory) are copied to `out`.  Returns their count; WRENC_GPU_EINVAL for a NULL argument, a name the block
 * does not have, a `cap` smaller than the member, or a rate model wrenc_gpu_create refuses. */
int wrenc_gpu_test_const_field(const wrenc_gpu_config* cfg, const char* name, void* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* WRENC_GPU_TEST_H */
