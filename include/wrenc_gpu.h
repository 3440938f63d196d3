/* wrenc_gpu.h -- C ABI of the MI355X (gfx950) all-intra RD-search path.
 *
 * Drop-in boundary for the ONE hot path of hjmkt/wrenc: the per-CTU RD search
 * (BlockSplitter::split_ct and everything it calls) plus the per-TU final pass.
 * The reference has no FFI; the seam is two call sites (paths relative to the
 * reference's src/):
 *   - search:     BlockSplitter::new + split_ct            ctu_encoder.rs:53-54
 *   - final pass: predict/transform/quantize/dequantize/
 *                 inverse_transform/recon per TU component  ctu_encoder.rs:1421-1461
 * Both are entered once per CTU from CtuEncoder::encode (ctu_encoder.rs:33) inside
 * SliceEncoder::encode's raster CTU loop (slice_encoder.rs:352-379).  Nothing in
 * them reads CABAC state, so this ABI is picture-granular: the device runs the
 * search of whole pictures (CTU wavefront inside a picture, many pictures in
 * flight) and hands back what the host entropy coder needs.
 *
 * Plain C: pointers and sizes only.  All functions return 0 on success or a
 * negative wrenc_gpu_status; wrenc_gpu_last_error() gives the text.  Nothing
 * aborts across this boundary (the reference panics or exit(0)s, main.rs:127-133).
 * One context per GPU, one host thread per context.
 */
#ifndef WRENC_GPU_H
#define WRENC_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "wrenc_format.h"
#include "wrenc_hash.h"
#include "wrenc_ratecurve.h"
#include "wrenc_distcurve.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wrenc_gpu_ctx wrenc_gpu_ctx;

enum wrenc_gpu_status {
    WRENC_GPU_OK = 0,
    WRENC_GPU_EINVAL = -1,   /* bad argument (size not a multiple of 32: picture.rs:178-181) */
    WRENC_GPU_ENODEV = -2,   /* no usable HIP device / wrong architecture */
    WRENC_GPU_ENOMEM = -3,
    WRENC_GPU_EHIP = -4,     /* HIP runtime error, see last_error */
    WRENC_GPU_ESTATE = -5,   /* slot not submitted / still in flight */
    WRENC_GPU_ELEVEL = -6    /* a quantised level reached 1024 (reference would panic,
                                block_splitter.rs:453).  Raised where a coefficient's quotient
                                qd = |(tc << sh) - off| / lsc is >= 2044, as the reference does in every
                                state.  At qd = 2043 the reference panics only if its search reaches the
                                position in a state with delta 1 (some non-zero coefficient later in scan
                                order); the device costs both delta classes at every position and raises
                                the error there regardless -- one step early for a position reached in
                                states 0 / 1 only, never late.  The DC position is exempt: its level is
                                qd / 2 in both delta classes, so 2043 quantises there on both sides */
};
/* WRENC_GPU_ELEVEL and the internal WRENC_GPU_EHIP "a team member never reached a meeting point" are reported by sync /
 * download / download_compact and are STICKY, like the reference's panic: the pictures of the call that raised them --
 * and of every call in flight next to it -- are undefined (a team that times out stops storing, its CTU and everything
 * that depends on it are garbage; the slots' zero-block bookkeeping no longer matches their level planes), every later
 * sync / download of the context fails the same way, and the context must be destroyed.  The wrenc_gpu_test_* entries
 * keep a word of their own and never poison a context: wrenc_gpu_test_quantize / _quantize_p16 / _quantize_pk return
 * WRENC_GPU_ELEVEL from the call whose blocks raised it (the levels and costs they wrote are then those of table
 * indices clamped to 1023, not the reference's) and clear the word on every return path, so the next call on the
 * context starts clean.
 * Only a candidate that is evaluated can raise WRENC_GPU_ELEVEL.  The wave schedule does not evaluate what cannot change
 * the result: the children of a split that has already lost, and, in a 4x4 luma leaf, the SAD search's candidates where
 * their header bits alone already cost as much as the best of {planar, DC}.  A candidate whose levels would have reached
 * 1024 and that is skipped this way raises nothing; the team schedule and the trace build evaluate everything. */

/* Resolved configuration.  The RD-model constants are resolved on the host
 * (libm pow/powf, exactly as block_splitter.rs:29-53,187-375 and
 * quantizer.rs:16-25,650-683 do) and passed as tables so that device code does
 * no transcendental math.  wrenc_gpu_default_config() fills every table from the
 * reference's defaults for a given QP. */
typedef struct wrenc_gpu_config {
    int32_t width;            /* luma, multiple of 32 (CLI --output-size, main.rs:176-191) */
    int32_t height;
    int32_t qp;               /* CLI --qp (main.rs:193-198), 26 when absent (ctu.rs:382) */
    int32_t max_split_depth;  /* CLI --max-split-depth 0..3 (main.rs:108-109) */
    int32_t device;           /* HIP device ordinal */
    int32_t n_slots;          /* pictures resident on the device at once (>= 1) */
    int64_t lv_table[1024];   /* lv_dq_trellis_table, block_splitter.rs:51-52 */
    int64_t dq_table[1024];   /* quantizer.rs:20-21 */
    int64_t lambda_q;         /* quantizer.rs:683 */
    float lambda_rd;          /* block_splitter.rs:472 */
    float lambda_rd_chroma;   /* block_splitter.rs:775-778 (extra-param "a") */
    /* header bits ((x*16384.0) as i64), block_splitter.rs:377-406.
     * [tree: 0 SINGLE_TREE, 1 DUAL_TREE_LUMA]
     * [cclm class: 0 not CCLM, 1..3 = cclm_mode_idx 0..2]
     * [mode class: 0 planar, 1..5 = mpm_idx 0..4, 6..66 = mpm_remainder 0..60] */
    int64_t header_bits_luma[2][4][67];
    /* block_splitter.rs:695-712. [0 not CCLM, 1..3 = cclm_mode_idx 0..2] */
    int64_t header_bits_chroma[4];
} wrenc_gpu_config;

/* Per-picture result (caller-allocated; any pointer may be NULL to skip it).
 * Replaces what the reference keeps in its Rust object graph:
 *   CT tree ctu.rs:1794-1821, CodingUnit.intra_pred_mode ctu.rs:1241,
 *   TransformUnit.cu_intra_pred_mode ctu.rs:361,
 *   TransformUnit.quantized_transformed_coeffs ctu.rs:340 (TransCoeffLevel,
 *   written by the final pass), Tile.reconst_pixels tile.rs:17. */
typedef struct wrenc_gpu_picture {
    uint8_t* rec_y;         /* width*height */
    uint8_t* rec_cb;        /* (width/2)*(height/2) */
    uint8_t* rec_cr;
    int16_t* lev_y;         /* TransCoeffLevel planes, each TB at its own position */
    int16_t* lev_cb;
    int16_t* lev_cr;
    uint8_t* cu_log2_size;  /* (width/4)*(height/4): log2 size of the luma CU covering the 4x4 */
    uint8_t* luma_mode;     /* (width/4)*(height/4): intra_pred_mode[0] of that CU */
    uint8_t* chroma_mode;   /* (width/8)*(height/8): chroma prediction mode of the chroma block
                               (TU array: 0..66, or 81 LT_CCLM / 82 L_CCLM / 83 T_CCLM) */
    float* ctu_cost;        /* one f32 per CTU: value split_ct returns at ctu_encoder.rs:54 */
} wrenc_gpu_picture;

/* Fill cfg (all tables) from the reference's default constants for this QP. */
int wrenc_gpu_default_config(wrenc_gpu_config* cfg, int width, int height, int qp,
                             int max_split_depth);

/* Re-resolve cfg's tables with the reference's --extra-params string "K1=V1,K2=V2" (main.rs:202-217):
 * the RD-model tuning knobs of block_splitter.rs:21-53,187-375,594-693,775 and quantizer.rs:16-19,650-683.
 * Keys of the code path that is live (dependent quantisation + trellis) take effect; other keys are accepted
 * and ignored, as in the reference.  WRENC_GPU_EINVAL (text in wrenc_gpu_last_error(NULL)) for an item that
 * is not KEY=VALUE or a live key whose value is not a number.  NULL or "" gives the defaults again. */
int wrenc_gpu_config_extra_params(wrenc_gpu_config* cfg, const char* extra_params);

/* WRENC_GPU_EINVAL for a geometry that is not whole CTUs, a QP outside 0..63 -- and for a quantiser rate model the device's
 * arithmetic does not cover: the trellis keeps its path costs in 32 bits, exact while 128 * 65535 + lambda_q * dq_table[i]
 * < 2^25 for every i.  That holds for the reference's defaults at every QP and for tuned models near them; it does not
 * for values such as quant_lv_pow = 2.5 or quant_qp_div_trellis = 1.5, which are refused here (the reference computes those
 * products in i64) instead of being searched with other results.  WRENC_GPU_ENODEV without an MI355X. */
int wrenc_gpu_create(const wrenc_gpu_config* cfg, wrenc_gpu_ctx** out);
void wrenc_gpu_destroy(wrenc_gpu_ctx* ctx);
const char* wrenc_gpu_last_error(const wrenc_gpu_ctx* ctx); /* ctx may be NULL: create errors */

/* Copy one picture's planes (host memory, given strides in bytes) into slot `slot`
 * (asynchronous on the context's copy stream, behind any search still reading the slot;
 * the host buffers must stay valid until wrenc_gpu_sync or wrenc_gpu_download of that
 * slot). Uploads overlap the search of other slots.  Replaces main.rs:318-350 +
 * picture.rs:169-196. */
int wrenc_gpu_upload(wrenc_gpu_ctx* ctx, int slot, const uint8_t* y, const uint8_t* cb,
                     const uint8_t* cr, size_t stride_y, size_t stride_c);

/* Pictures of any even size.  The context's width x height stay the CODED size, whole 32x32 CTUs; a visible size says
 * that the caller's pictures are vis_w x vis_h: wrenc_gpu_upload then takes planes of vis_w x vis_h and vis_w/2 x vis_h/2
 * (the stride checks use those widths), copies them into the top-left corner of the slot's planes and a device kernel
 * behind the copies replicates each plane's last visible column and row into the margin,
 *     org(x, y) = org(min(x, vis - 1), min(y, vis - 1)) per plane,
 * so the margin never crosses the bus.  Search, final pass, token pass, compact pass and complexity pass see an ordinary
 * picture of the coded size: wrenc_gpu_download, _download_compact and _download_tokens keep returning CODED-size maps,
 * levels and reconstruction (the caller crops the reconstruction), and wrenc_gpu_download_complexity stays over the coded
 * picture, margin included -- the margin is coded and costs bits, and those figures are rate control's estimate of bits.
 * wrenc_gpu_download_metrics reports the visible rectangle only (below).  The stream tells a decoder the visible size
 * by a conformance window: wrenc_bs_write_parameter_sets_window (wrenc_bitstream_window.h).
 * vis_w and vis_h: even, at least 16 (each chroma plane still holds one SSIM window), and the context's size exactly
 * the round-up of each to a multiple of 32; else WRENC_GPU_EINVAL.  WRENC_GPU_ESTATE once any slot of the context has
 * been uploaded into.  Passing the coded size itself puts the context back to the plain behaviour; a context on which
 * no visible size is set launches nothing it did not launch before. */
int wrenc_gpu_set_visible_size(wrenc_gpu_ctx* ctx, int vis_w, int vis_h);
int wrenc_gpu_visible_size(const wrenc_gpu_ctx* ctx, int* w, int* h); /* the coded size when none is set */
/* Scaling on the device.  A source size says that the caller's pictures are src_w x src_h and are resampled to the
 * context's visible size (the coded size unless one is set): wrenc_gpu_upload then takes planes of src_w x src_h and
 * src_w/2 x src_h/2 (the stride checks use those widths; wrenc_gpu_encode_picture follows), copies them into staging planes
 * on the device -- one set per context; copies, scaler, pad and retile of every upload run in order on one stream -- and a
 * kernel behind the copies writes the visible rectangle of the slot's planes; the margin of a padded context is filled
 * from the scaled picture as before.  The filter is defined in wrenc_scale.h, in integers: separable Catmull-Rom,
 * stretched by the ratio when shrinking, centre-aligned samples, edge samples repeated; the device meets it bit for bit.
 * Everything behind the upload sees the scaled picture as the slot's originals: search, final pass, token and compact
 * pass, wrenc_gpu_download_complexity, and wrenc_gpu_download_metrics -- which therefore measures the codec against the
 * SCALED originals, not the scaling itself.
 * src_w and src_h: even, at least 16, and per dimension within a factor of 4 of the visible size, in either direction;
 * else WRENC_GPU_EINVAL.  WRENC_GPU_ESTATE once any slot of the context has been uploaded into.  Passing the visible size
 * itself puts the context back to the plain behaviour; a context on which no source size is set launches and allocates
 * nothing it did not before.  While a source size is set wrenc_gpu_set_visible_size returns WRENC_GPU_ESTATE: set the
 * visible size first, then the source size. */
int wrenc_gpu_set_source_size(wrenc_gpu_ctx* ctx, int src_w, int src_h);
int wrenc_gpu_source_size(const wrenc_gpu_ctx* ctx, int* w, int* h); /* the visible size when none is set */
/* Host only: the taps of output sample o of one axis n_in -> n_out (wrenc_scale_taps of wrenc_scale.h): *first the input
 * index of coef[0] -- it may lie outside [0, n_in - 1], where the edge sample is read -- and *n_taps their number (at most
 * 16); the coefficients sum to 4096.  WRENC_GPU_EINVAL outside the limits (n_out <= 4 n_in, n_in <= 4 n_out, both 1 ..
 * 16384, 0 <= o < n_out) or for a null pointer. */
int wrenc_gpu_scale_taps(int n_in, int n_out, int o, int* first, int* n_taps, int16_t coef[17]);
/* Source formats.  A source format says how the caller's pictures lie in memory (wrenc_format.h names the six: yuv420p = 0
 * the plain behaviour, nv12, yuv420p10le, p010le, yuv422p, yuv422p10le) and wrenc_gpu_upload_planes takes them as they
 * are: it copies the RAW planes -- 16-bit words, interleaved CbCr, 4:2:2 rows; a 10-bit picture crosses the bus once -- into
 * raw staging planes on the device (one set per context, pitch a multiple of 32 bytes; allocated when the format is set, or
 * at the first upload when a size was set after it: WRENC_GPU_ENOMEM from that call when it fails) and a kernel behind the
 * copies writes planar 8-bit 4:2:0 by the rules of wrenc_format.h, in integers, bit for bit: into the scaler's staging
 * planes when a source size is set -- conversion comes BEFORE scaling -- else into the visible rectangle of the slot's
 * planes.  Scaler, padding and everything behind the upload then run as always, on the converted picture: search and
 * parameter sets stay 8-bit 4:2:0, and wrenc_gpu_download_metrics measures the codec against the CONVERTED (and scaled)
 * originals, not the conversion.  The planes are those of the context's source size (wrenc_gpu_source_size).
 * wrenc_gpu_set_source_format: any order with wrenc_gpu_set_visible_size / _set_source_size.  WRENC_GPU_EINVAL for an
 * unknown format, WRENC_GPU_ESTATE once any slot of the context has been uploaded into.  Format 0 puts the context back to
 * the plain behaviour; a context on which no format is set launches and allocates nothing it did not before.
 * wrenc_gpu_upload_planes: plane[p] and stride_bytes[p] as wrenc_gpu_format_layout numbers the planes; a two-plane format
 * does not read plane[2] and stride_bytes[2].  With format 0 it is wrenc_gpu_upload (which has one stride for both chroma
 * planes: WRENC_GPU_EINVAL when stride_bytes[1] != stride_bytes[2]).  WRENC_GPU_EINVAL for a null plane that the format
 * reads, a stride smaller than the plane's row_bytes, and an odd pointer or odd stride with a 16-bit format.  The host
 * buffers must stay valid as for wrenc_gpu_upload.
 * While the format is not 0, wrenc_gpu_upload and wrenc_gpu_encode_picture return WRENC_GPU_ESTATE: their uint8_t*
 * signature cannot say what is meant. */
int wrenc_gpu_set_source_format(wrenc_gpu_ctx* ctx, int format);
int wrenc_gpu_source_format(const wrenc_gpu_ctx* ctx); /* the id; 0 when none is set */
int wrenc_gpu_upload_planes(wrenc_gpu_ctx* ctx, int slot, const void* const plane[3], const size_t stride_bytes[3]);
/* Host only, callable without a device.  The id of a format's name (as ffmpeg names it) or WRENC_GPU_EINVAL; the name of an
 * id or NULL; and the layout of a tightly packed w x h frame as it lies in a raw file: planes, bytes per sample, per plane
 * row_bytes, rows and offset, and frame_bytes.  WRENC_GPU_EINVAL for an unknown format, an odd w or h, w or h below 16, or
 * a null pointer. */
int wrenc_gpu_format_from_name(const char* name);
const char* wrenc_gpu_format_name(int format);
int wrenc_gpu_format_layout(int format, int w, int h, struct wrenc_gpu_format_layout* out);
/* RGB sources.  wrenc_rgb.h names five layouts (rgb24 = 0, bgr24, rgb0, bgr0, gbrp: an id space of their own, separate from
 * the format ids above), two matrices (bt709 = 0, bt601 = 1) and two ranges (tv = 0, pc = 1) and defines the conversion to
 * 8-bit 4:2:0 Y'CbCr in integers: luma per pixel, chroma from the 2x2 mean, rounded once.  wrenc_gpu_set_source_rgb makes
 * wrenc_gpu_upload_planes take the layout's planes as wrenc_gpu_rgb_layout numbers them -- plane[0] alone for the packed
 * layouts, G, B, R for gbrp -- copy them into the raw staging planes as with a source format, and a kernel behind the copies
 * (wrenc_amd/csrc/dev_rgb.h) writes the converted picture, bit for bit what wrenc_gpu_rgb_convert_host gives: into the
 * scaler's staging planes when a source size is set -- conversion comes BEFORE scaling -- else into the slot's planes.
 * Everything behind the upload sees the converted picture.  The stream carries no VUI: matrix and range are NOT signalled.
 * The rules of wrenc_gpu_set_source_format apply: any order with the size setters; WRENC_GPU_EINVAL for an unknown layout,
 * matrix or range; WRENC_GPU_ESTATE once any slot has been uploaded into; layout -1 (matrix and range are then not read)
 * puts the context back, and a context on which no RGB source is set launches and allocates nothing it did not before.
 * An RGB source and a non-zero source format exclude each other: while one is set, setting the other returns
 * WRENC_GPU_ESTATE (wrenc_gpu_set_source_format(ctx, 0) stays a no-op that succeeds).  While an RGB source is set
 * wrenc_gpu_upload and wrenc_gpu_encode_picture return WRENC_GPU_ESTATE and wrenc_gpu_source_format keeps returning 0.
 * wrenc_gpu_source_rgb: the three ids; layout -1 (and 0, 0) when none is set. */
int wrenc_gpu_set_source_rgb(wrenc_gpu_ctx* ctx, int layout, int matrix, int range);
int wrenc_gpu_source_rgb(const wrenc_gpu_ctx* ctx, int* layout, int* matrix, int* range);
/* Host only, callable without a device.  The id of a layout's name ("rgba" and "bgra" are aliases of rgb0 and bgr0) or
 * WRENC_GPU_EINVAL; the name of an id or NULL; the layout of a tightly packed w x h frame (n_planes 1 or 3; the limits of
 * wrenc_gpu_format_layout); the nine coefficients in the order yr yg yb, br bg bb, rr rg rb, then yoff; and the rules of
 * wrenc_rgb.h over a whole picture -- planes and strides as wrenc_gpu_rgb_layout numbers them, y of w x h and cb, cr of
 * w/2 x h/2 bytes tightly packed -- which is what the device can be held against.  WRENC_GPU_EINVAL for an unknown id, a
 * size outside the limits, a null pointer that is read or a stride smaller than the row. */
int wrenc_gpu_rgb_from_name(const char* name);
const char* wrenc_gpu_rgb_name(int layout);
int wrenc_gpu_rgb_layout(int layout, int w, int h, struct wrenc_gpu_format_layout* out);
int wrenc_gpu_rgb_coefficients(int matrix, int range, int out[10]);
int wrenc_gpu_rgb_convert_host(int layout, int matrix, int range, int w, int h, const void* const plane[3], const size_t stride_bytes[3],
                               uint8_t* y, uint8_t* cb, uint8_t* cr);
/* Pictures that are already in device memory.  wrenc_gpu_upload_planes with planes that are DEVICE memory of the context's
 * device, for every source kind: format 0, the other formats and RGB.  The data is COPIED (device to device) into the places
 * the host entry copies to -- the kernels keep the alignment and read-past-row guarantees of the library's own pitches --;
 * the caller's memory is not read in place.  The null, stride and alignment checks of the host entry apply, and each plane
 * that is read must be device memory of the context's device (hipPointerGetAttributes): WRENC_GPU_EINVAL for a host pointer,
 * pinned or not, and for memory of another device.
 * Ordering, with no host wait in the call.  producer_stream is a hipStream_t; NULL is the null stream (PyTorch's default
 * stream on ROCm), handled like any other: the context's copy stream is non-blocking and does not synchronise with it by
 * itself.  The call records an event on the producer stream and the copy stream waits for it; once this upload's copies are
 * queued it records an event on the copy stream and the producer stream waits for that.  So the caller may queue the upload
 * right behind the work that writes the planes, and work that overwrites or frees them right behind the upload, on that
 * stream, without synchronising.  Work on OTHER streams that touches the planes is the caller's to order. */
int wrenc_gpu_upload_planes_device(wrenc_gpu_ctx* ctx, int slot, const void* const plane[3], const size_t stride_bytes[3],
                                   void* producer_stream);
/* Test entry: the coded-size original planes a slot holds (width*height, then (width/2)*(height/2) twice), margin
 * included.  Blocking, behind the copy stream.  WRENC_GPU_ESTATE for a slot never uploaded into. */
int wrenc_gpu_test_download_originals(wrenc_gpu_ctx* ctx, int slot, uint8_t* y, uint8_t* cb, uint8_t* cr);

/* Run search + final pass for slots [first_slot, first_slot + n_pictures) whose
 * planes are resident.  Asynchronous.  This is the call a C++ SliceEncoder::encode
 * makes in place of the per-CTU split_ct loop. */
int wrenc_gpu_encode(wrenc_gpu_ctx* ctx, int first_slot, int n_pictures);

/* Per-picture QP: slot `slot` is searched at qcfg->qp by the wrenc_gpu_encode calls enqueued from now on (a call already
 * enqueued keeps what it read).  qcfg is a config resolved for that QP the way the context's was (wrenc_gpu_default_config,
 * then wrenc_gpu_config_extra_params with the same string): the library derives nothing itself.
 *   Per QP, may differ from the context's config:  qp, lambda_q, lambda_rd, lambda_rd_chroma.
 *   Must equal the context's, bit for bit:         width, height, max_split_depth, lv_table, dq_table, header_bits_luma,
 *                                                  header_bits_chroma   (device and n_slots are not read).
 * A context holds one lambda set per QP: its own at its own QP, and for any other the first one registered.
 * WRENC_GPU_EINVAL (slot unchanged, context usable) for a bad slot, a QP outside 0..63, a field that must match and does
 * not, a second lambda set for a QP, or a rate model outside the range wrenc_gpu_create accepts (lambda_q grows with the
 * QP: a model that fits at the context's QP may not at QP 63).  qcfg NULL puts the slot back to the context's config.
 * An encode call whose pictures share one QP runs exactly as one of a context created at that QP; a mixed call orders
 * its pictures by QP (each workgroup holds one) and pads every QP class to a multiple of 4 pictures. */
int wrenc_gpu_set_slot_qp(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_config* qcfg);

/* Wait for everything queued on the context. */
int wrenc_gpu_sync(wrenc_gpu_ctx* ctx);

/* Copy a slot's results to host memory (blocking).  Waits for the wrenc_gpu_encode call
 * that searched the slot and for nothing queued after it, so with two sets of slots the
 * read-back of one set overlaps the search of the other. */
int wrenc_gpu_download(wrenc_gpu_ctx* ctx, int slot, wrenc_gpu_picture* out);

/* Compact read-back.  The level planes of a picture are mostly zeros (6 bytes per luma sample on the bus for a few
 * hundred coded bytes); a device pass behind the search packs them: one bit per 4x4 BLOCK OF LEVELS (picture-aligned,
 * luma plane, then Cb, then Cr, each in raster order of its 4x4 blocks: (W/4)(H/4) + 2 (W/8)(H/8) bits, bit b of word
 * b / 32) and, for the blocks with a non-zero level, the 16 levels (row-major) back to back in mask order.
 * wrenc_gpu_download_compact reads back `n` slots in one call: per picture the mask, its count of coded blocks, their
 * levels (up to payload_cap blocks: WRENC_GPU_ENOMEM with n_blocks set to the need if a picture has more), the maps,
 * and the reconstruction when asked for.  Blocking; waits for the encode call of the slots and nothing queued later.
 * wrenc_gpu_expand_levels is the host-side inverse (no device involved): dense level planes as wrenc_gpu_download
 * fills them, for consumers of the plane layout (wrenc_bs_write_picture). */
typedef struct wrenc_gpu_compact {
    uint32_t* mask;         /* wrenc_gpu_compact_mask_words(width, height) words */
    int16_t* payload;       /* payload_cap x 16 levels */
    size_t payload_cap;     /* in blocks of 16 levels */
    size_t n_blocks;        /* out: coded blocks of this picture */
    uint8_t* cu_log2_size;  /* as in wrenc_gpu_picture; any may be NULL */
    uint8_t* luma_mode;
    uint8_t* chroma_mode;
    uint8_t* rec_y;
    uint8_t* rec_cb;
    uint8_t* rec_cr;
} wrenc_gpu_compact;
size_t wrenc_gpu_compact_mask_words(int width, int height);
int wrenc_gpu_download_compact(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_gpu_compact* out);
void wrenc_gpu_expand_levels(int width, int height, const uint32_t* mask, const int16_t* payload, int16_t* lev_y,
                             int16_t* lev_cb, int16_t* lev_cr);

/* Token read-back (round 4): residual_coding done on the device.  Behind the search a device pass walks every CTU's
 * transform blocks in coding order and turns their levels into the tokens the host's arithmetic coder consumes as they
 * come (ctu_encoder.rs:1786-2269, context selection bool_coder.rs:2053-2400, binarisations :1133-1465):
 *     context-coded bin   (ctx << 1) | bin                      ctx: index into the flat context array of wrenc_amd/csrc/host/cabac.h
 *     bypass group        1 << 31 | (nbits - 1) << 25 | value   nbits <= 25
 * Per transform unit (CU luma + Cb + Cr; a 4x4 luma block of a split 8x8 CU; the 4x4 Cb + Cr pair of such a CU) one header
 * word per component -- bit 31: coded, bits 0..23: tokens of the component that follow, bit 30 (luma): the last
 * significant position is not the DC position (MtsDcOnly = 0), bit 29 (luma): a level outside the 16x16 low-frequency
 * corner (MtsZeroOutSigCoeffFlag = 0) -- then the components' tokens in order.  Tokens live in PAGES of
 * WRENC_GPU_TOKEN_PAGE words (the last word of a page is the index of the CTU's next page, 0xFFFFFFFF at its end) taken
 * from `pool`; first_page[ctu] (CTUs in raster order) is where a CTU starts.  The CU-level syntax stays on the host: it
 * needs only the maps.  wrenc_bs_write_picture_tokens (wrenc_bitstream.h) writes the same bytes from this record as
 * wrenc_bs_write_picture writes from the level planes, with the residual syntax walk gone from the host.
 * wrenc_gpu_download_tokens reads back `n` slots in one call: pool_cap_words of room in `pool` for all of them together
 * (WRENC_GPU_ENOMEM if it does not suffice, or if the device has no memory left for the pass's own scratch: fall back
 * to wrenc_gpu_download_compact), every picture's first_page table
 * and maps, its reconstruction when asked for.  The pages in use are spread over the WHOLE pool (it is cut into up to 64
 * sub-pools that fill side by side, each needing room for its share of the CTUs): page indices are valid up to
 * pool_cap_words -- that is wrenc_bs_tokens::pool_words -- and *pool_words_used is the words of the pages in use, i.e.
 * what crossed the bus (with WRENC_GPU_ENOMEM: of the pages asked for until the pass gave up, 0 when it did not run). */
#define WRENC_GPU_TOKEN_PAGE 64
typedef struct wrenc_gpu_tokens {
    uint32_t* first_page;   /* (width / 32) * (height / 32) entries */
    uint8_t* cu_log2_size;  /* as in wrenc_gpu_picture; any may be NULL */
    uint8_t* luma_mode;
    uint8_t* chroma_mode;
    uint8_t* rec_y;
    uint8_t* rec_cb;
    uint8_t* rec_cr;
} wrenc_gpu_tokens;
int wrenc_gpu_download_tokens(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_gpu_tokens* out, uint32_t* pool,
                              size_t pool_cap_words, size_t* pool_words_used);
/* Test entry: put an arbitrary record (maps + level planes, as wrenc_gpu_download fills them) into a slot as if a search
 * had produced it, so that the token pass can be compared with the host-only writer on records no search emits. */
int wrenc_gpu_test_load_record(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_picture* rec);
/* Test entry: put coded-size planes (width*height, then (width/2)*(height/2) twice) into a slot's reconstruction and mark the
 * slot encoded, so that wrenc_gpu_download_recon can be held against wrenc_recon.h on content no search emits, with a
 * margin unlike the visible edge.  Blocking. */
int wrenc_gpu_test_load_recon(wrenc_gpu_ctx* ctx, int slot, const uint8_t* y, const uint8_t* cb, const uint8_t* cr);

/* Metrics read-back: PSNR and SSIM of what a slot was given against what the search made of it, without the planes
 * crossing the bus.  A device pass behind the search reads the slot's originals (the upload's target) and its
 * reconstruction once and leaves, per plane, the sums the two metrics are made of, in the definitions of ffmpeg's psnr and
 * ssim filters as wrenc_amd/metrics.py restates them: the squared error; and over all (w/4 - 1)(h/4 - 1) windows of the
 * plane (2x2 blocks of 4x4 samples, one block apart) the sum of the window's f32 value
 *     ((float)(2 s1 s2 + c1) * (float)(2 cov + c2)) / ((float)(s1^2 + s2^2 + c1) * (float)(var + c2)),
 *     s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b over the window, var = 64 ss - s1^2 - s2^2,
 *     cov = 64 s12 - s1 s2, c1 = 416, c2 = 235963,
 * every f32 operation rounded on its own, the quotient correctly rounded.  The sums are added in a fixed order: the same
 * planes give the same bytes in any slot, any batch size and any run. */
typedef struct wrenc_gpu_metrics {
    uint64_t sse[3];           /* Y, Cb, Cr: sum of squared differences, exact */
    double   ssim_sum[3];      /* sum of the per-window f32 values */
    uint32_t ssim_windows[3];  /* (w/4 - 1)(h/4 - 1) of the plane */
} wrenc_gpu_metrics;

/* On a context with a visible size (wrenc_gpu_set_visible_size) the figures are those of the visible rectangle: per plane
 * of visible size w x h (a chroma width such as 17 is legal), sse over the w x h samples and SSIM over the
 * ((w >> 2) - 1)((h >> 2) - 1) windows of whole 4x4 blocks inside it -- a partial last block is dropped, as ffmpeg's filter
 * drops it -- with ssim_windows that count; wrenc_gpu_metrics_values is then called with the visible size.  The order of
 * summation is fixed there too.
 * n slots in one call; blocking; waits for the encode call that searched them and for nothing queued later.
 * WRENC_GPU_ESTATE unless every slot is in the encoded state (an upload into a slot replaces its originals
 * and puts it back to "uploaded": ask before re-using the slot).  Changes nothing in the slot. */
int wrenc_gpu_download_metrics(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_gpu_metrics* out);

/* Complexity read-back: how hard a slot's picture is to code, from its originals alone, BEFORE any search -- what a rate
 * controller needs to choose the picture's QP (include/wrenc_rate.h).  Over every picture-aligned 8x8 block of a plane
 * (Y at W x H, Cb and Cr at W/2 x H/2): the unnormalised 2-D 8x8 Hadamard transform (the +-1 matrix) of the 64 samples,
 * act = sum |coefficient| over the 63 coefficients other than DC (at most 130,560).  satd[p] is the plane's sum of act;
 * ctu_satd[c] the sum over the 16 luma, 4 Cb and 4 Cr blocks of CTU c (raster order).  Exact integers: the same planes
 * give the same figures in any slot, any batch size and any run.
 * n slots in one call; blocking.  Runs on the copy stream behind the slots' uploads and waits for those only: a search
 * queued or running on other slots goes on meanwhile.  Works on every slot that holds originals ("uploaded" or
 * "encoded"); WRENC_GPU_ESTATE for a slot never uploaded into, WRENC_GPU_EINVAL for a bad range.  Changes nothing in the
 * slot. */
typedef struct wrenc_gpu_complexity {
    uint64_t satd[3];        /* Y, Cb, Cr */
    uint32_t* ctu_satd;      /* (width/32)*(height/32) entries, may be NULL */
} wrenc_gpu_complexity;
int wrenc_gpu_download_complexity(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_gpu_complexity* out);

/* Rate histogram read-back: the distribution of a slot's residual coefficient magnitudes, from its originals alone, BEFORE
 * any search -- what sets the slope of the picture's bytes-at-QP curve (include/wrenc_rate.h: wrenc_rate_choose_vbv).  The
 * definition, in exact integers, is include/wrenc_ratecurve.h: per picture-aligned 8x8 block of every plane of the CODED
 * picture (a padded context's margin included) the best of the DC, V and H predictions from the neighbours' originals, the
 * 8x8 Hadamard transform of the residual, and per plane the count of coefficients in each of 57 log-magnitude bins.
 * QP-independent; 1536 bytes a picture over the bus; the same planes give the same table in any slot, batch and run.
 * The calling rules are wrenc_gpu_download_complexity's: n slots in one call, blocking, on the copy stream behind the slots'
 * uploads and behind no search; every slot that holds originals; WRENC_GPU_ESTATE for a slot never uploaded into,
 * WRENC_GPU_EINVAL for a bad range; changes nothing in the slot.  Its scratch is allocated on the first call: a context
 * that never calls it launches and allocates nothing it did not before. */
int wrenc_gpu_download_rate_hist(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_rate_hist* out);
/* Host only, no device: the bin of a coefficient magnitude 0 .. 16,320 (WRENC_GPU_EINVAL outside), and the table of a
 * picture of width x height (multiples of 16, at least 16; tightly packed planes) by wrenc_ratecurve.h itself
 * (WRENC_GPU_EINVAL for a bad size or a null pointer). */
int wrenc_gpu_rate_hist_bin(int magnitude);
int wrenc_gpu_rate_hist_host(int width, int height, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, wrenc_rate_hist* out);

/* Distortion curve read-back: the squared error that quantising a slot's residual coefficients leaves at every QP 0 .. 63,
 * from its originals alone, BEFORE any search -- what a quality target chooses a picture's QP by
 * (include/wrenc_rate_quality.h).  The definition, in exact integers, is include/wrenc_distcurve.h: the coefficients of the
 * rate histogram (same blocks, prediction and transform), each quantised with the step of every QP, and per plane and QP
 * the sum of the squared errors; sse8 / 4096 predicts the plane's sample-domain SSE.  1536 bytes a picture over the bus; the
 * same planes give the same table in any slot, batch and run.  The calling rules are wrenc_gpu_download_rate_hist's: n slots
 * in one call, blocking, on the copy stream behind the slots' uploads and behind no search; every slot that holds
 * originals; WRENC_GPU_ESTATE for a slot never uploaded into, WRENC_GPU_EINVAL for a bad range; changes nothing in the
 * slot.  Its scratch is allocated on the first call, for every slot at once: a context that never calls it launches and
 * allocates nothing it did not before. */
int wrenc_gpu_download_dist_curve(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_dist_curve* out);
/* Host only, no device: the table of a picture of width x height (multiples of 16, at least 16; tightly packed planes) by
 * wrenc_distcurve.h itself (WRENC_GPU_EINVAL for a bad size or a null pointer). */
int wrenc_gpu_dist_curve_host(int width, int height, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, wrenc_dist_curve* out);

/* Host only, no device: PSNR (dB) and SSIM as {Avg, Y, U, V} in wrenc_amd/metrics.py's definitions:
 * plane PSNR 10 log10(255^2 n / sse) (+infinity for sse 0), Avg from the MSE over all samples of the frame,
 * SSIM Avg = (4 Y + U + V) / 6. */
void wrenc_gpu_metrics_values(int width, int height, const wrenc_gpu_metrics* m, double psnr[4], double ssim[4]);

/* Hash read-back: the decoded picture hash (H.274 decoded picture hash SEI; the three definitions are in wrenc_hash.h) of
 * what the search made of a slot, without the planes crossing the bus: 48 bytes a picture.  A device pass behind the
 * search reads the slot's reconstruction once -- the coded planes, margin included on a context with a visible size, as a
 * decoder hashes the picture before the conformance window crops it -- and leaves the three components' values as the SEI
 * carries them (include/wrenc_bitstream_hash.h frames the message).  hash_type: WRENC_HASH_MD5, _CRC or _CHECKSUM.
 * Checksum and CRC are parallel passes at about memory rate; MD5 is a serial chain per plane and runs as one lane per
 * (picture, plane): it takes as long as the largest plane needs, however many pictures the call has.
 * n slots in one call; blocking; runs on a stream of its own (made at the first call) behind the encode call that searched
 * the slots and nothing queued later, so it delays neither the search of other slots nor uploads.  WRENC_GPU_ESTATE
 * unless every slot is in the encoded state, WRENC_GPU_EINVAL for a bad range or an unknown hash_type.  Changes nothing in
 * the slot.  The same planes give the same bytes in any slot, any batch size and any run. */
int wrenc_gpu_download_hashes(wrenc_gpu_ctx* ctx, int first_slot, int n, int hash_type, wrenc_picture_hash* out);

/* Measurement: the device time of the kernels of the last wrenc_gpu_download_hashes call, from HIP events around them on
 * the pass's stream.  Taken only in measurement mode (wrenc_gpu_stats_enable); WRENC_GPU_ESTATE when the last call was
 * not timed. */
int wrenc_gpu_last_hash_ms(wrenc_gpu_ctx* ctx, float* ms);

/* Reconstruction out: the coded picture as the caller wants it, made on the device.  wrenc_recon.h defines the output as a
 * function of the VISIBLE reconstruction alone -- what a decoder outputs behind the conformance window; the margin of a
 * padded context is never read -- in seven formats of ONE id space (rgb24 = 0, bgr24, rgb0, bgr0, gbrp as in wrenc_rgb.h, then
 * yuv420p = 5 and nv12 = 6), RGB by a matrix and a range with wrenc_rgb.h's ids from centre-sited bilinear chroma, in
 * integers, each sample rounded once.  A kernel behind the slot's search (wrenc_amd/csrc/dev_recon.h) writes the picture,
 * bit for bit what wrenc_gpu_recon_convert_host gives, into staging planes of the library's own (one set per context with
 * the library's alignment, allocated at the first call: WRENC_GPU_ENOMEM from that call when it fails); a 2-D copy with the
 * caller's strides then fills the caller's planes, and nothing outside the rows' bytes is written there.
 * Both entries: plane[p] and stride_bytes[p] as wrenc_gpu_recon_layout numbers the planes at the context's visible size
 * (the coded size when none is set); matrix and range are not read for the YUV outputs.  They run on a stream of their own
 * (made at the first call) behind the encode call that searched the slot and nothing queued later, as
 * wrenc_gpu_download_hashes does, and delay neither the search of other slots nor uploads.  WRENC_GPU_ESTATE unless the
 * slot is in the encoded state (an upload into the slot puts it back to "uploaded", as for the metrics);
 * WRENC_GPU_EINVAL for a bad slot, a null format, an unknown id, a null plane that is written or a stride below the row.
 * They change nothing in the slot; the same planes give the same bytes in any slot, batch and run.  A context that never
 * calls them launches and allocates nothing it did not before.
 * wrenc_gpu_download_recon: to host memory, blocking.  Only the visible picture in the output format crosses the bus,
 * once.  Any host memory works; the page-locked memory of wrenc_gpu_alloc_host runs at bus rate.
 * wrenc_gpu_download_recon_device: to DEVICE memory of the context's device (hipPointerGetAttributes: WRENC_GPU_EINVAL for
 * a host pointer, pinned or not, and for memory of another device), with no host wait -- the mirror of
 * wrenc_gpu_upload_planes_device.  consumer_stream is a hipStream_t; NULL is the null stream, handled like any other.  The
 * call records an event on the consumer stream and the copies into the caller's planes wait for it, so earlier work on that
 * stream that reads or writes the destination finishes first; behind the copies it records an event that the consumer
 * stream waits for, so what the caller queues there next sees the picture.  Work on OTHER streams is the caller's to
 * order.  The staging planes are reused by the next call on the context, behind this one's copies; an encode call queued
 * later waits for this call's kernel before it rewrites the slot. */
typedef struct wrenc_gpu_recon_format { int32_t format, matrix, range; } wrenc_gpu_recon_format;
int wrenc_gpu_download_recon(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_recon_format* format, void* const plane[3], const size_t stride_bytes[3]);
int wrenc_gpu_download_recon_device(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_recon_format* format, void* const plane[3],
                                    const size_t stride_bytes[3], void* consumer_stream);
/* Host only, callable without a device.  The id of an output format's name ("rgba" and "bgra" are aliases of rgb0 and bgr0)
 * or WRENC_GPU_EINVAL; the name of an id or NULL; the layout of a tightly packed w x h frame (the limits of
 * wrenc_gpu_format_layout); the coefficients in the order cy rv gu gv bu, then yoff; and the rules of wrenc_recon.h over a
 * whole picture -- y of w x h and cb, cr of w/2 x h/2 bytes tightly packed, to planes and strides as wrenc_gpu_recon_layout
 * numbers them -- which is what the device can be held against.  WRENC_GPU_EINVAL for an unknown id, a size outside the
 * limits, a null pointer that is used or a stride smaller than the row. */
int wrenc_gpu_recon_from_name(const char* name);
const char* wrenc_gpu_recon_name(int format);
int wrenc_gpu_recon_layout(int format, int w, int h, struct wrenc_gpu_format_layout* out);
int wrenc_gpu_recon_coefficients(int matrix, int range, int out[6]);
int wrenc_gpu_recon_convert_host(int format, int matrix, int range, int w, int h, const uint8_t* y, const uint8_t* cb, const uint8_t* cr,
                                 void* const plane[3], const size_t stride_bytes[3]);

/* Page-locked host memory for the planes handed to wrenc_gpu_upload / wrenc_gpu_download: transfers from
 * and to it run at PCIe rate and truly asynchronously (pageable buffers are staged by the runtime at a
 * fraction of that).  Optional: any host memory works.  Free with wrenc_gpu_free_host before destroy. */
void* wrenc_gpu_alloc_host(wrenc_gpu_ctx* ctx, size_t bytes);
void wrenc_gpu_free_host(wrenc_gpu_ctx* ctx, void* p);

/* Convenience: upload + encode + download of a single picture through slot 0. */
int wrenc_gpu_encode_picture(wrenc_gpu_ctx* ctx, const uint8_t* y, const uint8_t* cb,
                             const uint8_t* cr, wrenc_gpu_picture* out);

/* How an encode call maps CTUs to wavefronts.  Results are identical (bit-exact) either way.
 *   WAVE: one wavefront per CTU, a workgroup = the same CTU of 4 pictures.  Highest throughput, but it needs
 *         hundreds of pictures in flight to fill the GPU (a picture offers only one anti-diagonal of CTUs at a time).
 *   TEAM: four wavefronts per CTU.  After they have searched the CTU's 32x32 candidate together, each takes one level of
 *         the quad-tree and runs ahead (a node's unsplit search and the search of everything below it read only neighbours
 *         outside the node, block_splitter.rs:1081-1123); the levels meet at the split decisions, and the wavefront left
 *         without a level serves candidate packs to the others.  Shorter CTU latency, for calls with few pictures.
 *   AUTO (default): decided per anti-diagonal of CTUs: TEAM while pictures x CTUs of the diagonal cannot fill the GPU
 *         with one wave each, WAVE beyond. */
enum wrenc_gpu_schedule { WRENC_GPU_SCHEDULE_AUTO = 0, WRENC_GPU_SCHEDULE_WAVE = 1, WRENC_GPU_SCHEDULE_TEAM = 2 };
int wrenc_gpu_set_schedule(wrenc_gpu_ctx* ctx, int schedule);
int wrenc_gpu_last_schedule(const wrenc_gpu_ctx* ctx); /* what the most recent encode call used (AUTO = both) */
/* What the library found and how it was built: wavefronts of the search kernel the device holds at once (CUs x 20) and
 * the HIP streams an encode call deals its pictures to.  For measurement tools (bench.py, tools/fill_probe.py). */
int wrenc_gpu_device_info(const wrenc_gpu_ctx* ctx, long long* wave_slots, int* encode_lanes);
/* Test entry: overrides the number of wave slots AUTO compares a diagonal's CTUs x pictures with (default: what the
 * device holds, CUs x waves per CU), so that a SMALL encode call mixes TEAM and WAVE diagonals as a big one does on
 * the real figure (tests/test_gpu_groups.py).  slots <= 0 restores the device's value.  Results do not depend on it. */
int wrenc_gpu_test_set_wave_slots(wrenc_gpu_ctx* ctx, long long slots);
/* Test entry, needs no context and no device: the launch plan of an encode call (wrenc_amd/csrc/encode_plan.h) -- what
 * wrenc_gpu_encode issues for pictures of ctu_cols x ctu_rows CTUs with the QPs qps[0 .. n_pictures - 1] (0..63, in slot
 * order) under `schedule`, `wave_slots` and the depth (depth3: max_split_depth == 3), with the library's own build constants.
 * A launch: its stream (lane), the kernel (team: 1, wave: 0), the anti-diagonal with its first CTU row and its number of
 * CTUs, the kernel's pictures as entries first .. first + n - 1 of the call's list (a call at one QP has no list: of its
 * slots), the grid, the first group (wave kernel of a mixed call, else -1), the QP whose constant block it takes (-1: the
 * groups name the blocks), the (diagonal, lane) pair it belongs to -- the unit wrenc_gpu_last_encode_stats counts and
 * times as a launch -- and the CTU-pictures it searches without padding.
 * info is always filled.  launches (launches_cap records), entries (the picture of each list entry; entries_cap ints) and
 * groups (QP and pictures per group of WPB entries; 2 x groups_cap ints) may be NULL with a capacity of 0; WRENC_GPU_EINVAL
 * where a capacity is smaller than what info reports, and for arguments wrenc_gpu_encode could not be called with. */
typedef struct wrenc_gpu_plan_launch {
    int32_t lane, team, diag, r_min, count, first, n, grid, group, qp, span;
    int64_t ctus;
} wrenc_gpu_plan_launch;
typedef struct wrenc_gpu_plan_info {
    int32_t n_launches, n_entries, n_groups, n_lanes, n_spans, schedule; /* schedule: what runs (AUTO = both kernels) */
    int32_t wpb, team, encode_lanes, team_below_pct, team_below_pct_depth3; /* the build constants the plan was made with */
} wrenc_gpu_plan_info;
int wrenc_gpu_test_plan(int ctu_cols, int ctu_rows, const int* qps, int n_pictures, int schedule, long long wave_slots, int depth3,
                        wrenc_gpu_plan_info* info, wrenc_gpu_plan_launch* launches, int launches_cap, int* entries, int entries_cap,
                        int* groups, int groups_cap);
/* Test entry: how many workgroups since context creation found the scratch partition of their XCD full and took a
 * region of the shared overflow partition instead (wrenc_gpu.hip, acquire_scratch).  0 on MI355X: the saved
 * reconstructions of the search then stay behind the L2 of the XCD that wrote them.  Waits for the device. */
int wrenc_gpu_test_scratch_overflows(wrenc_gpu_ctx* ctx, long long* count);
/* Per-launch timing (two HIP events around every kernel launch) is OFF by default: the product path
 * (CLI, native program) never reads it.  bench.py / profiling switch it on.  While it is on, an encode
 * call first waits for the previous call's end event (the events are re-recorded), so consecutive calls
 * do not overlap: measurement mode only. */
int wrenc_gpu_stats_enable(wrenc_gpu_ctx* ctx, int on);

/* Device time (ms, HIP events on the context's own stream) and launch count of
 * the search kernel during the last wrenc_gpu_encode call (waits for its end).  WRENC_GPU_ESTATE unless
 * timing was on (wrenc_gpu_stats_enable) when that call was queued. */
int wrenc_gpu_last_encode_stats(wrenc_gpu_ctx* ctx, float* total_ms, float* kernel_ms_sum,
                                int* n_launches);
/* The same per kernel: out[0] = ctu_search_kernel (one wavefront per CTU), out[1] = ctu_search_team_kernel (four per
 * CTU): summed HIP-event durations of its launches in the last encode call, their number, and the CTU-pictures
 * (CTUs x pictures) they searched -- what a roofline per launch of ONE kernel needs. */
typedef struct wrenc_gpu_kernel_stats {
    float ms_sum;
    int32_t launches;
    int64_t ctu_pictures;
} wrenc_gpu_kernel_stats;
int wrenc_gpu_last_encode_kernel_stats(wrenc_gpu_ctx* ctx, wrenc_gpu_kernel_stats out[2]);

/* Transform blocks (a luma block, or a Cb + Cr pair) whose final-pass reconstruction differed from what
 * the search left in their place (expected 0; SURVEY.md 3.4 "treat as a property to test"), accumulated
 * since context creation.  Compared through a position-weighted checksum of the block's samples: a
 * change of any one sample is always seen. */
int wrenc_gpu_final_pass_mismatches(wrenc_gpu_ctx* ctx, long long* count);

#ifdef __cplusplus
}
#endif
#endif /* WRENC_GPU_H */
