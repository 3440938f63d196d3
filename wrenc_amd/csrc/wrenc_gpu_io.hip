// wrenc_gpu_io.hip -- pictures in and results out: every upload path of the C ABI (include/wrenc_gpu.h: plain, strided,
// visible size, scaler, source formats, RGB sources, device-resident planes) and every read-back (maps, compact, tokens,
// metrics, complexity, rate histogram, distortion curve, hashes, the reconstruction in an output format), with the kernels they launch.  A translation unit and a code object of its own in libwrenc_gpu.so (the command
// is at the top of wrenc_gpu.hip): what is added or changed here cannot move an instruction of the search kernels.
//
// The trace and profile builds (-DWRENC_TRACE, -DWRENC_PROFILE) define their device globals in dev_common.h; nothing here
// records a trace or counts cycles, so this unit compiles without them, as the block tests' unit does.
#undef WRENC_TRACE
#undef WRENC_PROFILE
#include "gpu_ctx.h"

// Two helpers of the search that the passes here use: the token pass walks the levels with the quantiser's dependent-
// quantisation state maps (dev_quant.h: position_map, compose_map), the scaler multiplies with dev_transform.h's dot2.
#include "dev_transform.h"
#include "dev_scan.h"
#include "dev_quant.h"
#define WRENC_TOKENS_KERNEL_TU
#include "dev_bins.h"
#include "dev_metrics.h"
#include "dev_hash.h"
#include "dev_complexity.h"
#include "dev_ratecurve.h"
#include "dev_distcurve.h"
#include "dev_pad.h"
#include "dev_scale.h"
#include "dev_format.h"
#include "dev_rgb.h"
#include "dev_recon.h"

#include <cmath>
#include <cstring>

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// Originals of a freshly uploaded picture, planar -> one contiguous tile per CTU (PicBufs::org_t): the search then
// fetches a CTU's 1.5 KB as 12 whole cache lines instead of 64 row pieces of lines it shares with three other CTUs.
// One wave per CTU, lane = dword.
__global__ __launch_bounds__(64) void retile_kernel(const uint8_t* __restrict__ planar, uint8_t* __restrict__ tiled, int W, int H,
                                                   int ctu_cols) {
    const int ctu = blockIdx.x, col = ctu % ctu_cols, row = ctu / ctu_cols;
    const size_t wh = (size_t)W * H;
    uint32_t* dst = (uint32_t*)(tiled + (size_t)ctu * kOrgTile);
    for (int w = threadIdx.x; w < kOrgTile / 4; w += 64) {
        size_t src;
        if (w < 256) { // luma: 8 dwords per row
            src = (size_t)(row * 32 + (w >> 3)) * W + col * 32 + (w & 7) * 4;
        } else {       // chroma: 4 dwords per row, Cb then Cr
            const int pl = (w - 256) >> 6, ww = (w - 256) & 63;
            src = wh + (size_t)pl * (wh >> 2) + (size_t)(row * 16 + (ww >> 2)) * (W >> 1) + col * 16 + (ww & 3) * 4;
        }
        dst[w] = *(const uint32_t*)(planar + src);
    }
}

// Compact read-back (include/wrenc_gpu.h): one workgroup per picture walks the picture's 4x4 blocks of levels in mask
// order, 1024 at a time: a thread loads one block (four 8-byte rows), the waves' ballots are the mask words, and the
// blocks with a non-zero level go to the payload at the running count + their rank (wave ballots, one LDS scan over
// the 16 waves).  The planes are read once at HBM rate; what crosses PCIe afterwards is the mask and the coded blocks.
__global__ __launch_bounds__(1024) void compact_levels_kernel(const PicBufs* __restrict__ slots, int first_slot, int W, int H,
                                                               uint32_t* masks, size_t mask_words, int16_t* payloads,
                                                               size_t payload_stride_blocks, unsigned* counts) {
    __shared__ unsigned s_wave[16];
    __shared__ unsigned s_base;
    const PicBufs pb = slots[first_slot + blockIdx.x];
    const int16_t* lev = pb.lev[0];
    uint32_t* mask = masks + (size_t)blockIdx.x * mask_words;
    int4* pay = (int4*)(payloads + (size_t)blockIdx.x * payload_stride_blocks * 16);
    const int bw = W >> 2, bh = H >> 2;                 // luma plane in 4x4 blocks
    const int nl = bw * bh, ncb = nl >> 2, total = nl + 2 * ncb;
    const size_t wh = (size_t)W * H;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b0 = 0; b0 < total; b0 += 1024) {
        const int b = b0 + threadIdx.x;
        int2 r0 = {0, 0}, r1 = {0, 0}, r2 = {0, 0}, r3 = {0, 0};
        if (b < total) {
            // plane, block row / column, stride
            int pb_ = b, pw = bw;
            size_t off = 0;
            int stride = W;
            if (b >= nl) {
                const int c = b - nl;
                const int pl = c >= ncb ? 1 : 0;
                pb_ = c - pl * ncb;
                pw = bw >> 1;
                stride = W >> 1;
                off = wh + (size_t)pl * (wh >> 2);
            }
            const int by = pb_ / pw, bx = pb_ - by * pw;
            const int16_t* p = lev + off + (size_t)(4 * by) * stride + 4 * bx;
            r0 = *(const int2*)p;
            r1 = *(const int2*)(p + stride);
            r2 = *(const int2*)(p + 2 * stride);
            r3 = *(const int2*)(p + 3 * stride);
        }
        const bool nz = (r0.x | r0.y | r1.x | r1.y | r2.x | r2.y | r3.x | r3.y) != 0;
        const unsigned long long bal = __ballot(nz);
        if (lane == 0) {
            if (b < total) mask[b >> 5] = (uint32_t)bal;
            if (b + 32 < total) mask[(b >> 5) + 1] = (uint32_t)(bal >> 32);
            s_wave[wave] = (unsigned)__popcll(bal);
        }
        __syncthreads();
        unsigned before = s_base;
        for (int wv = 0; wv < wave; ++wv) before += s_wave[wv];
        if (nz) {
            const size_t at = (size_t)before + (unsigned)__popcll(bal & ((1ULL << lane) - 1ULL));
            if (at < payload_stride_blocks) {
                pay[2 * at] = make_int4(r0.x, r0.y, r1.x, r1.y);
                pay[2 * at + 1] = make_int4(r2.x, r2.y, r3.x, r3.y);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned sum = 0;
            for (int wv = 0; wv < 16; ++wv) sum += s_wave[wv];
            s_base += sum;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = s_base;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// ---- the steps the read-back entry points share (wrenc_gpu_sync, wrenc_gpu_download, _download_compact, _download_tokens) ----

// slots first .. first + n - 1 exist (else WRENC_GPU_EINVAL with `range_msg`) and are in state `min_state` at least:
// 1 uploaded, 2 searched  (gpu_ctx.h: wrenc_gpu_encode checks its slots with it too)
int check_slots(wrenc_gpu_ctx* ctx, int first, int n, int min_state, const char* range_msg) {
    if (first < 0 || n < 1 || first + n > ctx->cfg.n_slots) return fail(ctx, WRENC_GPU_EINVAL, range_msg);
    for (int s = first; s < first + n; ++s)
        if (ctx->state[s] < min_state)
            return fail(ctx, WRENC_GPU_ESTATE, min_state == 2 ? "slot has not been encoded" : "slot has no uploaded picture");
    return WRENC_GPU_OK;
}

namespace {

// the copy stream (or `st`) waits for the encode calls that searched these slots and for nothing queued after them (the
// slots of one read-back usually share one call's event: each event is waited for once)
int wait_for_search(wrenc_gpu_ctx* ctx, int first, int n, hipStream_t st = nullptr) {
    hipStream_t cs = st ? st : ctx->copy_stream.get();
    hipEvent_t last = nullptr;
    for (int s = first; s < first + n; ++s)
        if (ctx->slot_event[s] && ctx->slot_event[s] != last) {
            last = ctx->slot_event[s];
            HIP_TRY(ctx, hipStreamWaitEvent(cs, last, 0));
        }
    return WRENC_GPU_OK;
}

// the encode calls' sticky overflow word, read on the copy stream (or `st`) behind what is queued there, as a status
int read_overflow(wrenc_gpu_ctx* ctx, hipStream_t st = nullptr) {
    hipStream_t cs = st ? st : ctx->copy_stream.get();
    int ovf = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&ovf, ctx->d_overflow.get(), sizeof(int), hipMemcpyDeviceToHost, cs));
    HIP_TRY(ctx, hipStreamSynchronize(cs));
    if (ovf & 2) return fail(ctx, WRENC_GPU_EHIP, "internal: a team member never reached a meeting point of the level schedule");
    if (ovf) return fail(ctx, WRENC_GPU_ELEVEL, "a quantised level reached 1024 (reference panics: block_splitter.rs:453)");
    return WRENC_GPU_OK;
}

// one slot's maps and reconstruction planes to the caller's buffers, NULL ones skipped (asynchronous, on the copy stream)
int copy_maps(wrenc_gpu_ctx* ctx, int slot, uint8_t* cu_log2_size, uint8_t* luma_mode, uint8_t* chroma_mode, uint8_t* rec_y,
              uint8_t* rec_cb, uint8_t* rec_cr) {
    const wrenc_gpu_config& c = ctx->cfg;
    const PicBufs& b = ctx->slots[slot];
    hipStream_t cs = ctx->copy_stream.get();
    const size_t n4 = (size_t)(c.width / 4) * (c.height / 4), n8 = (size_t)(c.width / 8) * (c.height / 8);
    if (cu_log2_size) HIP_TRY(ctx, hipMemcpyAsync(cu_log2_size, b.cu_log2, n4, hipMemcpyDeviceToHost, cs));
    if (luma_mode) HIP_TRY(ctx, hipMemcpyAsync(luma_mode, b.luma_mode, n4, hipMemcpyDeviceToHost, cs));
    if (chroma_mode) HIP_TRY(ctx, hipMemcpyAsync(chroma_mode, b.chroma_mode, n8, hipMemcpyDeviceToHost, cs));
    uint8_t* rec[3] = {rec_y, rec_cb, rec_cr};
    for (int p = 0; p < 3; ++p)
        if (rec[p]) HIP_TRY(ctx, hipMemcpyAsync(rec[p], b.rec[p], plane_bytes(c, p, 1), hipMemcpyDeviceToHost, cs));
    return WRENC_GPU_OK;
}

} // namespace

// (gpu_ctx.h: the block tests' unit runs the metrics and hash passes on pictures of its own)
// the metrics pass over n pictures of `slots` from `first` on, on `st`: the waves' partial sums, then the pictures' totals
// (maps: the test entry's per-window values, else NULL)
// vw x vh: the rectangle that is measured, the coded size or a context's visible size (the window variant of the kernel)
hipError_t launch_metrics(const wrenc_gpu_config& c, int vw, int vh, hipStream_t st, const PicBufs* slots, int first, int n,
                          MetricsPartial* partials, MetricsSums* sums, float* maps) {
    const int per_pic = met_plane(vw, vh, 0).waves + 2 * met_plane(vw, vh, 1).waves;
    const long long waves = (long long)n * per_pic;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if ((vw != c.width || vh != c.height) && maps) return hipErrorInvalidValue; // the window variant stores no maps
    if (vw != c.width || vh != c.height)
        hipLaunchKernelGGL((metrics_kernel<false, true>), grid, dim3(256), 0, st, slots, first, n, c.width, c.height, vw, vh, partials, maps);
    else if (maps)
        hipLaunchKernelGGL((metrics_kernel<true, false>), grid, dim3(256), 0, st, slots, first, n, c.width, c.height, vw, vh, partials, maps);
    else
        hipLaunchKernelGGL((metrics_kernel<false, false>), grid, dim3(256), 0, st, slots, first, n, c.width, c.height, vw, vh, partials, maps);
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(n), dim3(64), 0, st, partials, vw, vh, sums);
    return hipGetLastError();
}

void fill_metrics(int vw, int vh, const MetricsSums& s, wrenc_gpu_metrics& m) {
    for (int p = 0; p < 3; ++p) {
        m.sse[p] = s.sse[p];
        m.ssim_sum[p] = s.ssim[p];
        m.ssim_windows[p] = (uint32_t)met_plane(vw, vh, p ? 1 : 0).windows;
    }
}

// the hash pass over n pictures of `slots` from `first` on, on `st` (dev_hash.h): an MD5 lane per plane, or the waves'
// partials and the finish; `tables` is read by the CRC only
hipError_t launch_hashes(const wrenc_gpu_config& c, hipStream_t st, const PicBufs* slots, int first, int n, int hash_type,
                         const HashTables* tables, uint32_t* partials, wrenc_picture_hash* values) {
    if (hash_type == WRENC_HASH_MD5) {
        hipLaunchKernelGGL(hash_md5_kernel, dim3((unsigned)md5_waves(n)), dim3(64), 0, st, slots, first, n, c.width, c.height, values);
        return hipGetLastError();
    }
    const HashPlane L = hash_plane(c.width, c.height, 0), C = hash_plane(c.width, c.height, 1);
    const long long waves = (long long)n * (L.pieces + 2 * C.pieces);
    // a workgroup of the CRC pass copies the tables to LDS first: few enough workgroups that each takes many pieces
    const long long groups = (waves + 3) / 4;
    const dim3 grid((unsigned)(groups < 2048 ? groups : 2048));
    const uint32_t start_l = hash_crc_start_term(L.bytes), start_c = hash_crc_start_term(C.bytes);
    if (hash_type == WRENC_HASH_CRC) {
        hipLaunchKernelGGL(hash_piece_kernel<true>, grid, dim3(256), 0, st, slots, first, n, c.width, c.height, tables, partials);
        hipLaunchKernelGGL(hash_finish_kernel<true>, dim3((unsigned)n, 3), dim3(64), 0, st, partials, c.width, c.height, tables, start_l, start_c, values);
    } else {
        hipLaunchKernelGGL(hash_piece_kernel<false>, grid, dim3(256), 0, st, slots, first, n, c.width, c.height, tables, partials);
        hipLaunchKernelGGL(hash_finish_kernel<false>, dim3((unsigned)n, 3), dim3(64), 0, st, partials, c.width, c.height, tables, start_l, start_c, values);
    }
    return hipGetLastError();
}

size_t hash_partials(const wrenc_gpu_config& c) {
    return (size_t)hash_plane(c.width, c.height, 0).pieces + 2 * (size_t)hash_plane(c.width, c.height, 1).pieces;
}

// the CRC's tables, in place before anything queued on `st` after this call reads them
static hipError_t upload_hash_tables(HashTables* d_tables, hipStream_t st) {
    HashTables t;
    hash_fill_tables(t);
    const hipError_t e = hipMemcpyAsync(d_tables, &t, sizeof(t), hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// the RGB converter over one picture (dev_rgb.h), layout L
template <int L>
static void launch_rgb(const RgbArgs& a, hipStream_t cs) {
    const dim3 grid((unsigned)((a.w + 64 * kRgbGroup - 1) / (64 * kRgbGroup)), (unsigned)((a.h / 2 + kRgbRows - 1) / kRgbRows));
    hipLaunchKernelGGL(convert_rgb_kernel<L>, grid, dim3(64, kRgbRows), 0, cs, a);
}

// the RGB output of one picture's reconstruction (dev_recon.h), layout L
template <int L>
static void launch_recon_rgb(const ReconArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.w + 64 * kReconGroup - 1) / (64 * kReconGroup)), (unsigned)((a.h / 2 + kReconRows - 1) / kReconRows));
    hipLaunchKernelGGL(recon_rgb_kernel<L>, grid, dim3(64, kReconRows), 0, st, a);
}

extern "C" {

// what every upload ends with, on copy_stream behind whatever wrote the visible rectangle of the slot's planes
static int finish_upload(wrenc_gpu_ctx* ctx, int slot) {
    const size_t w = ctx->cfg.width, h = ctx->cfg.height, vw = (size_t)ctx->vis_w, vh = (size_t)ctx->vis_h;
    PicBufs& b = ctx->slots[slot];
    hipStream_t cs = ctx->copy_stream.get();
    // a picture smaller than the coded size: its last column and row replicated into the margin of the three planes
    // (dev_pad.h), behind the copies and in front of the tiling
    if (vw != w || vh != h) {
        const int items = pad_items((int)w, (int)h, (int)vw, (int)vh);
        hipLaunchKernelGGL(pad_edges_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, cs, (uint8_t*)b.org[0], (int)w, (int)h,
                           (int)vw, (int)vh);
    }
    // planar staging -> CTU tiles (what the search reads), behind the copies on the same stream
    hipLaunchKernelGGL(retile_kernel, dim3(ctx->ctu_cols * ctx->ctu_rows), dim3(64), 0, cs, b.org[0], (uint8_t*)b.org_t, (int)w,
                       (int)h, ctx->ctu_cols);
    HIP_TRY(ctx, hipGetLastError());
    ctx->uploads_pending = true;
    ctx->any_upload = true;
    ctx->state[slot] = 1;
    return WRENC_GPU_OK;
}

// Where the planes of an upload lie: host memory (the entries that take host pointers) or memory of the context's device
// (wrenc_gpu_upload_planes_device), whose copies are ordered against the caller's stream on both sides.
struct PlaneSource {
    hipMemcpyKind kind = hipMemcpyHostToDevice;
    bool device = false;
    hipStream_t producer = nullptr;
};

// device-resident planes: copy_stream goes on only behind what the producer stream has queued so far ...
static int wait_for_producer(wrenc_gpu_ctx* ctx, const PlaneSource& from) {
    if (!from.device) return WRENC_GPU_OK;
    if (!ctx->ev_producer) HIP_TRY(ctx, ctx->ev_producer.create(hipEventDisableTiming));
    if (!ctx->ev_copied) HIP_TRY(ctx, ctx->ev_copied.create(hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_producer.get(), from.producer));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream.get(), ctx->ev_producer.get(), 0));
    return WRENC_GPU_OK;
}

// ... and what the producer stream queues from now on runs behind the copies of this upload, which are all queued: the
// caller may overwrite or free the planes on that stream right away.  No host wait on either side.
static int release_producer(wrenc_gpu_ctx* ctx, const PlaneSource& from) {
    if (!from.device) return WRENC_GPU_OK;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_copied.get(), ctx->copy_stream.get()));
    HIP_TRY(ctx, hipStreamWaitEvent(from.producer, ctx->ev_copied.get(), 0));
    return WRENC_GPU_OK;
}

// the plain upload: planar 8-bit 4:2:0 planes of the source size (wrenc_gpu_upload, and format 0 of the entries below)
static int upload_plain(wrenc_gpu_ctx* ctx, int slot, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, size_t stride_y, size_t stride_c,
                        const PlaneSource& from) {
    if (slot < 0 || slot >= ctx->cfg.n_slots || !y || !cb || !cr) return fail(ctx, WRENC_GPU_EINVAL, "bad slot or null plane");
    if (ctx->src_format) return fail(ctx, WRENC_GPU_ESTATE, "a source format is set: the planes go through wrenc_gpu_upload_planes");
    if (ctx->src_rgb >= 0) return fail(ctx, WRENC_GPU_ESTATE, "an RGB source is set: the planes go through wrenc_gpu_upload_planes");
    const size_t w = ctx->cfg.width, h = ctx->cfg.height;
    const size_t vw = (size_t)ctx->vis_w, vh = (size_t)ctx->vis_h; // the slot's picture; w x h unless a visible size is set
    const bool scaling = ctx->src_w != 0;
    const size_t sw = scaling ? (size_t)ctx->src_w : vw, sh = scaling ? (size_t)ctx->src_h : vh; // the caller's planes
    if (stride_y < sw || stride_c < sw / 2) return fail(ctx, WRENC_GPU_EINVAL, "stride smaller than row");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    PicBufs& b = ctx->slots[slot];
    // the planes may still be read by a search in flight on this slot
    if (ctx->slot_event[slot]) HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream.get(), ctx->slot_event[slot], 0));
    hipStream_t cs = ctx->copy_stream.get();
    if (const int rc = wait_for_producer(ctx, from)) return rc;
    if (scaling) {
        // Source-size planes into the context's staging planes, then the scaler (dev_scale.h) writes the visible
        // rectangle of the slot's planes.  Copies, scaler, pad and retile all run on copy_stream, in order: the one set of
        // staging planes is read out before the next upload's copies reach it, whichever slot that one is for.  The
        // same holds one step earlier on a context with a source format (wrenc_gpu_upload_planes below): raw copies,
        // converter, scaler, pad and retile are one chain on this stream, so the one set of raw staging planes has been
        // converted out of, and the scaler's planes -- which the converter then writes in place of the copies -- scaled
        // out of, before the next upload's first copy starts.
        ScaleArgs a = ctx->scale_args;
        const uint8_t* const planes[3] = {y, cb, cr};
        for (int p = 0; p < 3; ++p)
            HIP_TRY(ctx, hipMemcpy2DAsync((void*)a.src[p], (size_t)a.src_pitch[p ? 1 : 0], planes[p], p ? stride_c : stride_y,
                                          p ? sw / 2 : sw, p ? sh / 2 : sh, from.kind, cs));
        if (const int rc = release_producer(ctx, from)) return rc;
        a.dst = (uint8_t*)b.org[0];
        hipLaunchKernelGGL(scale_kernel, dim3((unsigned)(a.tiles[0] + 2 * a.tiles[1])), dim3(256), 0, cs, a);
    } else {
        HIP_TRY(ctx, hipMemcpy2DAsync((void*)b.org[0], w, y, stride_y, vw, vh, from.kind, cs));
        HIP_TRY(ctx, hipMemcpy2DAsync((void*)b.org[1], w / 2, cb, stride_c, vw / 2, vh / 2, from.kind, cs));
        HIP_TRY(ctx, hipMemcpy2DAsync((void*)b.org[2], w / 2, cr, stride_c, vw / 2, vh / 2, from.kind, cs));
        if (const int rc = release_producer(ctx, from)) return rc;
    }
    return finish_upload(ctx, slot);
}

int wrenc_gpu_upload(wrenc_gpu_ctx* ctx, int slot, const uint8_t* y, const uint8_t* cb, const uint8_t* cr,
                     size_t stride_y, size_t stride_c) {
    if (!ctx) return WRENC_GPU_EINVAL;
    return upload_plain(ctx, slot, y, cb, cr, stride_y, stride_c, PlaneSource{});
}

int wrenc_gpu_set_visible_size(wrenc_gpu_ctx* ctx, int vis_w, int vis_h) {
    if (!ctx) return WRENC_GPU_EINVAL;
    const wrenc_gpu_config& c = ctx->cfg;
    if (vis_w != c.width || vis_h != c.height) {
        if (vis_w < 16 || vis_h < 16 || (vis_w & 1) || (vis_h & 1))
            return fail(ctx, WRENC_GPU_EINVAL, "the visible size must be even and at least 16x16");
        if ((vis_w + 31) / 32 * 32 != c.width || (vis_h + 31) / 32 * 32 != c.height)
            return fail(ctx, WRENC_GPU_EINVAL, "the context's size must be the visible size rounded up to a multiple of 32");
    }
    if (ctx->any_upload) return fail(ctx, WRENC_GPU_ESTATE, "the visible size must be set before the first upload");
    if (ctx->src_w) return fail(ctx, WRENC_GPU_ESTATE, "a source size is set: the visible size comes first, then the source size");
    ctx->vis_w = vis_w;
    ctx->vis_h = vis_h;
    return WRENC_GPU_OK;
}

int wrenc_gpu_visible_size(const wrenc_gpu_ctx* ctx, int* w, int* h) {
    if (!ctx || !w || !h) return WRENC_GPU_EINVAL;
    *w = ctx->vis_w;
    *h = ctx->vis_h;
    return WRENC_GPU_OK;
}

int wrenc_gpu_scale_taps(int n_in, int n_out, int o, int* first, int* n_taps, int16_t coef[WRENC_SCALE_MAX_TAPS]) {
    return wrenc_scale_taps(n_in, n_out, o, first, n_taps, coef) ? WRENC_GPU_EINVAL : WRENC_GPU_OK;
}

namespace {

// the tables of one axis (dev_scale.h: ScaleAxis) as they go to the device
struct ScaleAxisHost {
    std::vector<int> first, tile_base;
    std::vector<int16_t> coef;
    int n_in = 0, n_out = 0, taps = 0, span = 0;
};

// tile: output samples per tile of this axis; align4: tile_base rounded down to a multiple of 4 (the x axis: dword loads)
bool build_scale_axis(int n_in, int n_out, int tile, bool align4, ScaleAxisHost& h) {
    h.n_in = n_in;
    h.n_out = n_out;
    h.first.assign((size_t)n_out, 0);
    h.coef.assign((size_t)n_out * kScaleCoefs, 0);
    h.taps = 0;
    for (int o = 0; o < n_out; ++o) {
        int16_t k[WRENC_SCALE_MAX_TAPS];
        int n = 0;
        if (wrenc_scale_taps(n_in, n_out, o, &h.first[(size_t)o], &n, k) || n > kScaleCoefs) return false;
        for (int j = 0; j < n; ++j) h.coef[(size_t)o * kScaleCoefs + j] = k[j];
        h.taps = n > h.taps ? n : h.taps;
    }
    h.taps = (h.taps + 1) & ~1;
    const int tiles = (n_out + tile - 1) / tile;
    h.tile_base.assign((size_t)tiles, 0);
    h.span = 0;
    for (int t = 0; t < tiles; ++t) {
        int lo = h.first[(size_t)t * tile], hi = lo;
        for (int o = t * tile; o < n_out && o < (t + 1) * tile; ++o) {
            lo = h.first[(size_t)o] < lo ? h.first[(size_t)o] : lo;
            hi = h.first[(size_t)o] > hi ? h.first[(size_t)o] : hi;
        }
        if (align4) lo &= ~3;
        h.tile_base[(size_t)t] = lo;
        h.span = hi + h.taps - lo > h.span ? hi + h.taps - lo : h.span;
    }
    return true;
}

} // namespace

int wrenc_gpu_set_source_size(wrenc_gpu_ctx* ctx, int src_w, int src_h) {
    if (!ctx) return WRENC_GPU_EINVAL;
    const int vw = ctx->vis_w, vh = ctx->vis_h;
    const bool plain = src_w == vw && src_h == vh;
    if (!plain) {
        if (src_w < 16 || src_h < 16 || (src_w & 1) || (src_h & 1))
            return fail(ctx, WRENC_GPU_EINVAL, "the source size must be even and at least 16x16");
        if (src_w > 4 * vw || vw > 4 * src_w || src_h > 4 * vh || vh > 4 * src_h || src_w > WRENC_SCALE_MAX_SIZE ||
            src_h > WRENC_SCALE_MAX_SIZE)
            return fail(ctx, WRENC_GPU_EINVAL, "the source size must be within a factor of 4 of the visible size in each dimension");
    }
    if (ctx->any_upload) return fail(ctx, WRENC_GPU_ESTATE, "the source size must be set before the first upload");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    ctx->d_stage.reset();
    ctx->d_scale_tab.reset();
    ctx->src_w = ctx->src_h = 0;
    if (plain) return WRENC_GPU_OK;
    // the four tables: x and y of luma, x and y of chroma; every piece starts on a 16-byte boundary of one allocation
    ScaleAxisHost ax[4];
    const int n_in[4] = {src_w, src_h, src_w / 2, src_h / 2}, n_out[4] = {vw, vh, vw / 2, vh / 2};
    size_t at = 0, off[4][3];
    for (int i = 0; i < 4; ++i) {
        const bool is_x = !(i & 1);
        if (!build_scale_axis(n_in[i], n_out[i], is_x ? kScaleTileW : kScaleTileH, is_x, ax[i]) ||
            ax[i].span > (is_x ? kScaleSpanX : kScaleSpanY))
            return fail(ctx, WRENC_GPU_EINVAL, "the scaler's tables do not fit its tile");
        const size_t bytes[3] = {ax[i].first.size() * sizeof(int), ax[i].coef.size() * sizeof(int16_t), ax[i].tile_base.size() * sizeof(int)};
        for (int k = 0; k < 3; ++k) {
            off[i][k] = at;
            at += (bytes[k] + 15) & ~(size_t)15;
        }
    }
    std::vector<uint8_t> tab(at, 0);
    for (int i = 0; i < 4; ++i) {
        memcpy(&tab[off[i][0]], ax[i].first.data(), ax[i].first.size() * sizeof(int));
        memcpy(&tab[off[i][1]], ax[i].coef.data(), ax[i].coef.size() * sizeof(int16_t));
        memcpy(&tab[off[i][2]], ax[i].tile_base.data(), ax[i].tile_base.size() * sizeof(int));
    }
    const size_t pitch_y = ((size_t)src_w + 15) & ~(size_t)15, pitch_c = ((size_t)src_w / 2 + 15) & ~(size_t)15;
    const size_t stage_y = pitch_y * (size_t)src_h, stage_c = pitch_c * (size_t)(src_h / 2);
    hipError_t e = ctx->d_scale_tab.alloc(at);
    if (e == hipSuccess) e = ctx->d_stage.alloc(stage_y + 2 * stage_c);
    if (e == hipSuccess) e = hipMemcpy(ctx->d_scale_tab.get(), tab.data(), at, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ctx->d_stage.reset();
        ctx->d_scale_tab.reset();
        return fail(ctx, e == hipErrorOutOfMemory ? WRENC_GPU_ENOMEM : WRENC_GPU_EHIP, std::string("scaler buffers: ") + hipGetErrorString(e));
    }
    ScaleArgs& a = ctx->scale_args;
    a = ScaleArgs{};
    const uint8_t* base = ctx->d_scale_tab.get();
    for (int i = 0; i < 4; ++i) {
        ScaleAxis& d = (i & 1) ? a.y[i >> 1] : a.x[i >> 1];
        d.first = (const int*)(base + off[i][0]);
        d.coef = (const int16_t*)(base + off[i][1]);
        d.tile_base = (const int*)(base + off[i][2]);
        d.n_in = ax[i].n_in;
        d.n_out = ax[i].n_out;
        d.taps = ax[i].taps;
        d.span = ax[i].span;
    }
    a.src[0] = ctx->d_stage.get();
    a.src[1] = ctx->d_stage.get() + stage_y;
    a.src[2] = ctx->d_stage.get() + stage_y + stage_c;
    a.src_pitch[0] = (int)pitch_y;
    a.src_pitch[1] = (int)pitch_c;
    a.W = ctx->cfg.width;
    a.H = ctx->cfg.height;
    for (int c = 0; c < 2; ++c) {
        a.tiles_x[c] = (int)ax[2 * c].tile_base.size();
        a.tiles[c] = a.tiles_x[c] * (int)ax[2 * c + 1].tile_base.size();
    }
    ctx->src_w = src_w;
    ctx->src_h = src_h;
    return WRENC_GPU_OK;
}

int wrenc_gpu_source_size(const wrenc_gpu_ctx* ctx, int* w, int* h) {
    if (!ctx || !w || !h) return WRENC_GPU_EINVAL;
    *w = ctx->src_w ? ctx->src_w : ctx->vis_w;
    *h = ctx->src_w ? ctx->src_h : ctx->vis_h;
    return WRENC_GPU_OK;
}

int wrenc_gpu_format_from_name(const char* name) {
    const int f = wrenc_format_from_name(name);
    return f < 0 ? WRENC_GPU_EINVAL : f;
}

const char* wrenc_gpu_format_name(int format) { return wrenc_format_name(format); }

int wrenc_gpu_format_layout(int format, int w, int h, struct wrenc_gpu_format_layout* out) {
    return wrenc_format_layout(format, w, h, out) ? WRENC_GPU_EINVAL : WRENC_GPU_OK;
}

int wrenc_gpu_rgb_from_name(const char* name) {
    const int l = wrenc_rgb_from_name(name);
    return l < 0 ? WRENC_GPU_EINVAL : l;
}

const char* wrenc_gpu_rgb_name(int layout) { return wrenc_rgb_name(layout); }

int wrenc_gpu_rgb_layout(int layout, int w, int h, struct wrenc_gpu_format_layout* out) {
    return wrenc_rgb_layout(layout, w, h, out) ? WRENC_GPU_EINVAL : WRENC_GPU_OK;
}

int wrenc_gpu_rgb_coefficients(int matrix, int range, int out[10]) { return wrenc_rgb_coefficients(matrix, range, out) ? WRENC_GPU_EINVAL : WRENC_GPU_OK; }

int wrenc_gpu_rgb_convert_host(int layout, int matrix, int range, int w, int h, const void* const plane[3], const size_t stride_bytes[3],
                               uint8_t* y, uint8_t* cb, uint8_t* cr) {
    if (!plane) return WRENC_GPU_EINVAL;
    const uint8_t* const from[3] = {(const uint8_t*)plane[0], (const uint8_t*)plane[1], (const uint8_t*)plane[2]};
    return wrenc_rgb_convert(layout, matrix, range, w, h, from, stride_bytes, y, cb, cr) ? WRENC_GPU_EINVAL : WRENC_GPU_OK;
}

namespace {

// the raw staging planes of the context's format or RGB layout at its source size: pitches, offsets and the bytes of the
// allocation
struct RawStage {
    struct wrenc_gpu_format_layout lay;
    size_t pitch[3], off[3], bytes;
};

// rgb < 0: source format `format` (dev_format.h's pitch); else RGB layout `rgb` (dev_rgb.h's, with room for the last lane's reads)
bool raw_stage(const wrenc_gpu_ctx* ctx, int format, int rgb, RawStage& r) {
    const int sw = ctx->src_w ? ctx->src_w : ctx->vis_w, sh = ctx->src_w ? ctx->src_h : ctx->vis_h;
    if (rgb >= 0 ? wrenc_rgb_layout(rgb, sw, sh, &r.lay) : wrenc_format_layout(format, sw, sh, &r.lay)) return false;
    r.bytes = 0;
    for (int p = 0; p < 3; ++p) {
        r.pitch[p] = rgb >= 0 && p < r.lay.n_planes ? rgb_raw_pitch(rgb, sw) : format_raw_pitch(r.lay.row_bytes[p]);
        r.off[p] = r.bytes;
        r.bytes += r.pitch[p] * r.lay.rows[p];
    }
    return true;
}

// d_raw holds r.bytes: allocated here when it does not (the format, or a size, has changed since)
int ensure_raw_stage(wrenc_gpu_ctx* ctx, const RawStage& r) {
    if (ctx->d_raw && ctx->d_raw.count() == r.bytes) return WRENC_GPU_OK;
    const hipError_t e = ctx->d_raw.alloc(r.bytes);
    if (e != hipSuccess)
        return fail(ctx, e == hipErrorOutOfMemory ? WRENC_GPU_ENOMEM : WRENC_GPU_EHIP, std::string("raw staging planes: ") + hipGetErrorString(e));
    return WRENC_GPU_OK;
}

// the planes of the context's source kind -- format 0, another format or an RGB layout -- from `from` into slot `slot`
int upload_planes_from(wrenc_gpu_ctx* ctx, int slot, const void* const plane[3], const size_t stride_bytes[3], const PlaneSource& from) {
    if (!plane || !stride_bytes) return fail(ctx, WRENC_GPU_EINVAL, "null plane or stride list");
    const int format = ctx->src_format, rgb = ctx->src_rgb;
    if (format == WRENC_FORMAT_YUV420P && rgb < 0) {
        if (stride_bytes[1] != stride_bytes[2]) return fail(ctx, WRENC_GPU_EINVAL, "yuv420p: the two chroma planes share one stride");
        return upload_plain(ctx, slot, (const uint8_t*)plane[0], (const uint8_t*)plane[1], (const uint8_t*)plane[2], stride_bytes[0],
                            stride_bytes[1], from);
    }
    if (slot < 0 || slot >= ctx->cfg.n_slots) return fail(ctx, WRENC_GPU_EINVAL, "bad slot or null plane");
    RawStage r;
    if (!raw_stage(ctx, format, rgb, r)) return fail(ctx, WRENC_GPU_EINVAL, "the source format needs pictures of an even size, at least 16x16");
    for (int p = 0; p < r.lay.n_planes; ++p) {
        if (!plane[p]) return fail(ctx, WRENC_GPU_EINVAL, "bad slot or null plane");
        if (stride_bytes[p] < r.lay.row_bytes[p]) return fail(ctx, WRENC_GPU_EINVAL, "stride smaller than row");
        if (r.lay.bytes_per_sample == 2 && (((uintptr_t)plane[p] | stride_bytes[p]) & 1))
            return fail(ctx, WRENC_GPU_EINVAL, "a 16-bit format needs even plane addresses and strides");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = ensure_raw_stage(ctx, r);
    if (rc) return rc;
    const bool scaling = ctx->src_w != 0;
    const size_t w = ctx->cfg.width, h = ctx->cfg.height;
    PicBufs& b = ctx->slots[slot];
    // the planes may still be read by a search in flight on this slot
    if (ctx->slot_event[slot]) HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream.get(), ctx->slot_event[slot], 0));
    hipStream_t cs = ctx->copy_stream.get();
    if (const int rcw = wait_for_producer(ctx, from)) return rcw;
    // the caller's bytes as they are -- a 10-bit picture crosses the bus once -- and behind them the converter (dev_format.h,
    // dev_rgb.h)
    for (int p = 0; p < r.lay.n_planes; ++p)
        HIP_TRY(ctx, hipMemcpy2DAsync((void*)(ctx->d_raw.get() + r.off[p]), r.pitch[p], plane[p], stride_bytes[p], r.lay.row_bytes[p], r.lay.rows[p],
                                      from.kind, cs));
    if (const int rcr = release_producer(ctx, from)) return rcr;
    // the 8-bit planes the converter writes
    uint8_t* dst;
    size_t dst_off[3] = {0, 0, 0};
    int dst_pitch[2], cw, ch;
    if (scaling) { // into the scaler's staging planes, in the place of wrenc_gpu_upload's copies
        const ScaleArgs& s = ctx->scale_args;
        dst = ctx->d_stage.get();
        for (int p = 0; p < 3; ++p) dst_off[p] = (size_t)(s.src[p] - s.src[0]);
        dst_pitch[0] = s.src_pitch[0];
        dst_pitch[1] = s.src_pitch[1];
        cw = ctx->src_w;
        ch = ctx->src_h;
    } else { // into the visible rectangle of the slot's planes
        dst = (uint8_t*)b.org[0];
        dst_off[1] = w * h;
        dst_off[2] = w * h + w * h / 4;
        dst_pitch[0] = (int)w;
        dst_pitch[1] = (int)(w / 2);
        cw = ctx->vis_w;
        ch = ctx->vis_h;
    }
    if (rgb >= 0) {
        RgbArgs a = {};
        a.raw = ctx->d_raw.get();
        a.dst = dst;
        for (int p = 0; p < 3; ++p) {
            a.raw_off[p] = r.off[p];
            a.dst_off[p] = dst_off[p];
        }
        a.raw_pitch = (int)r.pitch[0];
        a.dst_pitch[0] = dst_pitch[0];
        a.dst_pitch[1] = dst_pitch[1];
        a.w = cw;
        a.h = ch;
        wrenc_rgb_coefficients(ctx->rgb_matrix, ctx->rgb_range, a.k);
        switch (rgb) {
        case WRENC_RGB_RGB24: launch_rgb<WRENC_RGB_RGB24>(a, cs); break;
        case WRENC_RGB_BGR24: launch_rgb<WRENC_RGB_BGR24>(a, cs); break;
        case WRENC_RGB_RGB0: launch_rgb<WRENC_RGB_RGB0>(a, cs); break;
        case WRENC_RGB_BGR0: launch_rgb<WRENC_RGB_BGR0>(a, cs); break;
        default: launch_rgb<WRENC_RGB_GBRP>(a, cs); break;
        }
    } else {
        FormatArgs a = {};
        a.raw = ctx->d_raw.get();
        a.dst = dst;
        for (int p = 0; p < 3; ++p) {
            a.raw_off[p] = r.off[p];
            a.raw_pitch[p] = (int)r.pitch[p];
            a.dst_off[p] = dst_off[p];
        }
        a.dst_pitch[0] = dst_pitch[0];
        a.dst_pitch[1] = dst_pitch[1];
        a.w = cw;
        a.h = ch;
        a.row_blocks[0] = (a.h + kFormatRows - 1) / kFormatRows;
        a.row_blocks[1] = (a.h / 2 + kFormatRows - 1) / kFormatRows;
        const dim3 grid((unsigned)((a.w + 64 * kFormatGroup - 1) / (64 * kFormatGroup)),
                        (unsigned)(a.row_blocks[0] + (r.lay.n_planes == 2 ? 1 : 2) * a.row_blocks[1])), block(64, kFormatRows);
        switch (format) {
        case WRENC_FORMAT_NV12: hipLaunchKernelGGL(convert_format_kernel<WRENC_FORMAT_NV12>, grid, block, 0, cs, a); break;
        case WRENC_FORMAT_YUV420P10LE: hipLaunchKernelGGL(convert_format_kernel<WRENC_FORMAT_YUV420P10LE>, grid, block, 0, cs, a); break;
        case WRENC_FORMAT_P010LE: hipLaunchKernelGGL(convert_format_kernel<WRENC_FORMAT_P010LE>, grid, block, 0, cs, a); break;
        case WRENC_FORMAT_YUV422P: hipLaunchKernelGGL(convert_format_kernel<WRENC_FORMAT_YUV422P>, grid, block, 0, cs, a); break;
        default: hipLaunchKernelGGL(convert_format_kernel<WRENC_FORMAT_YUV422P10LE>, grid, block, 0, cs, a); break;
        }
    }
    if (scaling) {
        ScaleArgs s = ctx->scale_args;
        s.dst = (uint8_t*)b.org[0];
        hipLaunchKernelGGL(scale_kernel, dim3((unsigned)(s.tiles[0] + 2 * s.tiles[1])), dim3(256), 0, cs, s);
    }
    return finish_upload(ctx, slot);
}

} // namespace

int wrenc_gpu_set_source_format(wrenc_gpu_ctx* ctx, int format) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (!wrenc_format_valid(format)) return fail(ctx, WRENC_GPU_EINVAL, "unknown source format");
    if (ctx->any_upload) return fail(ctx, WRENC_GPU_ESTATE, "the source format must be set before the first upload");
    if (ctx->src_rgb >= 0) { // the raw staging planes are the RGB source's
        if (format != WRENC_FORMAT_YUV420P) return fail(ctx, WRENC_GPU_ESTATE, "an RGB source is set (wrenc_gpu_set_source_rgb): put it back with layout -1 first");
        return WRENC_GPU_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    if (format == WRENC_FORMAT_YUV420P) {
        ctx->d_raw.reset();
        ctx->src_format = 0;
        return WRENC_GPU_OK;
    }
    RawStage r;
    if (!raw_stage(ctx, format, -1, r)) return fail(ctx, WRENC_GPU_EINVAL, "the source format needs pictures of an even size, at least 16x16");
    const int rc = ensure_raw_stage(ctx, r);
    if (rc) return rc;
    ctx->src_format = format;
    return WRENC_GPU_OK;
}

int wrenc_gpu_source_format(const wrenc_gpu_ctx* ctx) { return ctx ? ctx->src_format : WRENC_GPU_EINVAL; }

int wrenc_gpu_set_source_rgb(wrenc_gpu_ctx* ctx, int layout, int matrix, int range) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (layout != -1 && (!wrenc_rgb_valid(layout) || !wrenc_rgb_matrix_valid(matrix) || !wrenc_rgb_range_valid(range)))
        return fail(ctx, WRENC_GPU_EINVAL, "unknown RGB layout, matrix or range");
    if (ctx->any_upload) return fail(ctx, WRENC_GPU_ESTATE, "the RGB source must be set before the first upload");
    if (ctx->src_format) return fail(ctx, WRENC_GPU_ESTATE, "a source format is set (wrenc_gpu_set_source_format): put it back to 0 first");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    if (layout == -1) {
        ctx->d_raw.reset();
        ctx->src_rgb = -1;
        return WRENC_GPU_OK;
    }
    RawStage r;
    if (!raw_stage(ctx, 0, layout, r)) return fail(ctx, WRENC_GPU_EINVAL, "an RGB source needs pictures of an even size, at least 16x16");
    const int rc = ensure_raw_stage(ctx, r);
    if (rc) return rc;
    ctx->src_rgb = layout;
    ctx->rgb_matrix = matrix;
    ctx->rgb_range = range;
    return WRENC_GPU_OK;
}

int wrenc_gpu_source_rgb(const wrenc_gpu_ctx* ctx, int* layout, int* matrix, int* range) {
    if (!ctx || !layout || !matrix || !range) return WRENC_GPU_EINVAL;
    *layout = ctx->src_rgb;
    *matrix = ctx->src_rgb >= 0 ? ctx->rgb_matrix : 0;
    *range = ctx->src_rgb >= 0 ? ctx->rgb_range : 0;
    return WRENC_GPU_OK;
}

int wrenc_gpu_upload_planes(wrenc_gpu_ctx* ctx, int slot, const void* const plane[3], const size_t stride_bytes[3]) {
    if (!ctx) return WRENC_GPU_EINVAL;
    return upload_planes_from(ctx, slot, plane, stride_bytes, PlaneSource{});
}

int wrenc_gpu_upload_planes_device(wrenc_gpu_ctx* ctx, int slot, const void* const plane[3], const size_t stride_bytes[3], void* producer_stream) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (!plane || !stride_bytes) return fail(ctx, WRENC_GPU_EINVAL, "null plane or stride list");
    // the planes this source kind reads
    int n = 3;
    if (ctx->src_format || ctx->src_rgb >= 0) {
        RawStage r;
        if (!raw_stage(ctx, ctx->src_format, ctx->src_rgb, r)) return fail(ctx, WRENC_GPU_EINVAL, "the source format needs pictures of an even size, at least 16x16");
        n = r.lay.n_planes;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    for (int p = 0; p < n; ++p) {
        if (!plane[p]) return fail(ctx, WRENC_GPU_EINVAL, "bad slot or null plane");
        hipPointerAttribute_t at = {};
        const hipError_t e = hipPointerGetAttributes(&at, plane[p]);
        if (e != hipSuccess) (void)hipGetLastError(); // a pointer the runtime does not know: plain host memory
        if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->cfg.device)
            return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_upload_planes_device: a plane is not memory of the context's device (host planes go through wrenc_gpu_upload_planes)");
    }
    PlaneSource from;
    from.kind = hipMemcpyDeviceToDevice;
    from.device = true;
    from.producer = (hipStream_t)producer_stream;
    return upload_planes_from(ctx, slot, plane, stride_bytes, from);
}

int wrenc_gpu_test_download_originals(wrenc_gpu_ctx* ctx, int slot, uint8_t* y, uint8_t* cb, uint8_t* cr) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (slot < 0 || slot >= ctx->cfg.n_slots || !y || !cb || !cr) return fail(ctx, WRENC_GPU_EINVAL, "bad slot or null plane");
    if (ctx->state[slot] == 0) return fail(ctx, WRENC_GPU_ESTATE, "slot has no uploaded picture");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const PicBufs& b = ctx->slots[slot];
    uint8_t* out[3] = {y, cb, cr};
    // behind the slot's upload on the copy stream; a search only reads the planes
    for (int p = 0; p < 3; ++p)
        HIP_TRY(ctx, hipMemcpyAsync(out[p], b.org[p], plane_bytes(ctx->cfg, p, 1), hipMemcpyDeviceToHost, ctx->copy_stream.get()));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream.get()));
    return WRENC_GPU_OK;
}

int wrenc_gpu_sync(wrenc_gpu_ctx* ctx) {
    if (!ctx) return WRENC_GPU_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream.get()));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
    for (const HipStream& st : ctx->lanes) HIP_TRY(ctx, hipStreamSynchronize(st.get()));
    return read_overflow(ctx);
}

int wrenc_gpu_download(wrenc_gpu_ctx* ctx, int slot, wrenc_gpu_picture* out) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    if (const int rc = check_slots(ctx, slot, 1, 2, "bad slot")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const PicBufs& b = ctx->slots[slot];
    const wrenc_gpu_config& c = ctx->cfg;
    int16_t* lev[3] = {out->lev_y, out->lev_cb, out->lev_cr};
    // on the copy stream, behind the encode call that searched this slot and nothing later
    hipStream_t cs = ctx->copy_stream.get();
    if (const int rc = wait_for_search(ctx, slot, 1)) return rc;
    for (int k = 0; k < 3; ++k)
        if (lev[k]) HIP_TRY(ctx, hipMemcpyAsync(lev[k], b.lev[k], plane_bytes(c, k, 2), hipMemcpyDeviceToHost, cs));
    if (const int rc = copy_maps(ctx, slot, out->cu_log2_size, out->luma_mode, out->chroma_mode, out->rec_y, out->rec_cb, out->rec_cr))
        return rc;
    if (out->ctu_cost)
        HIP_TRY(ctx, hipMemcpyAsync(out->ctu_cost, b.ctu_cost, sizeof(float) * ctx->ctu_cols * ctx->ctu_rows,
                                    hipMemcpyDeviceToHost, cs));
    return read_overflow(ctx);
}

size_t wrenc_gpu_compact_mask_words(int width, int height) {
    const size_t blocks = (size_t)(width / 4) * (height / 4) * 3 / 2;
    return (blocks + 31) / 32;
}

int wrenc_gpu_download_compact(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_gpu_compact* out) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    if (const int rc = check_slots(ctx, first_slot, n, 2, "slot range out of bounds")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const wrenc_gpu_config& c = ctx->cfg;
    const size_t mask_words = wrenc_gpu_compact_mask_words(c.width, c.height);
    const size_t blocks = (size_t)(c.width / 4) * (c.height / 4) * 3 / 2;
    HIP_TRY(ctx, ctx->d_cmask.grow((size_t)n * mask_words));
    HIP_TRY(ctx, ctx->d_cpayload.grow((size_t)n * blocks * 16));
    HIP_TRY(ctx, ctx->d_ccount.grow((size_t)n));
    hipStream_t cs = ctx->copy_stream.get();
    if (const int rc = wait_for_search(ctx, first_slot, n)) return rc;
    hipLaunchKernelGGL(compact_levels_kernel, dim3(n), dim3(1024), 0, cs, ctx->d_slots.get(), first_slot, c.width, c.height, ctx->d_cmask.get(),
                       mask_words, ctx->d_cpayload.get(), blocks, ctx->d_ccount.get());
    HIP_TRY(ctx, hipGetLastError());
    std::vector<unsigned> counts((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(counts.data(), ctx->d_ccount.get(), (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, cs));
    if (const int rc = read_overflow(ctx)) return rc;
    bool short_buf = false;
    for (int k = 0; k < n; ++k) {
        wrenc_gpu_compact& o = out[k];
        o.n_blocks = counts[(size_t)k];
        if (o.mask) HIP_TRY(ctx, hipMemcpyAsync(o.mask, ctx->d_cmask.get() + (size_t)k * mask_words, mask_words * sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
        if (o.n_blocks > o.payload_cap || (o.n_blocks && !o.payload)) {
            short_buf = true;
        } else if (o.n_blocks) {
            HIP_TRY(ctx, hipMemcpyAsync(o.payload, ctx->d_cpayload.get() + (size_t)k * blocks * 16, o.n_blocks * 16 * sizeof(int16_t),
                                        hipMemcpyDeviceToHost, cs));
        }
        if (const int rc = copy_maps(ctx, first_slot + k, o.cu_log2_size, o.luma_mode, o.chroma_mode, o.rec_y, o.rec_cb, o.rec_cr))
            return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(cs));
    if (short_buf) return fail(ctx, WRENC_GPU_ENOMEM, "wrenc_gpu_download_compact: payload_cap is smaller than n_blocks of a picture");
    return WRENC_GPU_OK;
}

int wrenc_gpu_download_tokens(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_gpu_tokens* out, uint32_t* pool, size_t pool_cap_words,
                              size_t* pool_words_used) {
    if (!ctx || !out || !pool || !pool_words_used || n < 1) return WRENC_GPU_EINVAL;
    if (const int rc = check_slots(ctx, first_slot, n, 2, "bad slot range")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const int ctus = ctx->ctu_cols * ctx->ctu_rows;
    const size_t pages = pool_cap_words / kTokPage;
    if (pages < 1 || pages > 0xFFFFFFF0u) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_download_tokens: pool_cap_words");
    // device scratch of the pass, grown on demand; where there is no room for it the caller falls back as for a short pool
    constexpr int kCounterWords = kTokPools * kTokCounterStride + 1; // the sub-pools' page counters, the "a sub-pool ran out" flag
    const auto no_room = [&](hipError_t e) {
        *pool_words_used = 0;
        return fail(ctx, WRENC_GPU_ENOMEM, std::string("wrenc_gpu_download_tokens: device scratch: ") + hipGetErrorString(e));
    };
    if (const hipError_t e = ctx->d_tok_pool.grow(pages * kTokPage)) return no_room(e);
    if (const hipError_t e = ctx->d_tok_counter.grow(kCounterWords)) return no_room(e);
    if (const hipError_t e = ctx->d_tok_first.grow((size_t)n * ctus)) return no_room(e);
    hipStream_t cs = ctx->copy_stream.get();
    if (const int rc = wait_for_search(ctx, first_slot, n)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_tok_counter.get(), 0, kCounterWords * sizeof(unsigned), cs));
    const int waves = n * ctus;
    // sub-pools: enough CTUs in each (16 or more) that they fill evenly; one for a handful of CTUs
    int n_pools = 1;
    while (n_pools < kTokPools && n_pools * 32 <= waves) n_pools *= 2;
    const size_t sub = pages / (size_t)n_pools; // pages per sub-pool
    hipLaunchKernelGGL(residual_tokens_kernel, dim3((waves + 3) / 4), dim3(256), 0, cs, ctx->ctx_const(), ctx->d_slots.get(), first_slot, n,
                       ctx->d_tok_pool.get(), (unsigned)sub, n_pools - 1, ctx->d_tok_counter.get(), ctx->d_tok_first.get(), (int*)(ctx->d_tok_counter.get() + kCounterWords - 1));
    HIP_TRY(ctx, hipGetLastError());
    std::vector<unsigned> cnt((size_t)kCounterWords);
    HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), ctx->d_tok_counter.get(), kCounterWords * sizeof(unsigned), hipMemcpyDeviceToHost, cs));
    if (const int rc = read_overflow(ctx)) return rc;
    size_t asked = 0;
    bool short_of = cnt[(size_t)kCounterWords - 1] != 0;
    for (int p = 0; p < n_pools; ++p) {
        asked += cnt[(size_t)p * kTokCounterStride];
        short_of = short_of || cnt[(size_t)p * kTokCounterStride] > sub;
    }
    *pool_words_used = asked * kTokPage;
    if (short_of) return fail(ctx, WRENC_GPU_ENOMEM, "wrenc_gpu_download_tokens: the token pool is too small for these pictures");
    for (int p = 0; p < n_pools; ++p) // every sub-pool's pages in use, to the same place in the caller's pool
        if (cnt[(size_t)p * kTokCounterStride])
            HIP_TRY(ctx, hipMemcpyAsync(pool + (size_t)p * sub * kTokPage, ctx->d_tok_pool.get() + (size_t)p * sub * kTokPage,
                                        (size_t)cnt[(size_t)p * kTokCounterStride] * kTokPage * sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
    for (int k = 0; k < n; ++k) {
        wrenc_gpu_tokens& o = out[k];
        if (o.first_page) HIP_TRY(ctx, hipMemcpyAsync(o.first_page, ctx->d_tok_first.get() + (size_t)k * ctus, (size_t)ctus * sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
        if (const int rc = copy_maps(ctx, first_slot + k, o.cu_log2_size, o.luma_mode, o.chroma_mode, o.rec_y, o.rec_cb, o.rec_cr))
            return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(cs));
    return WRENC_GPU_OK;
}

int wrenc_gpu_download_metrics(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_gpu_metrics* out) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    if (const int rc = check_slots(ctx, first_slot, n, 2, "slot range out of bounds")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const wrenc_gpu_config& c = ctx->cfg;
    // a context with a visible size reports that rectangle only
    const int vw = ctx->vis_w, vh = ctx->vis_h;
    const size_t per_pic = (size_t)met_plane(vw, vh, 0).waves + 2 * (size_t)met_plane(vw, vh, 1).waves;
    HIP_TRY(ctx, ctx->d_mpartial.grow((size_t)n * per_pic));
    HIP_TRY(ctx, ctx->d_msums.grow((size_t)n));
    // on the copy stream, behind the encode call that searched these slots and nothing later
    hipStream_t cs = ctx->copy_stream.get();
    if (const int rc = wait_for_search(ctx, first_slot, n)) return rc;
    HIP_TRY(ctx, launch_metrics(c, vw, vh, cs, ctx->d_slots.get(), first_slot, n, ctx->d_mpartial.get(), ctx->d_msums.get(), nullptr));
    std::vector<MetricsSums> sums((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(sums.data(), ctx->d_msums.get(), (size_t)n * sizeof(MetricsSums), hipMemcpyDeviceToHost, cs));
    if (const int rc = read_overflow(ctx)) return rc;
    for (int k = 0; k < n; ++k) fill_metrics(vw, vh, sums[(size_t)k], out[k]);
    return WRENC_GPU_OK;
}

int wrenc_gpu_download_complexity(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_gpu_complexity* out) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    const wrenc_gpu_config& c = ctx->cfg;
    if (const int rc = check_slots(ctx, first_slot, n, 1, "slot range out of bounds")) return rc;
    HIP_TRY(ctx, hipSetDevice(c.device));
    const size_t per_pic = (size_t)cplx_waves(c.width, c.height), n_ctus = (size_t)ctx->ctu_cols * ctx->ctu_rows;
    if (!ctx->d_xpartial) HIP_TRY(ctx, ctx->d_xpartial.alloc((size_t)c.n_slots * per_pic));
    if (!ctx->d_xsums) HIP_TRY(ctx, ctx->d_xsums.alloc((size_t)c.n_slots));
    if (!ctx->d_xmap) HIP_TRY(ctx, ctx->d_xmap.alloc((size_t)c.n_slots * n_ctus));
    // on the copy stream: behind the slots' uploads (queued there) and behind no search -- the pass reads the originals only,
    // which a search of the same slot reads too and nothing but an upload writes
    hipStream_t cs = ctx->copy_stream.get();
    const size_t waves = (size_t)n * per_pic;
    hipLaunchKernelGGL(complexity_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, cs, ctx->d_slots.get(), first_slot, n, c.width,
                       c.height, ctx->d_xpartial.get(), ctx->d_xmap.get());
    hipLaunchKernelGGL(complexity_finish_kernel, dim3(n), dim3(64), 0, cs, ctx->d_xpartial.get(), c.width, c.height, ctx->d_xsums.get());
    HIP_TRY(ctx, hipGetLastError());
    std::vector<ComplexityPartial> sums((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(sums.data(), ctx->d_xsums.get(), (size_t)n * sizeof(ComplexityPartial), hipMemcpyDeviceToHost, cs));
    for (int k = 0; k < n; ++k)
        if (out[k].ctu_satd)
            HIP_TRY(ctx, hipMemcpyAsync(out[k].ctu_satd, ctx->d_xmap.get() + (size_t)k * n_ctus, n_ctus * sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
    HIP_TRY(ctx, hipStreamSynchronize(cs));
    for (int k = 0; k < n; ++k)
        for (int p = 0; p < 3; ++p) out[k].satd[p] = sums[(size_t)k].satd[p];
    return WRENC_GPU_OK;
}

int wrenc_gpu_download_rate_hist(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_rate_hist* out) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    const wrenc_gpu_config& c = ctx->cfg;
    if (const int rc = check_slots(ctx, first_slot, n, 1, "slot range out of bounds")) return rc;
    HIP_TRY(ctx, hipSetDevice(c.device));
    static_assert(sizeof(RateHistCounts) == sizeof(wrenc_rate_hist), "the device's table is the ABI's");
    const size_t per_pic = (size_t)cplx_waves(c.width, c.height);
    if (!ctx->d_rpartial) HIP_TRY(ctx, ctx->d_rpartial.alloc((size_t)c.n_slots * per_pic));
    if (!ctx->d_rsums) HIP_TRY(ctx, ctx->d_rsums.alloc((size_t)c.n_slots));
    // on the copy stream: behind the slots' uploads and behind no search, as the complexity pass
    hipStream_t cs = ctx->copy_stream.get();
    const size_t waves = (size_t)n * per_pic;
    hipLaunchKernelGGL(rate_hist_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, cs, ctx->d_slots.get(), first_slot, n, c.width, c.height,
                       ctx->d_rpartial.get());
    hipLaunchKernelGGL(rate_hist_finish_kernel, dim3(n), dim3(192), 0, cs, ctx->d_rpartial.get(), c.width, c.height, ctx->d_rsums.get());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_rsums.get(), (size_t)n * sizeof(wrenc_rate_hist), hipMemcpyDeviceToHost, cs));
    HIP_TRY(ctx, hipStreamSynchronize(cs));
    return WRENC_GPU_OK;
}

int wrenc_gpu_rate_hist_bin(int magnitude) {
    if (magnitude < 0 || magnitude > WRENC_RATECURVE_MAX_MAGNITUDE) return WRENC_GPU_EINVAL;
    return wrenc_ratecurve_bin(magnitude);
}

int wrenc_gpu_rate_hist_host(int width, int height, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, wrenc_rate_hist* out) {
    return wrenc_ratecurve_picture(y, cb, cr, width, height, out) ? WRENC_GPU_EINVAL : WRENC_GPU_OK;
}

int wrenc_gpu_download_dist_curve(wrenc_gpu_ctx* ctx, int first_slot, int n, wrenc_dist_curve* out) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    const wrenc_gpu_config& c = ctx->cfg;
    if (const int rc = check_slots(ctx, first_slot, n, 1, "slot range out of bounds")) return rc;
    HIP_TRY(ctx, hipSetDevice(c.device));
    static_assert(sizeof(DistCurveSums) == sizeof(wrenc_dist_curve), "the device's table is the ABI's");
    const size_t per_pic = (size_t)cplx_waves(c.width, c.height);
    if (!ctx->d_dpartial) HIP_TRY(ctx, ctx->d_dpartial.alloc((size_t)c.n_slots * per_pic));
    if (!ctx->d_dsums) HIP_TRY(ctx, ctx->d_dsums.alloc((size_t)c.n_slots));
    // on the copy stream: behind the slots' uploads and behind no search, as the rate histogram
    hipStream_t cs = ctx->copy_stream.get();
    const size_t waves = (size_t)n * per_pic;
    hipLaunchKernelGGL(dist_curve_kernel, dim3((unsigned)((waves + kDcWaves - 1) / kDcWaves)), dim3(64 * kDcWaves), 0, cs, ctx->d_slots.get(),
                       first_slot, n, c.width, c.height, ctx->d_dpartial.get());
    hipLaunchKernelGGL(dist_curve_finish_kernel, dim3(n), dim3(192), 0, cs, ctx->d_dpartial.get(), c.width, c.height, ctx->d_dsums.get());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_dsums.get(), (size_t)n * sizeof(wrenc_dist_curve), hipMemcpyDeviceToHost, cs));
    HIP_TRY(ctx, hipStreamSynchronize(cs));
    return WRENC_GPU_OK;
}

int wrenc_gpu_dist_curve_host(int width, int height, const uint8_t* y, const uint8_t* cb, const uint8_t* cr, wrenc_dist_curve* out) {
    return wrenc_distcurve_picture(y, cb, cr, width, height, out) ? WRENC_GPU_EINVAL : WRENC_GPU_OK;
}

void wrenc_gpu_metrics_values(int width, int height, const wrenc_gpu_metrics* m, double psnr[4], double ssim[4]) {
    const double samples[3] = {(double)width * height, (double)(width / 2) * (height / 2), (double)(width / 2) * (height / 2)};
    const auto db = [](double mse) { return mse == 0.0 ? (double)INFINITY : 10.0 * log10(255.0 * 255.0 / mse); };
    double weighted = 0.0;
    for (int p = 0; p < 3; ++p) {
        const double mse = (double)m->sse[p] / samples[p];
        psnr[1 + p] = db(mse);
        weighted += mse * samples[p];
        ssim[1 + p] = m->ssim_sum[p] / (double)m->ssim_windows[p];
    }
    psnr[0] = db(weighted / (samples[0] + samples[1] + samples[2]));
    ssim[0] = (4.0 * ssim[1] + ssim[2] + ssim[3]) / 6.0;
}

int wrenc_gpu_download_hashes(wrenc_gpu_ctx* ctx, int first_slot, int n, int hash_type, wrenc_picture_hash* out) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    if (hash_type != WRENC_HASH_MD5 && hash_type != WRENC_HASH_CRC && hash_type != WRENC_HASH_CHECKSUM)
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_download_hashes: unknown hash type");
    if (const int rc = check_slots(ctx, first_slot, n, 2, "slot range out of bounds")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const wrenc_gpu_config& c = ctx->cfg;
    if (!ctx->hash_stream) HIP_TRY(ctx, ctx->hash_stream.create(hipStreamNonBlocking));
    if (!ctx->d_htables) { // held by the context once they are filled
        DevBuf<HashTables> t;
        HIP_TRY(ctx, t.alloc(1));
        HIP_TRY(ctx, upload_hash_tables(t.get(), ctx->hash_stream.get()));
        ctx->d_htables = std::move(t);
    }
    HIP_TRY(ctx, ctx->d_hpartial.grow((size_t)n * hash_partials(c)));
    HIP_TRY(ctx, ctx->d_hvalues.grow((size_t)n));
    // on the hash stream, behind the encode call that searched these slots and nothing later; the search of other slots
    // and the copy stream's uploads go on meanwhile
    hipStream_t hs = ctx->hash_stream.get();
    if (const int rc = wait_for_search(ctx, first_slot, n, hs)) return rc;
    ctx->hash_timed = false;
    if (ctx->stats_enabled) {
        for (HipEvent& e : ctx->hash_ev)
            if (!e) HIP_TRY(ctx, e.create());
        HIP_TRY(ctx, hipEventRecord(ctx->hash_ev[0].get(), hs));
    }
    HIP_TRY(ctx, launch_hashes(c, hs, ctx->d_slots.get(), first_slot, n, hash_type, ctx->d_htables.get(), ctx->d_hpartial.get(), ctx->d_hvalues.get()));
    if (ctx->stats_enabled) {
        HIP_TRY(ctx, hipEventRecord(ctx->hash_ev[1].get(), hs));
        ctx->hash_timed = true;
    }
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_hvalues.get(), (size_t)n * sizeof(wrenc_picture_hash), hipMemcpyDeviceToHost, hs));
    return read_overflow(ctx, hs); // (synchronises the stream)
}

int wrenc_gpu_last_hash_ms(wrenc_gpu_ctx* ctx, float* ms) {
    if (!ctx || !ms) return WRENC_GPU_EINVAL;
    if (!ctx->hash_timed) return fail(ctx, WRENC_GPU_ESTATE, "no timed hash pass: wrenc_gpu_stats_enable, then wrenc_gpu_download_hashes");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->hash_ev[0].get(), ctx->hash_ev[1].get()));
    return WRENC_GPU_OK;
}

int wrenc_gpu_recon_from_name(const char* name) {
    const int f = wrenc_recon_from_name(name);
    return f < 0 ? WRENC_GPU_EINVAL : f;
}

const char* wrenc_gpu_recon_name(int format) { return wrenc_recon_name(format); }

int wrenc_gpu_recon_layout(int format, int w, int h, struct wrenc_gpu_format_layout* out) {
    return wrenc_recon_layout(format, w, h, out) ? WRENC_GPU_EINVAL : WRENC_GPU_OK;
}

int wrenc_gpu_recon_coefficients(int matrix, int range, int out[6]) { return wrenc_recon_coefficients(matrix, range, out) ? WRENC_GPU_EINVAL : WRENC_GPU_OK; }

int wrenc_gpu_recon_convert_host(int format, int matrix, int range, int w, int h, const uint8_t* y, const uint8_t* cb, const uint8_t* cr,
                                 void* const plane[3], const size_t stride_bytes[3]) {
    if (!plane) return WRENC_GPU_EINVAL;
    uint8_t* const to[3] = {(uint8_t*)plane[0], (uint8_t*)plane[1], (uint8_t*)plane[2]};
    return wrenc_recon_convert(format, matrix, range, w, h, y, cb, cr, to, stride_bytes) ? WRENC_GPU_EINVAL : WRENC_GPU_OK;
}

namespace {

// the recon staging planes of output format `format` at the context's visible size: the frame's layout, the planes'
// pitches (dev_recon.h) and offsets, and the bytes they take
struct ReconStage {
    struct wrenc_gpu_format_layout lay;
    size_t pitch[3], off[3], bytes;
};

bool recon_stage(const wrenc_gpu_ctx* ctx, int format, ReconStage& r) {
    const int vw = ctx->vis_w, vh = ctx->vis_h;
    if (wrenc_recon_layout(format, vw, vh, &r.lay)) return false;
    r.bytes = 0;
    for (int p = 0; p < 3; ++p) {
        r.pitch[p] = r.off[p] = 0;
        if (p >= r.lay.n_planes) continue;
        r.pitch[p] = recon_stage_pitch(format, p, wrenc_recon_is_rgb(format) || !p ? vw : vw / 2);
        r.off[p] = r.bytes;
        r.bytes += r.pitch[p] * r.lay.rows[p];
    }
    return true;
}

// What the two recon entries share: the checks, the staging planes, the wait for the slot's search and the kernel, all on
// the recon stream; `r` is then what the caller's planes are copied from.  device: each plane written must be memory of the
// context's device.
int recon_to_stage(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_recon_format* fmt, void* const plane[3], const size_t stride_bytes[3], bool device,
                   ReconStage& r) {
    if (!fmt || !plane || !stride_bytes) return fail(ctx, WRENC_GPU_EINVAL, "null format, plane list or stride list");
    if (const int rc = check_slots(ctx, slot, 1, 2, "bad slot")) return rc;
    int k[6] = {0, 0, 0, 0, 0, 0};
    if (!wrenc_recon_valid(fmt->format) || (wrenc_recon_is_rgb(fmt->format) && wrenc_recon_coefficients(fmt->matrix, fmt->range, k)))
        return fail(ctx, WRENC_GPU_EINVAL, "unknown recon format, matrix or range");
    if (!recon_stage(ctx, fmt->format, r)) return fail(ctx, WRENC_GPU_EINVAL, "the recon formats need pictures of an even size, at least 16x16");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    for (int p = 0; p < r.lay.n_planes; ++p) {
        if (!plane[p]) return fail(ctx, WRENC_GPU_EINVAL, "null plane");
        if (stride_bytes[p] < r.lay.row_bytes[p]) return fail(ctx, WRENC_GPU_EINVAL, "stride smaller than row");
        if (!device) continue;
        hipPointerAttribute_t at = {};
        const hipError_t e = hipPointerGetAttributes(&at, plane[p]);
        if (e != hipSuccess) (void)hipGetLastError(); // a pointer the runtime does not know: plain host memory
        if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->cfg.device)
            return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_download_recon_device: a plane is not memory of the context's device (host planes go through wrenc_gpu_download_recon)");
    }
    if (!ctx->recon_stream) HIP_TRY(ctx, ctx->recon_stream.create(hipStreamNonBlocking));
    if (!ctx->ev_recon_read) HIP_TRY(ctx, ctx->ev_recon_read.create(hipEventDisableTiming));
    if (!ctx->d_recon) { // once, with room for every output format: a later call frees nothing under work in flight
        size_t most = 0;
        for (int f = 0; f < WRENC_RECON_COUNT; ++f) {
            ReconStage s;
            if (recon_stage(ctx, f, s) && s.bytes > most) most = s.bytes;
        }
        const hipError_t e = ctx->d_recon.alloc(most);
        if (e != hipSuccess)
            return fail(ctx, e == hipErrorOutOfMemory ? WRENC_GPU_ENOMEM : WRENC_GPU_EHIP, std::string("recon staging planes: ") + hipGetErrorString(e));
    }
    // on the recon stream, behind the encode call that searched the slot and nothing later, and behind the copies of the
    // call before (same stream); the search of other slots and the copy stream's uploads go on meanwhile
    hipStream_t rs = ctx->recon_stream.get();
    if (const int rc = wait_for_search(ctx, slot, 1, rs)) return rc;
    const wrenc_gpu_config& c = ctx->cfg;
    const PicBufs& b = ctx->slots[slot];
    ReconArgs a = {};
    for (int p = 0; p < 3; ++p) {
        a.rec[p] = b.rec[p];
        a.dst_off[p] = r.off[p];
        a.dst_pitch[p] = (int)r.pitch[p];
    }
    a.dst = ctx->d_recon.get();
    a.W = c.width;
    a.w = ctx->vis_w;
    a.h = ctx->vis_h;
    if (wrenc_recon_is_rgb(fmt->format)) {
        a.cy16 = 16 * k[0];
        a.yk = (1 << 17) - 16 * k[0] * k[5];
        a.rv = k[1], a.gu = k[2], a.gv = k[3], a.bu = k[4];
        switch (fmt->format) {
        case WRENC_RGB_RGB24: launch_recon_rgb<WRENC_RGB_RGB24>(a, rs); break;
        case WRENC_RGB_BGR24: launch_recon_rgb<WRENC_RGB_BGR24>(a, rs); break;
        case WRENC_RGB_RGB0: launch_recon_rgb<WRENC_RGB_RGB0>(a, rs); break;
        case WRENC_RGB_BGR0: launch_recon_rgb<WRENC_RGB_BGR0>(a, rs); break;
        default: launch_recon_rgb<WRENC_RGB_GBRP>(a, rs); break;
        }
    } else {
        const bool pairs = fmt->format == WRENC_RECON_NV12;
        a.row_blocks[0] = (a.h + kReconRows - 1) / kReconRows;
        a.row_blocks[1] = (a.h / 2 + kReconRows - 1) / kReconRows;
        const dim3 grid((unsigned)((a.w + 64 * kReconGroup - 1) / (64 * kReconGroup)), (unsigned)(a.row_blocks[0] + (pairs ? 1 : 2) * a.row_blocks[1]));
        if (pairs)
            hipLaunchKernelGGL(recon_yuv_kernel<true>, grid, dim3(64, kReconRows), 0, rs, a);
        else
            hipLaunchKernelGGL(recon_yuv_kernel<false>, grid, dim3(64, kReconRows), 0, rs, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return WRENC_GPU_OK;
}

} // namespace

int wrenc_gpu_download_recon(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_recon_format* format, void* const plane[3], const size_t stride_bytes[3]) {
    if (!ctx) return WRENC_GPU_EINVAL;
    ReconStage r;
    if (const int rc = recon_to_stage(ctx, slot, format, plane, stride_bytes, false, r)) return rc;
    hipStream_t rs = ctx->recon_stream.get();
    // the visible picture in the output format, once over the bus
    for (int p = 0; p < r.lay.n_planes; ++p)
        HIP_TRY(ctx, hipMemcpy2DAsync(plane[p], stride_bytes[p], ctx->d_recon.get() + r.off[p], r.pitch[p], r.lay.row_bytes[p], r.lay.rows[p],
                                      hipMemcpyDeviceToHost, rs));
    return read_overflow(ctx, rs); // (synchronises the stream)
}

int wrenc_gpu_download_recon_device(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_recon_format* format, void* const plane[3],
                                    const size_t stride_bytes[3], void* consumer_stream) {
    if (!ctx) return WRENC_GPU_EINVAL;
    ReconStage r;
    if (const int rc = recon_to_stage(ctx, slot, format, plane, stride_bytes, true, r)) return rc;
    hipStream_t rs = ctx->recon_stream.get(), consumer = (hipStream_t)consumer_stream;
    if (!ctx->ev_consumer) HIP_TRY(ctx, ctx->ev_consumer.create(hipEventDisableTiming));
    if (!ctx->ev_recon_copied) HIP_TRY(ctx, ctx->ev_recon_copied.create(hipEventDisableTiming));
    // no host wait: an encode call queued later must not rewrite the slot's planes under the kernel
    HIP_TRY(ctx, hipEventRecord(ctx->ev_recon_read.get(), rs));
    ctx->recon_read_pending = true;
    // the copies into the caller's planes go on only behind what the consumer stream has queued so far (the kernel does
    // not wait: it writes the library's staging planes) ...
    HIP_TRY(ctx, hipEventRecord(ctx->ev_consumer.get(), consumer));
    HIP_TRY(ctx, hipStreamWaitEvent(rs, ctx->ev_consumer.get(), 0));
    for (int p = 0; p < r.lay.n_planes; ++p)
        HIP_TRY(ctx, hipMemcpy2DAsync(plane[p], stride_bytes[p], ctx->d_recon.get() + r.off[p], r.pitch[p], r.lay.row_bytes[p], r.lay.rows[p],
                                      hipMemcpyDeviceToDevice, rs));
    // ... and what the consumer stream queues from now on runs behind them
    HIP_TRY(ctx, hipEventRecord(ctx->ev_recon_copied.get(), rs));
    HIP_TRY(ctx, hipStreamWaitEvent(consumer, ctx->ev_recon_copied.get(), 0));
    return WRENC_GPU_OK;
}

int wrenc_gpu_test_load_recon(wrenc_gpu_ctx* ctx, int slot, const uint8_t* y, const uint8_t* cb, const uint8_t* cr) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (slot < 0 || slot >= ctx->cfg.n_slots || !y || !cb || !cr) return fail(ctx, WRENC_GPU_EINVAL, "bad slot or null plane");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    const PicBufs& b = ctx->slots[slot];
    const uint8_t* from[3] = {y, cb, cr};
    for (int p = 0; p < 3; ++p) HIP_TRY(ctx, hipMemcpy(b.rec[p], from[p], plane_bytes(ctx->cfg, p, 1), hipMemcpyHostToDevice));
    ctx->state[slot] = 2;
    return WRENC_GPU_OK;
}

int wrenc_gpu_test_load_record(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_picture* rec) {
    if (!ctx || !rec || !rec->cu_log2_size || !rec->luma_mode || !rec->chroma_mode || !rec->lev_y || !rec->lev_cb || !rec->lev_cr)
        return WRENC_GPU_EINVAL;
    if (slot < 0 || slot >= ctx->cfg.n_slots) return fail(ctx, WRENC_GPU_EINVAL, "bad slot");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    const wrenc_gpu_config& c = ctx->cfg;
    const PicBufs& b = ctx->slots[slot];
    const size_t n4 = (size_t)(c.width / 4) * (c.height / 4), n8 = (size_t)(c.width / 8) * (c.height / 8);
    const int16_t* lev[3] = {rec->lev_y, rec->lev_cb, rec->lev_cr};
    for (int k = 0; k < 3; ++k) HIP_TRY(ctx, hipMemcpy(b.lev[k], lev[k], plane_bytes(c, k, 2), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(b.cu_log2, rec->cu_log2_size, n4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(b.luma_mode, rec->luma_mode, n4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(b.chroma_mode, rec->chroma_mode, n8, hipMemcpyHostToDevice));
    // (the slot's "these 4x4 blocks may be non-zero" bookkeeping no longer matches its planes: every block may be)
    HIP_TRY(ctx, hipMemset(b.lev_dirty, 0xFF, (size_t)ctx->ctu_cols * ctx->ctu_rows * 4 * sizeof(uint32_t)));
    ctx->state[slot] = 2;
    return WRENC_GPU_OK;
}

void wrenc_gpu_expand_levels(int width, int height, const uint32_t* mask, const int16_t* payload, int16_t* lev_y, int16_t* lev_cb,
                             int16_t* lev_cr) {
    const size_t wh = (size_t)width * height;
    memset(lev_y, 0, wh * sizeof(int16_t));
    memset(lev_cb, 0, wh / 4 * sizeof(int16_t));
    memset(lev_cr, 0, wh / 4 * sizeof(int16_t));
    const int bw = width / 4, bh = height / 4;
    const size_t nl = (size_t)bw * bh, ncb = nl / 4, total = nl + 2 * ncb;
    size_t at = 0;
    for (size_t w0 = 0; w0 < total; w0 += 32) {
        uint32_t m = mask[w0 >> 5];
        while (m) {
            const int bit = __builtin_ctz(m);
            m &= m - 1;
            const size_t b = w0 + (size_t)bit;
            if (b >= total) break;
            int16_t* plane = lev_y;
            size_t pb_ = b;
            int pw = bw, stride = width;
            if (b >= nl) {
                const size_t cidx = b - nl;
                const int pl = cidx >= ncb ? 1 : 0;
                pb_ = cidx - (size_t)pl * ncb;
                pw = bw / 2;
                stride = width / 2;
                plane = pl ? lev_cr : lev_cb;
            }
            const size_t by = pb_ / (size_t)pw, bx = pb_ - by * (size_t)pw;
            int16_t* d = plane + (4 * by) * (size_t)stride + 4 * bx;
            const int16_t* s = payload + 16 * at++;
            for (int r = 0; r < 4; ++r) memcpy(d + (size_t)r * stride, s + 4 * r, 4 * sizeof(int16_t));
        }
    }
}

void* wrenc_gpu_alloc_host(wrenc_gpu_ctx* ctx, size_t bytes) {
    if (!ctx || bytes == 0) return nullptr;
    void* p = nullptr;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); // (not to be reported by the next launch check: the caller may go on without the memory)
        (void)fail(ctx, WRENC_GPU_ENOMEM, "hipHostMalloc failed");
        return nullptr;
    }
    return p;
}

void wrenc_gpu_free_host(wrenc_gpu_ctx* ctx, void* p) {
    if (ctx && p) (void)hipHostFree(p);
}

} // extern "C"
