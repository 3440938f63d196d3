// wrenc_gpu.hip -- kernels + C ABI (include/wrenc_gpu.h) of the MI355X all-intra
// RD-search path.  Built for gfx950 only, together with the block tests' unit (wrenc_gpu_test.hip: the kernels and entries
// of include/wrenc_gpu_test.h; a code object of its own, so nothing there reaches the code of the kernels here):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -o libwrenc_gpu.so wrenc_gpu.hip wrenc_gpu_test.hip
//
// Scheduling: a picture's CTUs depend on their left, above-left, above and
// above-right neighbours (encoder_context.rs:934-948), so CTU (r, c) can run once
// every CTU on anti-diagonal c + 2r - 1 is done.  One launch processes one
// anti-diagonal of every picture of the batch (one wave per CTU); stream order
// between launches is the only synchronisation between CTUs.  (The one in-kernel
// wait is a workgroup's acquire of a scratch region from a bitmap that always has
// more regions than workgroups can be resident, see ctu_search_kernel.)
#include "gpu_ctx.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// Scratch regions for resident workgroups (WPB x kWaveScratch bytes each: the saved reconstructions of dev_search.h
// copy_block), handed out through a bitmap.  The pool covers the workgroups that can be resident at once, not the
// ones of a launch, and it is PARTITIONED BY XCD: a workgroup takes the lowest free region of the partition of the XCD
// it runs on (s_getreg XCC_ID).  The regions in use on an XCD are then the same 160 or so (32 CUs x kWorkgroupsPerCU)
// for the whole run, written and re-read through that XCD's own L2 only: about 2 MB that can stay in the 4 MB L2
// instead of going out to the fabric with every save, and no other L2 ever holds a line of them, so giving a region
// back needs no L2 write-back.  (Round 2 picked a region anywhere in a pool of 4096 from a hash of the workgroup
// index and ran __threadfence() = buffer_wbl2 sc1 + buffer_inv sc1 at every workgroup's end: every saved
// reconstruction went out to memory.)  A region is only ever used by one workgroup at a time and nothing is read
// that the same workgroup did not write, so its contents need no hand-over.
// Should a partition ever be full (another device, another occupancy) a workgroup takes a region of the OVERFLOW
// partition, which any XCD may use and whose users write their L2 lines back before they release it, as round 2 did;
// the word behind the bitmap counts how often that happened (wrenc_gpu_test_scratch_overflows: 0 on MI355X).
constexpr int kXcdMax = 8;
constexpr int kRegionsPerXcd = 256;    // whole bitmap words; >= CUs per XCD x kWorkgroupsPerCU (32 x 5 = 160)
constexpr int kAffineRegions = kXcdMax * kRegionsPerXcd;
constexpr int kOverflowRegions = 2048; // >= every workgroup that can be resident, should XCC_ID not tell them apart
constexpr int kScratchSlots = kAffineRegions + kOverflowRegions;
constexpr int kSlotMapWords = kScratchSlots / 64 + 1; // + the overflow counter

__device__ __forceinline__ int xcc_id() {
    // hwreg(HW_REG_XCC_ID = 20, offset 0, size 4): the XCD this wave runs on
    return (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | ((4 - 1) << 11)) & (kXcdMax - 1));
}
// the lowest free region of bitmap words [w0, w0 + nw), or -1 if they are all taken
__device__ __forceinline__ int take_region(unsigned long long* slot_map, unsigned w0, unsigned nw) {
    for (unsigned w = w0; w < w0 + nw; ++w) {
        unsigned long long cur = __hip_atomic_load(&slot_map[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (~cur) {
            const int b = __ffsll((unsigned long long)~cur) - 1;
            const unsigned long long bit = 1ULL << b;
            const unsigned long long old = atomicOr(&slot_map[w], bit);
            if (!(old & bit)) return (int)(w * 64 + b);
            cur = old; // somebody else got it: look again in what the word held then
        }
    }
    return -1;
}
// (The region number travels through a cell of wave 0's LDS that the search only uses later.)
__device__ __forceinline__ int acquire_scratch(unsigned long long* slot_map) {
    if (threadIdx.x == 0) {
        int slot = take_region(slot_map, (unsigned)xcc_id() * (kRegionsPerXcd / 64), kRegionsPerXcd / 64);
        if (slot < 0) {
            atomicAdd(&slot_map[kScratchSlots / 64], 1ULL);
            // the overflow partition has a region for every workgroup that can be resident: a free one turns up
            while (slot < 0) slot = take_region(slot_map, kAffineRegions / 64, kOverflowRegions / 64);
        }
        SHW[0].slot_xfer = slot;
    }
    __syncthreads();
    const int scratch_slot = uni(SHW[0].slot_xfer);
    __syncthreads(); // everybody has read the cell before the search may overwrite it
    return scratch_slot;
}
// give the scratch region back once every wave is through with it
__device__ __forceinline__ void release_scratch(unsigned long long* slot_map, int scratch_slot) {
    if (scratch_slot >= kAffineRegions) __threadfence(); // overflow partition: the next user may sit behind another L2
    __syncthreads();
    if (threadIdx.x == 0) atomicAnd(&slot_map[scratch_slot >> 6], ~(1ULL << (scratch_slot & 63)));
}

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

// Wave schedule: one workgroup = the same CTU of WPB consecutive pictures, one wave each.
// D3: built for max-split-depth 3 (with the 4x4 leaves of split 8x8 CUs) or for the smaller depths (without)
// groups: NULL for a call at one QP (block k); else the call's groups from this launch's first one (k unused).
template <bool D3>
__global__ __launch_bounds__(64 * WPB, 5) void ctu_search_kernel(const DevConst* __restrict__ k,
                                                              const PicBufs* __restrict__ slots, int first_slot,
                                                              int n_pictures, int diag, int r_min, int count,
                                                              uint8_t* pred_scratch, unsigned long long* slot_map,
                                                              unsigned long long* mismatch, int* overflow,
                                                              const CallGroup* __restrict__ groups) {
    const int scratch_slot = acquire_scratch(slot_map);
    const int group = blockIdx.x / count;
    const int j = blockIdx.x - group * count;
    const int row = r_min + j;
    const int col = diag - 2 * row;
    int pic = group * WPB + WAVE;
    if (groups) {
        k = groups[group].k;
        n_pictures = group * WPB + groups[group].n_real;
    }
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    c.mismatch = mismatch;
    c.write = pic < n_pictures ? 1 : 0;
    c.trace = c.write;
    c.store = c.write;
    c.solo = 0;
    c.member = 0;
    if (pic >= n_pictures) pic = n_pictures - 1; // padding wave: same work, no stores
    const PicBufs pb = slots[first_slot + pic];
    c.org = (const GLOBAL_AS uint8_t*)pb.org_t + (size_t)(row * c.k->ctu_cols + col) * kOrgTile;
    c.W = c.k->W;
    c.WH = c.k->W * c.k->H;
    c.pred_scratch = nullptr;
    c.slots = (GLOBAL_AS uint8_t*)(pred_scratch + ((size_t)scratch_slot * WPB + WAVE) * kWaveScratch);
    int ovf = 0;
    encode_ctu<false, D3>(c, pb, col, row, &ovf);
    if (ovf && LANE == 0) atomicOr(overflow, 1);
    release_scratch(slot_map, scratch_slot);
}

// Team schedule: one workgroup = the same CTU of WPB / kTeam consecutive pictures, kTeam waves each
// (dev_search.h, leaf_step_team).  For encode calls with too few pictures to fill the GPU one wave per CTU.
// (A mixed-QP call launches it once per QP class of a lane: reading a group's block here, as the wave kernel does,
// costs this kernel 12 VGPRs.)
template <bool D3>
__global__ __launch_bounds__(64 * WPB, 5) void ctu_search_team_kernel(const DevConst* __restrict__ k,
                                                                   const PicBufs* __restrict__ slots, int first_slot,
                                                                   int n_pictures, int diag, int r_min, int count,
                                                                   uint8_t* pred_scratch, unsigned long long* slot_map,
                                                                   unsigned long long* mismatch, int* overflow) {
    const int scratch_slot = acquire_scratch(slot_map);
    constexpr int kTeams = WPB >= kTeam ? WPB / kTeam : 1; // (WPB < kTeam: occupancy experiments, wave schedule only)
    const int group = blockIdx.x / count;
    const int j = blockIdx.x - group * count;
    const int row = r_min + j;
    const int col = diag - 2 * row;
    int pic = group * kTeams + WAVE / kTeam;
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    c.mismatch = mismatch;
    c.member = WAVE & (kTeam - 1);
    c.trace = pic < n_pictures ? 1 : 0;
    c.write = (c.trace && c.member == 0) ? 1 : 0; // one member stores the picture's results
    c.store = c.trace;                            // (every member stores the levels of its share of the final pass)
    c.solo = 1;
    if (pic >= n_pictures) pic = n_pictures - 1;  // padding team: same work, no stores
    const PicBufs pb = slots[first_slot + pic];
    c.org = (const GLOBAL_AS uint8_t*)pb.org_t + (size_t)(row * k->ctu_cols + col) * kOrgTile;
    c.W = k->W;
    c.WH = k->W * k->H;
    c.pred_scratch = nullptr;
    c.slots = (GLOBAL_AS uint8_t*)(pred_scratch + ((size_t)scratch_slot * WPB + WAVE) * kWaveScratch);
    int ovf = 0;
    encode_ctu<true, D3>(c, pb, col, row, &ovf);
    if (ovf && LANE == 0) atomicOr(overflow, 1);
    if (SHT.lvb.pad_ && LANE == 0) atomicOr(overflow, 2); // a meeting point of the level schedule timed out
    release_scratch(slot_map, scratch_slot);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace {

thread_local std::string g_create_error;

// An encode call splits its pictures over this many HIP streams.  Pictures are independent, so the
// streams' anti-diagonal launches overlap and one lane's tail (partially filled GPU) is filled by
// the other lanes' work.
#ifndef WRENC_ENCODE_LANES
#define WRENC_ENCODE_LANES 4
#endif
constexpr int kEncodeLanes = WRENC_ENCODE_LANES;


// AUTO picks the team schedule for an anti-diagonal while one wave per CTU would leave more than half of the
// GPU's wave slots empty (slots: CUs x kWorkgroupsPerCU x WPB = 5120 on an MI355X).  Measured (DESIGN.md section 5,
// gpurun_out/r3b): threshold at 25 / 50 / 75 / 100 % of the slots gives 282 / 306 / 270 / 269 frames/s at 1080p depth 2
// with 128 pictures, 54.4 / 55.9 / 53.8 / 48.9 at 3840x2176 depth 3 with 128; 50 % is best at every batch size tried.
// End of round 3 (level schedule at every depth, leaf searches a third faster): at max-split-depth 3, where all four
// members of a team have a tree level of their own, 65 % is better at every batch size between 30 and 240 pictures of
// 3840x2176 (60 pictures: 89.0 against 86.1 frames/s; 90: 102.6 / 100.9; 128: 115.8 / 114.5; 7680x4320, 32 pictures:
// 23.2 / 22.5; gpurun_out/s69, s70); at depth 2 it is 50 % still (128 pictures of 1080p: 459 against 454 at 65 %).
constexpr int kTeamBelowSlotsPct = 50, kTeamBelowSlotsPctDepth3 = 65;
// what plan_encode (encode_plan.h) is given of this build
constexpr PlanBuild kPlanBuild = {WPB, kTeam, kEncodeLanes, kTeamBelowSlotsPct, kTeamBelowSlotsPctDepth3};
static_assert(kPlanAuto == WRENC_GPU_SCHEDULE_AUTO && kPlanWave == WRENC_GPU_SCHEDULE_WAVE && kPlanTeam == WRENC_GPU_SCHEDULE_TEAM,
              "encode_plan.h restates wrenc_gpu_schedule");

// DCT-2 integer cosines c[j] ~ 64*sqrt(2)*cos(j*pi/128), H.266 8.7.4.5
// (the reference's 64-point matrix, transformer.rs:934-1191, is row k = c[(2n+1)k])
const int kCos[65] = {64, 91, 90, 90, 90, 90, 90, 90, 89, 88, 88, 87, 87, 86, 85, 84, 83, 83, 82, 81, 80, 79,
                      78, 77, 75, 73, 73, 71, 70, 69, 67, 65, 64, 62, 61, 59, 57, 56, 54, 52, 50, 48, 46, 44,
                      43, 41, 38, 37, 36, 33, 31, 28, 25, 24, 22, 20, 18, 15, 13, 11, 9,  7,  4,  2,  0};

int dct64(int k, int n) {
    int t = ((2 * n + 1) * k) % 256;
    if (t > 128) t = 256 - t;
    return t > 64 ? -kCos[128 - t] : kCos[t];
}

// H.266 Table 24 (common.rs:145) and Table 25 fC (common.rs:153)
const int16_t kIntraAngle[95] = {
    512, 341, 256, 171, 128, 102, 86,  73,  64,  57,  51,  45,  39,  35,  0,   0,   32,  29,  26,
    23,  20,  18,  16,  14,  12,  10,  8,   6,   4,   3,   2,   1,   0,   -1,  -2,  -3,  -4,  -6,
    -8,  -10, -12, -14, -16, -18, -20, -23, -26, -29, -32, -29, -26, -23, -20, -18, -16, -14, -12,
    -10, -8,  -6,  -4,  -3,  -2,  -1,  0,   1,   2,   3,   4,   6,   8,   10,  12,  14,  16,  18,
    20,  23,  26,  29,  32,  35,  39,  45,  51,  57,  64,  73,  86,  102, 128, 171, 256, 341, 512};
const int8_t kFC[32][4] = {
    {0, 64, 0, 0},    {-1, 63, 2, 0},   {-2, 62, 4, 0},   {-2, 60, 7, -1},  {-2, 58, 10, -2}, {-3, 57, 12, -2},
    {-4, 56, 14, -2}, {-4, 55, 15, -2}, {-4, 54, 16, -2}, {-5, 53, 18, -2}, {-6, 52, 20, -2}, {-6, 49, 24, -3},
    {-6, 46, 28, -4}, {-5, 44, 29, -4}, {-4, 42, 30, -4}, {-4, 39, 33, -4}, {-4, 36, 36, -4}, {-4, 33, 39, -4},
    {-4, 30, 42, -4}, {-4, 29, 44, -5}, {-4, 28, 46, -6}, {-3, 24, 49, -6}, {-2, 20, 52, -6}, {-2, 18, 53, -5},
    {-2, 16, 54, -4}, {-2, 15, 55, -4}, {-2, 14, 56, -4}, {-2, 12, 57, -3}, {-2, 10, 58, -2}, {-1, 7, 60, -2},
    {0, 4, 62, -2},   {0, 2, 63, -1}};

constexpr void diag_scan(int lw, int lh, uint8_t (*out)[2]) { // ctu.rs:54-77
    const int bw = 1 << lw, bh = 1 << lh;
    int i = 0, x = 0, y = 0;
    bool stop = false;
    while (!stop) {
        while (y >= 0) {
            if (x < bw && y < bh) {
                out[i][0] = (uint8_t)x;
                out[i][1] = (uint8_t)y;
                ++i;
            }
            --y;
            ++x;
        }
        y = x;
        x = 0;
        if (i >= bw * bh) stop = true;
    }
}

// The quantisers compute the scan (dev_scan.h) where wrenc_gpu_config below fills DevConst::scan_idx for everyone else:
// the closed form against that construction -- diag_scan and the fill loop, as a constant expression -- for every
// position of every block size.  A wrong formula does not build.
constexpr bool scan_closed_form_holds() {
    for (int idx = 0; idx < 4; ++idx) {
        const int lg = idx + 2, n = 1 << lg, nsb = 1 << (2 * lg - 4);
        uint8_t d4[16][2] = {}, dsb[64][2] = {};
        diag_scan(2, 2, d4);
        diag_scan(idx, idx, dsb);
        for (int p = 0; p < n * n; ++p) {
            const int sb = nsb - 1 - (p >> 4), sp = 15 - (p & 15);
            const int x = (dsb[sb][0] << 2) + d4[sp][0];
            const int y = (dsb[sb][1] << 2) + d4[sp][1];
            if (wrenc::scan_raster(lg, p) != y * n + x) return false;
            if (wrenc::scan_sb_origin(lg, p >> 4) + wrenc::scan_nib_offset(lg, (int)wrenc::scan_nibs_from(p & 15) & 15) != y * n + x) return false;
            const int org = wrenc::scan_sb_origin(lg, p >> 4); // ... and the forms the quantisers take the origin in
            if (wrenc::scan_word_origin(wrenc::scan_batch_word(lg, p >> 6), (p >> 4) & 3) != org) return false;
            if (lg == 3 && wrenc::scan_sb_origin_ct<3>(p >> 4) != org) return false;
            if (lg == 4 && wrenc::scan_sb_origin_ct<4>(p >> 4) != org) return false;
        }
    }
    return true;
}
static_assert(scan_closed_form_holds(), "dev_scan.h: the closed form differs from the scan table's construction");

} // namespace

// (gpu_ctx.h: shared with the block tests' unit)
int fail(wrenc_gpu_ctx* ctx, int code, const std::string& msg) {
    if (ctx)
        ctx->err = msg;
    else
        g_create_error = msg;
    return code;
}

size_t plane_bytes(const wrenc_gpu_config& c, int comp, size_t elem) {
    const size_t w = comp ? c.width / 2 : c.width, h = comp ? c.height / 2 : c.height;
    return w * h * elem;
}

namespace {

// ---- the steps the read-back entry points share (wrenc_gpu_sync, wrenc_gpu_download, _download_compact, _download_tokens) ----

// slots first .. first + n - 1 exist (else WRENC_GPU_EINVAL with `range_msg`) and are in state `min_state` at least:
// 1 uploaded, 2 searched
int check_slots(wrenc_gpu_ctx* ctx, int first, int n, int min_state, const char* range_msg) {
    if (first < 0 || n < 1 || first + n > ctx->cfg.n_slots) return fail(ctx, WRENC_GPU_EINVAL, range_msg);
    for (int s = first; s < first + n; ++s)
        if (ctx->state[s] < min_state)
            return fail(ctx, WRENC_GPU_ESTATE, min_state == 2 ? "slot has not been encoded" : "slot has no uploaded picture");
    return WRENC_GPU_OK;
}

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

// DevConst::head_rng: the coefficients that do not end the head proof's region, and those with a quotient below 2, as one
// interval around zero each (dev_quant.h: head_alpha, quotient -- the same integer arithmetic here on the host, over
// every 16-bit coefficient; test_head_ranges_kernel holds the result against the device functions).  An interval that
// stops at the first coefficient that fails can only be too narrow, which costs a longer walk, never a wrong level.
void fill_head_ranges(DevConst& k) {
    const int ldq1 = (int32_t)k.ldq[1], ldq2 = (int32_t)k.ldq[2], ldq3 = (int32_t)k.ldq[3]; // (the 32-bit table of the kernels' LDS)
    for (int idx = 0; idx < 4; ++idx) {
        const int sh = idx + 2 + 4, off = (1 << sh) >> 1, lsc = k.lsc;
        const int dp[4] = {0, (lsc + off) >> sh, (2 * lsc + off) >> sh, (3 * lsc + off) >> sh};
        const int dn[4] = {0, (-lsc + off) >> sh, (-2 * lsc + off) >> sh, (-3 * lsc + off) >> sh};
        const auto quot = [&](int tc) {
            int S = (int)((unsigned)tc << sh) - off;
            if (tc < 0) S = -S;
            return tc == 0 ? 0 : (int)((uint32_t)(((uint64_t)(uint32_t)S * k.div_magic) >> 32) >> k.div_shift);
        };
        const auto bad = [&](int tc, bool dcn) {
            const int qd = quot(tc);
            const bool neg = tc < 0;
            const int d1 = abs(tc - (neg ? dn[1] : dp[1])), d2 = abs(tc - (neg ? dn[2] : dp[2])), d3 = abs(tc - (neg ? dn[3] : dp[3]));
            const int d1o = abs(tc - (neg ? dp[1] : dn[1]));
            const int c0tz = 128 * abs(tc);
            const int c0d0 = c0tz + ldq1;
            const int c1d0 = 128 * d2 + ldq2;
            const int c0d1 = dcn ? 128 * d1o + ldq1 : (qd ? 128 * d1 + ldq2 : c0d0);
            const int c1d1 = (qd && !dcn) ? 128 * d3 + ldq3 : 128 * d1 + ldq2;
            int alpha = c1d0 - c0tz;
            int beta = std::min(std::min(c0d0, c0d1), c1d1) - c0tz;
            if (tc == 0) {
                alpha = 1 << 28;
                beta = ldq1;
            }
            return qd >= 2 || alpha < 0 || beta < 0 || ldq1 < 0;
        };
        const auto interval = [&](int32_t* r, auto&& fails) { // r[0] = -lowest, r[1] = how many: the run of passing coefficients around 0
            r[0] = r[1] = 0;
            if (fails(0)) return;
            int tp = 0, tn = 0;
            while (tp < 32767 && !fails(tp + 1)) ++tp;
            while (tn < 32768 && !fails(-(tn + 1))) ++tn;
            r[0] = tn;
            r[1] = tp + tn + 1;
        };
        interval(&k.head_rng[idx][0], [&](int tc) { return bad(tc, false); });
        interval(&k.head_rng[idx][2], [&](int tc) { return bad(tc, true); });
        interval(&k.head_rng[idx][4], [&](int tc) { return quot(tc) >= 2; });
    }
}

// DevConst::avail_tab: the reference's availability rules (ctu.rs:2083-2188, encoder_context.rs:918-956 -- the same
// arithmetic as above_right_avail / below_left_avail / nb_avail of dev_common.h) evaluated on the host for a CTU in the
// middle of a 3 x 3-CTU picture, every block position and size.
void fill_avail_tab(DevConst& k) {
    const int W = 96, H = 96, ctu_x = 32, ctu_y = 32;
    const auto above_right = [&](int bx, int by, int lg) {
        for (;;) {
            const int n = 1 << lg;
            if (ctu_x + bx + n >= W) return false;
            if (lg == 5) return ctu_y > 0 && ctu_x + 32 < W;
            const int px = bx & ~(2 * n - 1), py = by & ~(2 * n - 1);
            if (bx == px && by == py) return ctu_y + by > 0;
            if (by == py) {
                bx = px;
                by = py;
                lg += 1;
                continue;
            }
            return bx == px;
        }
    };
    const auto below_left = [&](int bx, int by, int lg) {
        for (;;) {
            const int n = 1 << lg;
            if (ctu_y + by + n >= H) return false;
            if (lg == 5) return false;
            const int px = bx & ~(2 * n - 1), py = by & ~(2 * n - 1);
            if (px < bx) return false;
            if (by + n < py + 2 * n) return ctu_x + bx > 0;
            bx = px;
            by = py;
            lg += 1;
        }
    };
    for (int lg = 2; lg <= 5; ++lg)
        for (int by = 0; by < 32; by += 4)
            for (int bx = 0; bx < 32; bx += 4) {
                int avm = 0;
                if (!(bx & ((1 << lg) - 1)) && !(by & ((1 << lg) - 1))) {
                    const int tn = 1 << lg, gx = ctu_x + bx, gy = ctu_y + by;
                    const bool ar = above_right(bx, by, lg), bl = below_left(bx, by, lg);
                    const auto nb = [&](int xn, int yn) {
                        return xn >= 0 && yn >= 0 && xn < W && yn < H && ((xn >> 5) <= (gx >> 5) || (yn >> 5) < (gy >> 5)) &&
                               (yn >> 5) < (gy >> 5) + 1 && (xn < gx + tn || ar) && (yn < gy + tn || bl);
                    };
                    avm = (nb(gx - 1, gy + tn) ? 1 : 0) | (nb(gx - 1, gy) ? 2 : 0) | (nb(gx - 1, gy - 1) ? 4 : 0) | (nb(gx, gy - 1) ? 8 : 0) |
                          (nb(gx + tn, gy - 1) ? 16 : 0);
                }
                k.avail_tab[lg - 2][(by >> 2) * 8 + (bx >> 2)] = (uint8_t)avm;
            }
}

// DevConst::split_floor (dev_search.h, kSplitCut): lower bounds of what the children of a split cost, from the tables of
// this config alone.  A leaf costs (float)ssd + lambda * ((float)(level cost + header bits) / 16384) with ssd >= 0.  The
// level cost is a sum of lv_table entries (block_splitter.rs:415-460) and 0 for a block without levels, so 0 is its
// greatest lower bound when no entry is negative; the header bits are one entry of the leaf's tree type.  Conversion to
// f32, the product with a lambda >= 0 and the f32 sum are monotone, so the same expression over the smallest entry is
// <= every cost of that tree type.  A node returns its unsplit cost or the f32 sum of its children in z-order from 0.0,
// hence min(the unsplit floor, the children's floors summed the same way); a node at max-split-depth is a leaf.
// Where the tables prove nothing (a negative lv_table entry or header-bit minimum, a lambda that is not >= 0) every
// floor is 0.0, which is the sibling rule's own premise that costs are >= 0.
// DevConst::cand_floor (dev_search.h, kCandidateCut) under the same conditions: per mode class of a 4x4 DUAL_TREE_LUMA
// leaf the expression of rd_cost itself over ssd = 0 and the class's header bits alone, and the smallest of them over
// the classes only an angular mode can have; -inf where the tables prove nothing or a floor is not finite.
void fill_split_floors(const wrenc_gpu_config& cfg, DevConst& k) {
#pragma clang fp contract(off)
    for (float& f : k.split_floor) f = 0.0f;
    for (float& f : k.cand_floor) f = -INFINITY;
    k.cand_floor_ang = -INFINITY;
    for (int i = 0; i < 1024; ++i)
        if (cfg.lv_table[i] < 0) return;
    if (!(cfg.lambda_rd >= 0.0f) || !(cfg.lambda_rd_chroma >= 0.0f)) return;
    int64_t dual = INT64_MAX, single = INT64_MAX, chroma = INT64_MAX;
    for (int cls = 0; cls < 67; ++cls) dual = std::min(dual, cfg.header_bits_luma[1][0][cls]); // (a 4x4 luma leaf is never CCLM)
    for (int cc = 0; cc < 4; ++cc) {
        for (int cls = 0; cls < 67; ++cls) single = std::min(single, cfg.header_bits_luma[0][cc][cls]);
        chroma = std::min(chroma, cfg.header_bits_chroma[cc]);
    }
    if (dual < 0 || single < 0 || chroma < 0) return;
    const auto floor_of = [](float lambda, int64_t bits) {
        const float f = 0.0f + lambda * ((float)bits / 16384.0f);
        return f >= 0.0f ? f : 0.0f;
    };
    const float f4 = floor_of(cfg.lambda_rd, dual), fc = floor_of(cfg.lambda_rd_chroma, chroma);
    const float fs = floor_of(cfg.lambda_rd, single);
    k.split_floor[0] = f4;
    k.split_floor[1] = fc;
    for (int level = 2; level >= 0; --level) {
        float sum = 0.0f;
        if (level == 2)
            sum = ((((sum + f4) + f4) + f4) + f4) + fc;
        else
            for (int i = 0; i < 4; ++i) sum = sum + k.split_floor[2 + level + 1];
        k.split_floor[2 + level] = level < cfg.max_split_depth ? std::min(fs, sum) : fs;
    }
    float cand[67], ang = INFINITY;
    for (int cls = 0; cls < 67; ++cls) {
        const float lv = (float)cfg.header_bits_luma[1][0][cls] * (1.0f / 16384.0f); // (rd_cost, dev_search.h, term by term)
        const float prod = cfg.lambda_rd * lv;
        cand[cls] = (float)0ULL + prod;
        if (!std::isfinite(cand[cls])) return;
        if (cls >= 2) ang = std::min(ang, cand[cls]);
    }
    memcpy(k.cand_floor, cand, sizeof(cand));
    k.cand_floor_ang = ang;
}

} // namespace

// (gpu_ctx.h: the block tests read a config's constants too)
void fill_dev_const(const wrenc_gpu_config& cfg, DevConst& k) {
    memset(&k, 0, sizeof(k));
    fill_split_floors(cfg, k);
    k.W = cfg.width;
    k.H = cfg.height;
    k.qp = cfg.qp;
    k.max_depth = cfg.max_split_depth;
    k.ctu_cols = cfg.width / 32;
    k.ctu_rows = cfg.height / 32;
    static const int level_scale[6] = {40, 45, 51, 57, 64, 72}; // quantizer.rs:8
    k.lsc = (16 * level_scale[(cfg.qp + 1) % 6]) << ((cfg.qp + 1) / 6);
    {
        // n / lsc for n < 2^26 (|tc << sh| of a 16-bit coefficient) as mul_hi(n, m) >> s: with k = 26 + ceil(log2 lsc) and
        // m = floor(2^k / lsc) + 1 the error n (m lsc - 2^k) / (lsc 2^k) stays below 1 / lsc, and m < 2^28 fits 32 bits
        // (n itself does not depend on the QP: a 16-bit coefficient, the largest shift 8 + 5 - 5 + 1 = 9 of a 32x32 block, the rounding offset)
        static_assert((32768LL << 9) + (1 << 8) < (1LL << 26), "quotient(): |(tc << sh) - off| stays below 2^26");
        int lg = 0;
        while ((1 << lg) < k.lsc) ++lg;
        const int kk = 26 + lg;
        k.div_magic = (uint32_t)(((1ULL << kk) / (uint64_t)k.lsc) + 1);
        k.div_shift = (uint32_t)(kk - 32);
    }
    k.lambda_q = cfg.lambda_q;
    k.lambda_rd = cfg.lambda_rd;
    k.lambda_rd_chroma = cfg.lambda_rd_chroma;
    for (int i = 0; i < 1024; ++i) {
        k.ldq[i] = cfg.lambda_q * cfg.dq_table[i];
        k.lv[i] = cfg.lv_table[i];
    }
    memcpy(k.hb_luma, cfg.header_bits_luma, sizeof(k.hb_luma));
    memcpy(k.hb_chroma, cfg.header_bits_chroma, sizeof(k.hb_chroma));
    for (int idx = 0; idx < 4; ++idx) {
        const int n = 4 << idx, step = 64 / n;
        for (int u = 0; u < n; ++u)
            for (int x = 0; x < n; ++x) {
                k.dct[idx][u][x] = (int16_t)dct64(u * step, x);
                k.dct_t[idx][x][u] = (int16_t)dct64(u * step, x);
            }
    }
    diag_scan(2, 2, k.diag4);
    for (int idx = 0; idx < 4; ++idx) diag_scan(idx, idx, k.diag_sb[idx]);
    for (int idx = 0; idx < 4; ++idx) { // reverse-scan position -> raster index (ctu.rs:827-845: 4x4 sub-blocks)
        const int lg = idx + 2, n = 1 << lg, nsb = 1 << (2 * lg - 4);
        for (int p = 0; p < n * n; ++p) {
            const int sb = nsb - 1 - (p >> 4), sp = 15 - (p & 15);
            const int x = (k.diag_sb[idx][sb][0] << 2) + k.diag4[sp][0];
            const int y = (k.diag_sb[idx][sb][1] << 2) + k.diag4[sp][1];
            k.scan_idx[idx][p] = (uint16_t)(y * n + x);
        }
    }
    memcpy(k.intra_angle, kIntraAngle, sizeof(kIntraAngle));
    for (int mode = 0; mode < 67; ++mode) {
        // intraPredAngle and invAngle (intra_predictor.rs:1287-1310) of mode 2..66, one dword per mode
        const int angle = mode >= 2 ? kIntraAngle[14 + mode] : 0;
        int inv = 0;
        if (angle > 0)
            inv = (512 * 32 + angle / 2) / angle;
        else if (angle < 0)
            inv = -((512 * 32 + (-angle) / 2) / -angle);
        k.ang_tab[mode] = (int32_t)(((uint32_t)(uint16_t)(int16_t)angle) | ((uint32_t)(uint16_t)(int16_t)inv << 16));
    }
    memcpy(k.fc, kFC, sizeof(kFC));
    for (int u = 0; u < 32; ++u) // MFMA experiment: the 32-point basis as signed bytes
        for (int x = 0; x < 32; ++x) k.dct32_a[u][x] = (int8_t)dct64(u * 2, x);
    for (int v = 0; v < 32; ++v)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 16; ++j) k.dct32_p[v][h][j] = (int8_t)dct64(v * 2, 8 * (j / 4) + 4 * h + j % 4);
    int colsum[32];
    for (int n = 0; n < 32; ++n) {
        colsum[n] = 0;
        for (int i = 0; i < 32; ++i) colsum[n] += dct64(i * 2, n);
    }
    for (int y = 0; y < 32; ++y) {
        for (int i = 0; i < 32; ++i) k.idct32_b[y][i] = (int8_t)dct64(i * 2, y);
        k.idct32_k1[y] = 128 * colsum[y] + 64;
    }
    for (int x = 0; x < 32; ++x)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 16; ++j) k.idct32_p[x][h][j] = (int8_t)dct64((8 * (j / 4) + 4 * h + j % 4) * 2, x);
    for (int h = 0; h < 2; ++h)
        for (int w = 0; w < 16; ++w) k.idct32_k2[h][w] = 128 * colsum[8 * (w / 4) + 4 * h + w % 4] + 2048;
    // the 8x8 and 16x16 transforms as i8 MFMAs (DevConst::fdct_b ...)
    memset(k.fdct_b, 0, sizeof(k.fdct_b));
    memset(k.fdct16_p, 0, sizeof(k.fdct16_p));
    memset(k.fdct8_p, 0, sizeof(k.fdct8_p));
    memset(k.idct_b, 0, sizeof(k.idct_b));
    memset(k.idct16_p, 0, sizeof(k.idct16_p));
    memset(k.idct8_p, 0, sizeof(k.idct8_p));
    for (int idx = 0; idx < 2; ++idx) {
        const int n = 8 << idx, step = 64 / n;
        auto T = [&](int u, int x) { return dct64(u * step, x); };
        auto yk = [](int j, int h) { return 8 * (j / 4) + 4 * h + j % 4; };
        int s[16];
        for (int y = 0; y < n; ++y) {
            s[y] = 0;
            for (int i = 0; i < n; ++i) s[y] += T(i, y);
        }
        for (int m = 0; m < 32; ++m)
            for (int h = 0; h < 2; ++h) {
                for (int j = 0; j < 16; ++j) {
                    const int blk = n == 16 ? h : 2 * h + j / 8, x = j % n;
                    if (m / n == blk) {
                        k.fdct_b[idx][m][h][j] = (int8_t)T(m % n, x);
                        k.idct_b[idx][m][h][j] = (int8_t)T(x, m % n);
                    }
                    if (n == 16) {
                        if (j < 8 && m < 16) k.fdct16_p[m][h][j] = (int8_t)T(m, yk(j, h));
                        if (j / 8 == m / 16) k.idct16_p[m][h][j] = (int8_t)T(yk(j % 8, h), m % 16);
                    } else {
                        if (j / 4 == m / 8 && m / 8 < 3) k.fdct8_p[m][h][j] = (int8_t)T(m % 8, 4 * h + j % 4);
                        if (j < 8 && j / 4 == m / 16 && m % 16 < 8) k.idct8_p[m][h][j] = (int8_t)T(4 * h + j % 4, m % 16);
                    }
                }
                for (int w = 0; w < n / 2; ++w)
                    (n == 16 ? k.idct16_k2[h][w] : k.idct8_k2[h][w]) = 128 * s[yk(w, h)] + 2048;
            }
        for (int m = 0; m < 32; ++m) k.idct_k1[idx][m] = 128 * s[m % n] + 64;
    }
    fill_head_ranges(k);
    fill_avail_tab(k);
}

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

extern "C" {

// The RD-model constants the reference reads from --extra-params, with its defaults for the live
// (dependent quantisation + trellis) variants: block_splitter.rs:29-44,187-375,594-693,775 and
// quantizer.rs:16-19,650-683.  Types follow the reference's parse::<f64> / <f32> / <i64>.
struct RdParams {
    double lv_pow = 0.48592678233563835, lv_offset = 0.15150746310196822;               // lv_dq_trellis_table
    double quant_lv_pow = 0.5004010166085378;                                            // dq_table
    double quant_qp_div = 5.218413785332902, quant_lambda_mul = 1.2709404305806742;      // lambda of the trellis
    long long quant_lambda_offset = 11;
    float qp_div = 4.4043665f, lambda_mul = 1.1282581f;
    float non_planar_offset = 2.2153597f, mpm_idx_offset = 1.3660221f, mpm_remainder_mult = 0.5007182f,
          mpm_remainder_offset = 2.2973304f, planar_offset = 0.9626864f, header_bits = 1.1772872f,
          chroma_header_bits = 1.309252f, cclm_pow = 0.4587651f, mpm_idx_pow = 0.40271285f,
          mpm_remainder_pow = 0.34385094f, cclm_mode_idx_offset = 2.1f, non_cclm_offset = 0.89f, cclm_offset = 0.53f;
    bool has_a = false; // "a" replaces lambda_mul in the chroma cost function (block_splitter.rs:775-778)
    float a = 0.0f;
};

static void resolve_config(wrenc_gpu_config* cfg, const RdParams& p) {
    const int qp = cfg->qp;
    // block_splitter.rs:29-53 (lv_dq_trellis), quantizer.rs:16-25
    for (int i = 0; i < 1024; ++i) {
        cfg->lv_table[i] = (int64_t)(std::pow((double)i + p.lv_offset, p.lv_pow) * 16384.0);
        cfg->dq_table[i] = (int64_t)std::pow((double)(i * 16384), p.quant_lv_pow);
    }
    // quantizer.rs:650-683
    cfg->lambda_q = (int64_t)(std::pow(2.0, (double)qp / p.quant_qp_div) * p.quant_lambda_mul) + p.quant_lambda_offset;
    // block_splitter.rs:289-309,472
    cfg->lambda_rd = std::pow(2.0f, (float)qp / p.qp_div) * p.lambda_mul;
    cfg->lambda_rd_chroma = std::pow(2.0f, (float)qp / p.qp_div) * (p.has_a ? p.a : p.lambda_mul); // :775-778
    // block_splitter.rs:187-406 (dep-quant + trellis variants)
    for (int tree = 0; tree < 2; ++tree)
        for (int cc = 0; cc < 4; ++cc)
            for (int cls = 0; cls < 67; ++cls) {
                float cclm_bits;
                if (cc > 0)
                    cclm_bits = p.cclm_offset + std::pow((float)(cc - 1) + p.cclm_mode_idx_offset, p.cclm_pow);
                else if (tree == 1)
                    cclm_bits = 0.0f;
                else
                    cclm_bits = p.non_cclm_offset;
                float mode_bits;
                if (cls == 0) {
                    mode_bits = p.planar_offset;
                } else {
                    float t;
                    if (cls <= 5)
                        t = std::pow((float)(cls - 1) + p.mpm_idx_offset, p.mpm_idx_pow);
                    else
                        t = p.mpm_remainder_mult * std::pow((float)(cls - 6) + p.mpm_remainder_offset, p.mpm_remainder_pow);
                    mode_bits = p.non_planar_offset + t;
                }
                mode_bits = mode_bits + cclm_bits;
                const float hb = tree == 0 ? p.header_bits + mode_bits : p.header_bits / 3.0f + mode_bits;
                cfg->header_bits_luma[tree][cc][cls] = (int64_t)(hb * 16384.0f);
            }
    for (int cc = 0; cc < 4; ++cc) {
        const float mode_bits =
            cc > 0 ? p.cclm_offset + std::pow((float)(cc - 1) + p.cclm_mode_idx_offset, p.cclm_pow) : p.non_cclm_offset;
        cfg->header_bits_chroma[cc] = (int64_t)((p.chroma_header_bits + mode_bits) * 16384.0f);
    }
}

int wrenc_gpu_default_config(wrenc_gpu_config* cfg, int width, int height, int qp, int max_split_depth) {
    if (!cfg) return WRENC_GPU_EINVAL;
    memset(cfg, 0, sizeof(*cfg));
    cfg->width = width;
    cfg->height = height;
    cfg->qp = qp;
    cfg->max_split_depth = max_split_depth;
    cfg->device = 0;
    cfg->n_slots = 1;
    resolve_config(cfg, RdParams());
    return WRENC_GPU_OK;
}

int wrenc_gpu_config_extra_params(wrenc_gpu_config* cfg, const char* extra_params) {
    if (!cfg) return WRENC_GPU_EINVAL;
    RdParams p;
    const struct { const char* key; double* f64; float* f32; long long* i64; } live[] = {
        {"lv_pow_dq_trellis", &p.lv_pow, nullptr, nullptr},
        {"lv_offset_dq_trellis", &p.lv_offset, nullptr, nullptr},
        {"quant_lv_pow", &p.quant_lv_pow, nullptr, nullptr},
        {"quant_qp_div_trellis", &p.quant_qp_div, nullptr, nullptr},
        {"quant_lambda_mul_trellis", &p.quant_lambda_mul, nullptr, nullptr},
        {"quant_lambda_offset_trellis", nullptr, nullptr, &p.quant_lambda_offset},
        {"qp_div_dq_trellis", nullptr, &p.qp_div, nullptr},
        {"lambda_mul_dq_trellis", nullptr, &p.lambda_mul, nullptr},
        {"non_planar_offset_dq_trellis", nullptr, &p.non_planar_offset, nullptr},
        {"mpm_idx_offset_dq_trellis", nullptr, &p.mpm_idx_offset, nullptr},
        {"mpm_remainder_mult_dq_trellis", nullptr, &p.mpm_remainder_mult, nullptr},
        {"mpm_remainder_offset_dq_trellis", nullptr, &p.mpm_remainder_offset, nullptr},
        {"planer_offset_dq_trellis", nullptr, &p.planar_offset, nullptr}, // sic
        {"header_bits_dq_trellis", nullptr, &p.header_bits, nullptr},
        {"chroma_header_bits_dq_trellis", nullptr, &p.chroma_header_bits, nullptr},
        {"cclm_pow", nullptr, &p.cclm_pow, nullptr},
        {"mpm_idx_pow", nullptr, &p.mpm_idx_pow, nullptr},
        {"mpm_remainder_pow", nullptr, &p.mpm_remainder_pow, nullptr},
        {"cclm_mode_idx_offset_dq_trellis", nullptr, &p.cclm_mode_idx_offset, nullptr},
        {"non_cclm_offset_dq_trellis", nullptr, &p.non_cclm_offset, nullptr},
        {"cclm_offset_dq_trellis", nullptr, &p.cclm_offset, nullptr},
        {"a", nullptr, &p.a, nullptr},
    };
    const std::string text = extra_params ? extra_params : "";
    size_t pos = 0;
    while (!text.empty() && pos <= text.size()) {
        size_t end = text.find(',', pos);
        if (end == std::string::npos) end = text.size();
        const std::string item = text.substr(pos, end - pos);
        const size_t eq = item.find('=');
        if (eq == std::string::npos || item.find('=', eq + 1) != std::string::npos)
            return fail(nullptr, WRENC_GPU_EINVAL, "Invalid extra-params: " + text); // main.rs:205-215
        const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
        for (const auto& l : live) {
            if (key != l.key) continue;
            char* rest = nullptr;
            if (l.f64) *l.f64 = strtod(val.c_str(), &rest);
            if (l.f32) *l.f32 = strtof(val.c_str(), &rest);
            if (l.i64) *l.i64 = strtoll(val.c_str(), &rest, 10);
            if (val.empty() || (rest && *rest)) // the reference's parse().unwrap() panics here
                return fail(nullptr, WRENC_GPU_EINVAL, "extra-params: " + key + " has no numeric value: " + val);
            if (key == "a") p.has_a = true;
        }
        // any other key is stored and never read by the live code path, as in the reference
        pos = end + 1;
    }
    resolve_config(cfg, p);
    return WRENC_GPU_OK;
}

const char* wrenc_gpu_last_error(const wrenc_gpu_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void wrenc_gpu_destroy(wrenc_gpu_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    // every stream that exists (a context whose creation failed half-way has only some)
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream.get());
    for (const HipStream& st : ctx->lanes)
        if (st) (void)hipStreamSynchronize(st.get());
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream.get());
    if (ctx->hash_stream) (void)hipStreamSynchronize(ctx->hash_stream.get());
    delete ctx; // (frees the device memory and destroys the streams and events: every stream has been synchronised above)
}

// The trellis keeps path costs in 32 bits (dev_quant.h, above kNoBranch): exact as long as one step costs less than 2^25,
// i.e. 128 * 65535 + lambda_q * dq_table[bits] < 2^25 for every table entry -- true for the reference's defaults at every
// QP (22.6 M at QP 63) and for rate models anywhere near them, not for e.g. quant_lv_pow = 2.5 or quant_qp_div_trellis =
// 1.5 (--extra-params), where the reference's own i64 products reach 10^11 .. 10^19.  Refused rather than searched
// with other results than the reference's.  (lambda_q grows with the QP: a model may fit at one QP and not at another.)
static bool rate_model_fits(const wrenc_gpu_config& cfg) {
    constexpr long long kStepRoom = (1LL << 25) - 128LL * 65535LL;
    bool fits = cfg.lambda_q >= 0 && cfg.lambda_q < kStepRoom;
    for (int i = 0; fits && i < 1024; ++i)
        fits = cfg.dq_table[i] >= 0 && cfg.dq_table[i] < kStepRoom && cfg.lambda_q * cfg.dq_table[i] < kStepRoom;
    return fits;
}
static const char* const kRateModelMsg =
    "the quantiser's rate model (lambda_q x dq_table) is outside the range the device's 32-bit trellis costs cover";

// The constant block of qc.qp into the context's table (wrenc_gpu_ctx::qconst), built from `qc`: the context's own config
// or one that differs from it in the QP and the lambdas only.  hipErrorOutOfMemory where the host has no memory either.
static hipError_t make_qp_const(wrenc_gpu_ctx* ctx, const wrenc_gpu_config& qc) {
    std::unique_ptr<DevConst> hk(new (std::nothrow) DevConst());
    if (!hk) return hipErrorOutOfMemory;
    fill_dev_const(qc, *hk);
    DevBuf<DevConst> d;
    if (hipError_t e = d.alloc(1)) return e;
    if (hipError_t e = hipMemcpy(d.get(), hk.get(), sizeof(DevConst), hipMemcpyHostToDevice)) return e;
    ctx->qconst[qc.qp] = wrenc_gpu_ctx::QpConst{std::move(d), qc.lambda_q, qc.lambda_rd, qc.lambda_rd_chroma};
    return hipSuccess;
}

int wrenc_gpu_create(const wrenc_gpu_config* cfg, wrenc_gpu_ctx** out) {
    if (!cfg || !out) return fail(nullptr, WRENC_GPU_EINVAL, "null argument");
    *out = nullptr;
    if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 31) || (cfg->height & 31))
        return fail(nullptr, WRENC_GPU_EINVAL, "width and height must be positive multiples of 32");
    if (cfg->qp < 0 || cfg->qp > 63) return fail(nullptr, WRENC_GPU_EINVAL, "qp out of range 0..63");
    if (cfg->max_split_depth < 0 || cfg->max_split_depth > 3)
        return fail(nullptr, WRENC_GPU_EINVAL, "max_split_depth out of range 0..3");
    if (cfg->n_slots < 1) return fail(nullptr, WRENC_GPU_EINVAL, "n_slots must be >= 1");
    if (!rate_model_fits(*cfg)) return fail(nullptr, WRENC_GPU_EINVAL, kRateModelMsg);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, WRENC_GPU_ENODEV, "no HIP device available");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, WRENC_GPU_ENODEV, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess)
        return fail(nullptr, WRENC_GPU_ENODEV, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, WRENC_GPU_ENODEV, std::string("built for gfx950, device is ") + prop.gcnArchName);
    wrenc_gpu_ctx* ctx = new (std::nothrow) wrenc_gpu_ctx();
    if (!ctx) return fail(nullptr, WRENC_GPU_ENOMEM, "out of host memory");
    ctx->cfg = *cfg;
    ctx->wave_slots = ctx->device_wave_slots = (long long)prop.multiProcessorCount * kWorkgroupsPerCU * WPB;
    ctx->ctu_cols = cfg->width / 32;
    ctx->ctu_rows = cfg->height / 32;
    ctx->vis_w = cfg->width;
    ctx->vis_h = cfg->height;
    auto bail = [&](int code, const std::string& msg) {
        g_create_error = msg;
        wrenc_gpu_destroy(ctx);
        return code;
    };
#define CREATE_TRY(expr)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return bail(e_ == hipErrorOutOfMemory ? WRENC_GPU_ENOMEM : WRENC_GPU_EHIP,              \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)
    CREATE_TRY(hipSetDevice(cfg->device));
    CREATE_TRY(ctx->stream.create(hipStreamNonBlocking));
    CREATE_TRY(ctx->ev_uploaded.create(hipEventDisableTiming));
    ctx->enc_events.resize(8);
    for (HipEvent& e : ctx->enc_events) CREATE_TRY(e.create(hipEventDisableTiming));
    ctx->slot_event.assign((size_t)cfg->n_slots, nullptr);
    CREATE_TRY(ctx->ev_fork.create());
    ctx->lanes.resize(kEncodeLanes - 1);
    ctx->lane_done.resize(kEncodeLanes - 1);
    for (int i = 0; i < kEncodeLanes - 1; ++i) {
        CREATE_TRY(ctx->lanes[(size_t)i].create(hipStreamNonBlocking));
        CREATE_TRY(ctx->lane_done[(size_t)i].create());
    }
    // Created after the encode lanes on purpose: the runtime deals streams onto its hardware queues in
    // creation order (4 per process unless GPU_MAX_HW_QUEUES says otherwise), and two lanes on one queue
    // would run one after the other.  With 4 queues the copy stream shares lane 0's.
    CREATE_TRY(ctx->copy_stream.create(hipStreamNonBlocking));
    CREATE_TRY(ctx->ev_begin.create());
    CREATE_TRY(ctx->ev_end.create());
    CREATE_TRY(make_qp_const(ctx, *cfg));
    CREATE_TRY(ctx->d_mismatch.alloc(1));
    CREATE_TRY(hipMemset(ctx->d_mismatch.get(), 0, sizeof(unsigned long long)));
    CREATE_TRY(ctx->d_overflow.alloc(2)); // [0]: encode calls (sticky), [1]: the building-block test entries
    CREATE_TRY(hipMemset(ctx->d_overflow.get(), 0, 2 * sizeof(int)));
    ctx->slots.assign(cfg->n_slots, PicBufs{});
    ctx->slot_mem.resize((size_t)cfg->n_slots);
    ctx->state.assign(cfg->n_slots, 0);
    ctx->slot_qp.assign(cfg->n_slots, cfg->qp);
    ctx->call_lists.resize(ctx->enc_events.size());
    for (int s = 0; s < cfg->n_slots; ++s) {
        PicBufs& b = ctx->slots[s];
        wrenc_gpu_ctx::SlotMem& m = ctx->slot_mem[(size_t)s];
        // Y | Cb | Cr of a picture are one slab each for originals, reconstruction and levels: the
        // kernel addresses a plane by an element offset, never by selecting a pointer per lane
        const size_t wh = (size_t)cfg->width * cfg->height;
        const size_t n_ctus = (size_t)ctx->ctu_cols * ctx->ctu_rows;
        const size_t n4 = (size_t)(cfg->width / 4) * (cfg->height / 4), n8 = (size_t)(cfg->width / 8) * (cfg->height / 8);
        CREATE_TRY(m.org.alloc(wh + wh / 2));
        CREATE_TRY(m.org_t.alloc(n_ctus * kOrgTile));
        CREATE_TRY(m.border.alloc(n_ctus * kBorderBytes));
        CREATE_TRY(m.rec.alloc(wh + wh / 2));
        CREATE_TRY(m.lev.alloc(wh + wh / 2));
        CREATE_TRY(m.lev_dirty.alloc(n_ctus * 4));
        CREATE_TRY(m.cu_log2.alloc(n4));
        CREATE_TRY(m.luma_mode.alloc(n4));
        CREATE_TRY(m.chroma_mode.alloc(n8));
        CREATE_TRY(m.ctu_cost.alloc(n_ctus));
        const size_t plane_at[3] = {0, wh, wh + wh / 4};
        for (int p = 0; p < 3; ++p) {
            b.org[p] = m.org.get() + plane_at[p];
            b.rec[p] = m.rec.get() + plane_at[p];
            b.lev[p] = m.lev.get() + plane_at[p];
        }
        b.org_t = m.org_t.get();
        b.border = m.border.get();
        b.lev_dirty = m.lev_dirty.get();
        b.cu_log2 = m.cu_log2.get();
        b.luma_mode = m.luma_mode.get();
        b.chroma_mode = m.chroma_mode.get();
        b.ctu_cost = m.ctu_cost.get();
        // the planes start zeroed, with no block marked as holding levels (PicBufs::lev_dirty)
        CREATE_TRY(hipMemsetAsync(b.lev[0], 0, (wh + wh / 2) * sizeof(int16_t), ctx->stream.get()));
        CREATE_TRY(hipMemsetAsync(b.lev_dirty, 0, n_ctus * 4 * sizeof(uint32_t), ctx->stream.get()));
    }
    CREATE_TRY(ctx->d_slots.alloc((size_t)cfg->n_slots));
    CREATE_TRY(hipMemcpy(ctx->d_slots.get(), ctx->slots.data(), sizeof(PicBufs) * cfg->n_slots, hipMemcpyHostToDevice));
    CREATE_TRY(hipStreamSynchronize(ctx->stream.get())); // the level planes are zero before anything can reach them
#undef CREATE_TRY
    *out = ctx;
    return WRENC_GPU_OK;
}

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

int wrenc_gpu_upload(wrenc_gpu_ctx* ctx, int slot, const uint8_t* y, const uint8_t* cb, const uint8_t* cr,
                     size_t stride_y, size_t stride_c) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (slot < 0 || slot >= ctx->cfg.n_slots || !y || !cb || !cr) return fail(ctx, WRENC_GPU_EINVAL, "bad slot or null plane");
    if (ctx->src_format) return fail(ctx, WRENC_GPU_ESTATE, "a source format is set: the planes go through wrenc_gpu_upload_planes");
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
    if (scaling) {
        // Source-size planes into the context's staging planes, then the scaler (dev_scale.h) writes the visible
        // rectangle of the slot's planes.  Copies, scaler, pad and retile all run on copy_stream, in order: the one set of
        // staging planes is read out before the next upload's copies reach it, whichever slot that one is for.  The
        // same holds one step earlier on a context with a source format (wrenc_gpu_upload_planes below): raw copies,
        // converter, scaler, pad and retile are one chain on this stream, so the one set of raw staging planes has been
        // converted out of, and the scaler's planes -- which the converter then writes in place of the copies -- scaled
        // out of, before the next upload's first copy starts.
        ScaleArgs a = ctx->scale_args;
        const uint8_t* const from[3] = {y, cb, cr};
        for (int p = 0; p < 3; ++p)
            HIP_TRY(ctx, hipMemcpy2DAsync((void*)a.src[p], (size_t)a.src_pitch[p ? 1 : 0], from[p], p ? stride_c : stride_y,
                                          p ? sw / 2 : sw, p ? sh / 2 : sh, hipMemcpyHostToDevice, cs));
        a.dst = (uint8_t*)b.org[0];
        hipLaunchKernelGGL(scale_kernel, dim3((unsigned)(a.tiles[0] + 2 * a.tiles[1])), dim3(256), 0, cs, a);
    } else {
        HIP_TRY(ctx, hipMemcpy2DAsync((void*)b.org[0], w, y, stride_y, vw, vh, hipMemcpyHostToDevice, cs));
        HIP_TRY(ctx, hipMemcpy2DAsync((void*)b.org[1], w / 2, cb, stride_c, vw / 2, vh / 2, hipMemcpyHostToDevice, cs));
        HIP_TRY(ctx, hipMemcpy2DAsync((void*)b.org[2], w / 2, cr, stride_c, vw / 2, vh / 2, hipMemcpyHostToDevice, cs));
    }
    return finish_upload(ctx, slot);
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

namespace {

// the raw staging planes of the context's format at its source size: pitches, offsets and the bytes of the allocation
struct RawStage {
    struct wrenc_gpu_format_layout lay;
    size_t pitch[3], off[3], bytes;
};

bool raw_stage(const wrenc_gpu_ctx* ctx, int format, RawStage& r) {
    const int sw = ctx->src_w ? ctx->src_w : ctx->vis_w, sh = ctx->src_w ? ctx->src_h : ctx->vis_h;
    if (wrenc_format_layout(format, sw, sh, &r.lay)) return false;
    r.bytes = 0;
    for (int p = 0; p < 3; ++p) {
        r.pitch[p] = format_raw_pitch(r.lay.row_bytes[p]);
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

} // namespace

int wrenc_gpu_set_source_format(wrenc_gpu_ctx* ctx, int format) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (!wrenc_format_valid(format)) return fail(ctx, WRENC_GPU_EINVAL, "unknown source format");
    if (ctx->any_upload) return fail(ctx, WRENC_GPU_ESTATE, "the source format must be set before the first upload");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    if (format == WRENC_FORMAT_YUV420P) {
        ctx->d_raw.reset();
        ctx->src_format = 0;
        return WRENC_GPU_OK;
    }
    RawStage r;
    if (!raw_stage(ctx, format, r)) return fail(ctx, WRENC_GPU_EINVAL, "the source format needs pictures of an even size, at least 16x16");
    const int rc = ensure_raw_stage(ctx, r);
    if (rc) return rc;
    ctx->src_format = format;
    return WRENC_GPU_OK;
}

int wrenc_gpu_source_format(const wrenc_gpu_ctx* ctx) { return ctx ? ctx->src_format : WRENC_GPU_EINVAL; }

int wrenc_gpu_upload_planes(wrenc_gpu_ctx* ctx, int slot, const void* const plane[3], const size_t stride_bytes[3]) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (!plane || !stride_bytes) return fail(ctx, WRENC_GPU_EINVAL, "null plane or stride list");
    const int format = ctx->src_format;
    if (format == WRENC_FORMAT_YUV420P) {
        if (stride_bytes[1] != stride_bytes[2]) return fail(ctx, WRENC_GPU_EINVAL, "yuv420p: the two chroma planes share one stride");
        return wrenc_gpu_upload(ctx, slot, (const uint8_t*)plane[0], (const uint8_t*)plane[1], (const uint8_t*)plane[2], stride_bytes[0],
                                stride_bytes[1]);
    }
    if (slot < 0 || slot >= ctx->cfg.n_slots) return fail(ctx, WRENC_GPU_EINVAL, "bad slot or null plane");
    RawStage r;
    if (!raw_stage(ctx, format, r)) return fail(ctx, WRENC_GPU_EINVAL, "the source format needs pictures of an even size, at least 16x16");
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
    // the caller's bytes as they are -- a 10-bit picture crosses the bus once -- and behind them the converter (dev_format.h)
    FormatArgs a = {};
    a.raw = ctx->d_raw.get();
    for (int p = 0; p < r.lay.n_planes; ++p) {
        HIP_TRY(ctx, hipMemcpy2DAsync((void*)(ctx->d_raw.get() + r.off[p]), r.pitch[p], plane[p], stride_bytes[p], r.lay.row_bytes[p], r.lay.rows[p],
                                      hipMemcpyHostToDevice, cs));
        a.raw_off[p] = r.off[p];
        a.raw_pitch[p] = (int)r.pitch[p];
    }
    if (scaling) { // into the scaler's staging planes, in the place of wrenc_gpu_upload's copies
        const ScaleArgs& s = ctx->scale_args;
        a.dst = ctx->d_stage.get();
        for (int p = 0; p < 3; ++p) a.dst_off[p] = (size_t)(s.src[p] - s.src[0]);
        a.dst_pitch[0] = s.src_pitch[0];
        a.dst_pitch[1] = s.src_pitch[1];
        a.w = ctx->src_w;
        a.h = ctx->src_h;
    } else { // into the visible rectangle of the slot's planes
        a.dst = (uint8_t*)b.org[0];
        a.dst_off[1] = w * h;
        a.dst_off[2] = w * h + w * h / 4;
        a.dst_pitch[0] = (int)w;
        a.dst_pitch[1] = (int)(w / 2);
        a.w = ctx->vis_w;
        a.h = ctx->vis_h;
    }
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
    if (scaling) {
        ScaleArgs s = ctx->scale_args;
        s.dst = (uint8_t*)b.org[0];
        hipLaunchKernelGGL(scale_kernel, dim3((unsigned)(s.tiles[0] + 2 * s.tiles[1])), dim3(256), 0, cs, s);
    }
    return finish_upload(ctx, slot);
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

int wrenc_gpu_set_slot_qp(wrenc_gpu_ctx* ctx, int slot, const wrenc_gpu_config* qcfg) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (slot < 0 || slot >= ctx->cfg.n_slots) return fail(ctx, WRENC_GPU_EINVAL, "bad slot");
    const wrenc_gpu_config& c = ctx->cfg;
    if (!qcfg) {
        ctx->slot_qp[slot] = c.qp;
        return WRENC_GPU_OK;
    }
    if (qcfg->qp < 0 || qcfg->qp > 63) return fail(ctx, WRENC_GPU_EINVAL, "qp out of range 0..63");
    if (qcfg->width != c.width || qcfg->height != c.height || qcfg->max_split_depth != c.max_split_depth ||
        memcmp(qcfg->lv_table, c.lv_table, sizeof(c.lv_table)) || memcmp(qcfg->dq_table, c.dq_table, sizeof(c.dq_table)) ||
        memcmp(qcfg->header_bits_luma, c.header_bits_luma, sizeof(c.header_bits_luma)) ||
        memcmp(qcfg->header_bits_chroma, c.header_bits_chroma, sizeof(c.header_bits_chroma)))
        return fail(ctx, WRENC_GPU_EINVAL,
                    "a slot's config may differ from the context's in qp, lambda_q, lambda_rd and lambda_rd_chroma only");
    const int q = qcfg->qp;
    const wrenc_gpu_ctx::QpConst& known = ctx->qconst[q];
    if (known.d) {
        if (qcfg->lambda_q != known.lambda_q || memcmp(&qcfg->lambda_rd, &known.lambda_rd, sizeof(float)) ||
            memcmp(&qcfg->lambda_rd_chroma, &known.lambda_rd_chroma, sizeof(float)))
            return fail(ctx, WRENC_GPU_EINVAL, "the context has another lambda set for this QP");
        ctx->slot_qp[slot] = q;
        return WRENC_GPU_OK;
    }
    if (!rate_model_fits(*qcfg)) return fail(ctx, WRENC_GPU_EINVAL, kRateModelMsg);
    // the QP's constant block, built once: it is never changed or freed while the context lives, so a call in flight
    // that reads it is not disturbed
    HIP_TRY(ctx, hipSetDevice(c.device));
    if (const hipError_t e = make_qp_const(ctx, *qcfg)) {
        (void)hipGetLastError();
        return fail(ctx, e == hipErrorOutOfMemory ? WRENC_GPU_ENOMEM : WRENC_GPU_EHIP,
                    std::string("constant block of a QP: ") + hipGetErrorString(e));
    }
    ctx->slot_qp[slot] = q;
    return WRENC_GPU_OK;
}

int wrenc_gpu_encode(wrenc_gpu_ctx* ctx, int first_slot, int n_pictures) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (const int rc = check_slots(ctx, first_slot, n_pictures, 1, "slot range out of bounds")) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const bool timed = ctx->stats_enabled;
    // the timing events are re-recorded by every call: the previous call's must have been reached first
    if (timed && ctx->stats_valid) HIP_TRY(ctx, hipEventSynchronize(ctx->ev_end.get()));
    ctx->stats_valid = false; // until this call has recorded the events that go with its plan
    // The whole schedule is decided before anything is queued (encode_plan.h), and kept: the statistics entry points read it.
    // The pictures' QPs are read now: a later wrenc_gpu_set_slot_qp does not change this call.  A call at one QP runs its
    // slots in place with that QP's constant block; a mixed one from a list of its own (CallGroup, above the kernels).
    const bool d3 = ctx->cfg.max_split_depth == 3; // the kernels built with / without the 4x4 leaves of split 8x8 CUs
    Plan& plan = ctx->plan;
    ctx->call_qp.assign(ctx->slot_qp.begin() + first_slot, ctx->slot_qp.begin() + first_slot + n_pictures);
    plan_encode(plan, ctx->ctu_cols, ctx->ctu_rows, ctx->call_qp.data(), n_pictures, ctx->schedule, ctx->wave_slots, d3, kPlanBuild);
    const PicBufs* d_pics = ctx->d_slots.get();
    const CallGroup* d_groups = nullptr;
    int list_first = first_slot;
    if (plan.mixed()) {
        // this call's list: the ring entry of the completion event it will record, last used by the call that recorded
        // that event before -- which must be done before the list is rewritten
        const size_t ring = ctx->enc_event_next % ctx->enc_events.size();
        HIP_TRY(ctx, hipEventSynchronize(ctx->enc_events[ring].get()));
        wrenc_gpu_ctx::CallList& cl = ctx->call_lists[ring];
        cl.pics.clear();
        cl.groups.clear();
        for (const int i : plan.entries) cl.pics.push_back(ctx->slots[(size_t)(first_slot + i)]);
        for (const PlanGroup& g : plan.groups) cl.groups.push_back(CallGroup{ctx->qconst[g.qp].d.get(), g.n_real});
        if (cl.d_pics.grow(cl.pics.size()) != hipSuccess || cl.d_groups.grow(cl.groups.size()) != hipSuccess)
            return fail(ctx, WRENC_GPU_ENOMEM, "no device memory for the picture list of a mixed-QP call");
        HIP_TRY(ctx, hipMemcpyAsync(cl.d_pics.get(), cl.pics.data(), sizeof(PicBufs) * cl.pics.size(), hipMemcpyHostToDevice, ctx->stream.get()));
        HIP_TRY(ctx, hipMemcpyAsync(cl.d_groups.get(), cl.groups.data(), sizeof(CallGroup) * cl.groups.size(), hipMemcpyHostToDevice,
                                    ctx->stream.get()));
        d_pics = cl.d_pics.get();
        d_groups = cl.d_groups.get();
        list_first = 0;
    }
    const int n_lanes = plan.n_lanes;
    if (!ctx->d_pred_scratch) { // into locals first: a call that fails here leaves the context with neither
        DevBuf<uint8_t> scratch;
        DevBuf<unsigned long long> map;
        HIP_TRY(ctx, scratch.alloc((size_t)kScratchSlots * WPB * kWaveScratch));
        HIP_TRY(ctx, map.alloc(kSlotMapWords));
        HIP_TRY(ctx, hipMemset(map.get(), 0, kSlotMapWords * 8));
        ctx->d_pred_scratch = std::move(scratch);
        ctx->d_slot_map = std::move(map);
    }
    while (timed && ctx->ev_pool.size() < 2 * (size_t)plan.n_spans) {
        HipEvent e;
        HIP_TRY(ctx, e.create());
        ctx->ev_pool.push_back(std::move(e));
    }
    // The scratch-region bitmap is only ever changed by running workgroups (acquire at start, release at
    // end).  A kernel that was aborted would leave its bits set for good, so the map is cleared whenever no
    // encode call is in flight (the last call's completion event has been reached).
    if (ctx->last_done == nullptr || hipEventQuery(ctx->last_done) == hipSuccess)
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_slot_map.get(), 0, kScratchSlots / 8, ctx->stream.get())); // (not the overflow counter)
    if (ctx->uploads_pending) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev_uploaded.get(), ctx->copy_stream.get()));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream.get(), ctx->ev_uploaded.get(), 0));
        ctx->uploads_pending = false;
    }
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_begin.get(), ctx->stream.get()));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork.get(), ctx->stream.get()));
    for (int l = 1; l < n_lanes; ++l) HIP_TRY(ctx, hipStreamWaitEvent(ctx->lanes[l - 1].get(), ctx->ev_fork.get(), 0));
    for (size_t i = 0; i < plan.launches.size(); ++i) {
        const PlanLaunch& L = plan.launches[i];
        hipStream_t st = L.lane == 0 ? ctx->stream.get() : ctx->lanes[L.lane - 1].get();
        // a span's launches (one, or one per QP class for the teams of a mixed call) follow each other: one pair of events
        const bool opens = i == 0 || plan.launches[i - 1].span != L.span;
        const bool closes = i + 1 == plan.launches.size() || plan.launches[i + 1].span != L.span;
        if (timed && opens) HIP_TRY(ctx, hipEventRecord(ctx->ev_pool[2 * (size_t)L.span].get(), st));
        // (the wave kernel of a mixed call takes each group's block from `groups` and ignores the one it is given)
        const DevConst* k = ctx->qconst[L.qp < 0 ? ctx->cfg.qp : L.qp].d.get();
        const auto launch = [&](auto kernel, auto... groups) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)L.grid), dim3(64 * WPB), 0, st, k, d_pics, list_first + L.first, L.n, L.diag, L.r_min,
                               L.count, ctx->d_pred_scratch.get(), ctx->d_slot_map.get(), ctx->d_mismatch.get(), ctx->d_overflow.get(),
                               groups...);
        };
        const CallGroup* groups = L.group < 0 ? nullptr : d_groups + L.group;
        if (L.team)
            d3 ? launch(ctu_search_team_kernel<true>) : launch(ctu_search_team_kernel<false>);
        else
            d3 ? launch(ctu_search_kernel<true>, groups) : launch(ctu_search_kernel<false>, groups);
        HIP_TRY(ctx, hipGetLastError());
        if (timed && closes) HIP_TRY(ctx, hipEventRecord(ctx->ev_pool[2 * (size_t)L.span + 1].get(), st));
    }
    for (int l = 1; l < n_lanes; ++l) {
        HIP_TRY(ctx, hipEventRecord(ctx->lane_done[l - 1].get(), ctx->lanes[l - 1].get()));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream.get(), ctx->lane_done[l - 1].get(), 0));
    }
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_end.get(), ctx->stream.get()));
    // downloads of these slots wait for this call only, not for searches queued after it
    hipEvent_t done = ctx->enc_events[ctx->enc_event_next++ % ctx->enc_events.size()].get();
    HIP_TRY(ctx, hipEventRecord(done, ctx->stream.get()));
    ctx->last_done = done;
    ctx->stats_valid = timed;
    for (int s = first_slot; s < first_slot + n_pictures; ++s) {
        ctx->state[s] = 2;
        ctx->slot_event[s] = done;
    }
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

int wrenc_gpu_encode_picture(wrenc_gpu_ctx* ctx, const uint8_t* y, const uint8_t* cb, const uint8_t* cr,
                             wrenc_gpu_picture* out) {
    if (!ctx) return WRENC_GPU_EINVAL;
    const int row = ctx->src_w ? ctx->src_w : ctx->vis_w;
    int rc = wrenc_gpu_upload(ctx, 0, y, cb, cr, (size_t)row, (size_t)row / 2);
    if (rc) return rc;
    rc = wrenc_gpu_encode(ctx, 0, 1);
    if (rc) return rc;
    return wrenc_gpu_download(ctx, 0, out);
}

int wrenc_gpu_last_encode_stats(wrenc_gpu_ctx* ctx, float* total_ms, float* kernel_ms_sum, int* n_launches) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (!ctx->stats_enabled) return fail(ctx, WRENC_GPU_ESTATE, "per-launch timing is off (wrenc_gpu_stats_enable)");
    if (!ctx->stats_valid) return fail(ctx, WRENC_GPU_ESTATE, "no encode has been queued since timing was switched on");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_end.get()));
    float t = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->ev_begin.get(), ctx->ev_end.get()));
    float sum = 0.f;
    for (size_t i = 0; i < (size_t)ctx->plan.n_spans; ++i) {
        float k = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&k, ctx->ev_pool[2 * i].get(), ctx->ev_pool[2 * i + 1].get()));
        sum += k;
    }
    if (total_ms) *total_ms = t;
    if (kernel_ms_sum) *kernel_ms_sum = sum;
    if (n_launches) *n_launches = ctx->plan.n_spans;
    return WRENC_GPU_OK;
}

int wrenc_gpu_last_encode_kernel_stats(wrenc_gpu_ctx* ctx, wrenc_gpu_kernel_stats out[2]) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    if (!ctx->stats_enabled) return fail(ctx, WRENC_GPU_ESTATE, "per-launch timing is off (wrenc_gpu_stats_enable)");
    if (!ctx->stats_valid) return fail(ctx, WRENC_GPU_ESTATE, "no encode has been queued since timing was switched on");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_end.get()));
    for (int k = 0; k < 2; ++k) out[k] = wrenc_gpu_kernel_stats{0.f, 0, 0};
    // per span (a lane's launches of one diagonal, all of one kernel): its pair of events once, the CTU-pictures of each launch
    int span = -1;
    for (const PlanLaunch& L : ctx->plan.launches) {
        wrenc_gpu_kernel_stats& o = out[L.team];
        o.ctu_pictures += L.ctus;
        if (L.span == span) continue;
        span = L.span;
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_pool[2 * (size_t)span].get(), ctx->ev_pool[2 * (size_t)span + 1].get()));
        o.ms_sum += ms;
        o.launches += 1;
    }
    return WRENC_GPU_OK;
}

int wrenc_gpu_set_schedule(wrenc_gpu_ctx* ctx, int schedule) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (schedule != WRENC_GPU_SCHEDULE_AUTO && schedule != WRENC_GPU_SCHEDULE_WAVE && schedule != WRENC_GPU_SCHEDULE_TEAM)
        return fail(ctx, WRENC_GPU_EINVAL, "schedule must be WRENC_GPU_SCHEDULE_AUTO, _WAVE or _TEAM");
    ctx->schedule = schedule;
    return WRENC_GPU_OK;
}

int wrenc_gpu_last_schedule(const wrenc_gpu_ctx* ctx) { return ctx ? ctx->plan.schedule : WRENC_GPU_EINVAL; }

int wrenc_gpu_test_plan(int ctu_cols, int ctu_rows, const int* qps, int n_pictures, int schedule, long long wave_slots, int depth3,
                        wrenc_gpu_plan_info* info, wrenc_gpu_plan_launch* launches, int launches_cap, int* entries, int entries_cap,
                        int* groups, int groups_cap) {
    if (!qps || !info || ctu_cols < 1 || ctu_rows < 1 || n_pictures < 1 || wave_slots < 1) return WRENC_GPU_EINVAL;
    if (schedule != WRENC_GPU_SCHEDULE_AUTO && schedule != WRENC_GPU_SCHEDULE_WAVE && schedule != WRENC_GPU_SCHEDULE_TEAM)
        return WRENC_GPU_EINVAL;
    for (int i = 0; i < n_pictures; ++i)
        if (qps[i] < 0 || qps[i] > 63) return WRENC_GPU_EINVAL;
    Plan p;
    plan_encode(p, ctu_cols, ctu_rows, qps, n_pictures, schedule, wave_slots, depth3 != 0, kPlanBuild);
    *info = wrenc_gpu_plan_info{(int32_t)p.launches.size(), (int32_t)p.entries.size(), (int32_t)p.groups.size(), p.n_lanes, p.n_spans,
                                p.schedule, kPlanBuild.wpb, kPlanBuild.team, kPlanBuild.lanes, kPlanBuild.team_below_pct,
                                kPlanBuild.team_below_pct_d3};
    if ((!launches && launches_cap) || (!entries && entries_cap) || (!groups && groups_cap)) return WRENC_GPU_EINVAL;
    if (launches_cap < info->n_launches || entries_cap < info->n_entries || groups_cap < info->n_groups) return WRENC_GPU_EINVAL;
    for (size_t i = 0; i < p.launches.size(); ++i) {
        const PlanLaunch& L = p.launches[i];
        launches[i] = wrenc_gpu_plan_launch{L.lane, L.team, L.diag, L.r_min, L.count, L.first, L.n, L.grid, L.group, L.qp, L.span, L.ctus};
    }
    for (size_t i = 0; i < p.entries.size(); ++i) entries[i] = p.entries[i];
    for (size_t i = 0; i < p.groups.size(); ++i) groups[2 * i] = p.groups[i].qp, groups[2 * i + 1] = p.groups[i].n_real;
    return WRENC_GPU_OK;
}

int wrenc_gpu_device_info(const wrenc_gpu_ctx* ctx, long long* wave_slots, int* encode_lanes) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (wave_slots) *wave_slots = ctx->device_wave_slots;
    if (encode_lanes) *encode_lanes = kEncodeLanes;
    return WRENC_GPU_OK;
}

int wrenc_gpu_test_set_wave_slots(wrenc_gpu_ctx* ctx, long long slots) {
    if (!ctx) return WRENC_GPU_EINVAL;
    ctx->wave_slots = slots > 0 ? slots : ctx->device_wave_slots;
    return WRENC_GPU_OK;
}

int wrenc_gpu_test_scratch_overflows(wrenc_gpu_ctx* ctx, long long* count) {
    if (!ctx || !count) return WRENC_GPU_EINVAL;
    *count = 0;
    if (!ctx->d_slot_map) return WRENC_GPU_OK; // no encode call yet
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    unsigned long long v = 0;
    HIP_TRY(ctx, hipMemcpy(&v, ctx->d_slot_map.get() + kScratchSlots / 64, sizeof(v), hipMemcpyDeviceToHost));
    *count = (long long)v;
    return WRENC_GPU_OK;
}

int wrenc_gpu_stats_enable(wrenc_gpu_ctx* ctx, int on) {
    if (!ctx) return WRENC_GPU_EINVAL;
    ctx->stats_enabled = on != 0;
    ctx->stats_valid = false;
    return WRENC_GPU_OK;
}

int wrenc_gpu_final_pass_mismatches(wrenc_gpu_ctx* ctx, long long* count) {
    if (!ctx || !count) return WRENC_GPU_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
    unsigned long long v = 0;
    HIP_TRY(ctx, hipMemcpy(&v, ctx->d_mismatch.get(), sizeof(v), hipMemcpyDeviceToHost));
    *count = (long long)v;
    return WRENC_GPU_OK;
}

#ifdef WRENC_TRACE
// diagnostic build only: copies up to max_records records (8 ints each) of the last encode call's trace,
// returns the number of records made; resets the trace
extern "C" long wrenc_gpu_trace_read(wrenc_gpu_ctx* ctx, int* out, long max_records) {
    if (!ctx) return -1;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_trace_n), sizeof(n)) != hipSuccess) return -1;
    long take = n < kTraceMax ? (long)n : (long)kTraceMax;
    if (take > max_records) take = max_records;
    if (take > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trace), (size_t)take * 8 * sizeof(int)) != hipSuccess) return -1;
    const unsigned int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_trace_n), &zero, sizeof(zero)) != hipSuccess) return -1;
    return (long)n;
}
#endif

#ifdef WRENC_PROFILE
// diagnostic build only: read and clear the per-phase cycle counters
int wrenc_gpu_prof_read(wrenc_gpu_ctx* ctx, unsigned long long* out, int n) {
    if (!ctx || !out) return WRENC_GPU_EINVAL;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
    unsigned long long host[PH_COUNT];
    HIP_TRY(ctx, hipMemcpyFromSymbol(host, HIP_SYMBOL(g_prof), sizeof(host)));
    for (int i = 0; i < n && i < PH_COUNT; ++i) out[i] = host[i];
    memset(host, 0, sizeof(host));
    HIP_TRY(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_prof), host, sizeof(host)));
    return WRENC_GPU_OK;
}
#endif

} // extern "C"
