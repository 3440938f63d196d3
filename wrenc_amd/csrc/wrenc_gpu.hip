// wrenc_gpu.hip -- kernels + C ABI (include/wrenc_gpu.h) of the MI355X all-intra
// RD-search path.  Built for gfx950 only:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -o libwrenc_gpu.so wrenc_gpu.hip
//
// Scheduling: a picture's CTUs depend on their left, above-left, above and
// above-right neighbours (encoder_context.rs:934-948), so CTU (r, c) can run once
// every CTU on anti-diagonal c + 2r - 1 is done.  One launch processes one
// anti-diagonal of every picture of the batch (one wave per CTU); stream order
// between launches is the only synchronisation between CTUs.  (The one in-kernel
// wait is a workgroup's acquire of a scratch region from a bitmap that always has
// more regions than workgroups can be resident, see ctu_search_kernel.)
#include "../../include/wrenc_gpu.h"
#include "../../include/wrenc_scale.h"
#include "../../include/wrenc_format.h"
#include "../../include/wrenc_ratecurve.h"
#include "wrenc_dev.h"

#include <hip/hip_runtime.h>

#include "encode_plan.h"
#include "host_mem.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

using namespace wrenc;

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

// A mixed-QP encode call (wrenc_gpu_set_slot_qp) runs its pictures from a per-call list, ordered by QP and padded so that
// every group of WPB consecutive entries holds ONE QP: load_tables fills the workgroup's LDS tables (lambda_q x dq_table)
// with each thread reading its own wave's constant block, so a workgroup must never mix blocks.  Per group: the QP's
// constant block and how many of its WPB entries are pictures (the rest are padding: same work, no stores).
struct CallGroup {
    const DevConst* k;
    int n_real;
};

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

// building-block kernels: one wave per group of nb blocks of side 1 << lg, laid out [blk][y][x]; the transforms and the
// dequantiser work on r1[o1 ..], where the search puts a pack's chroma behind its luma (the host entries check that the
// group fits r1 and r2)
__global__ __launch_bounds__(64) void test_fwd_dct_kernel(const DevConst* __restrict__ k,
                                                          const int16_t* in, int lg, int nb, int o1, int16_t* out,
                                                          int arm, int reps) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    const int total = nb << (2 * lg);
    // arm: DCT_SEARCH, or the version of the 8x8 / 16x16 transforms the host names (dev_transform.h); reps repeats the
    // transform of the same group for the micro-benchmark
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = threadIdx.x; i < total; i += 64) SH.r1[o1 + i] = in[(size_t)blockIdx.x * total + i];
        WSYNC();
        if (arm == DCT_VDOT2)
            fwd_dct_lg<DCT_VDOT2>(c, lg, nb, o1);
        else if (arm == DCT_MFMA)
            fwd_dct_lg<DCT_MFMA>(c, lg, nb, o1);
        else
            fwd_dct_lg(c, lg, nb, o1);
    }
    for (int i = threadIdx.x; i < total; i += 64) out[(size_t)blockIdx.x * total + i] = SH.r1[o1 + i];
}

// MFMA experiment: the 32x32 forward transform as i8 MFMAs (dev_transform.h); `reps` repeats the transform
// of the same block in place for the micro-benchmark (the result of the last repetition is stored)
__shared__ int32_t s_h32[33 * 32]; // the v_dot2 arm's i32 intermediate (the search kernel has no such room)
__global__ __launch_bounds__(64) void test_fwd_dct32_kernel(const DevConst* __restrict__ k, const int16_t* in, int16_t* out,
                                                           int mfma, int reps) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = threadIdx.x; i < 1024; i += 64) SH.r1[i] = in[(size_t)blockIdx.x * 1024 + i];
        WSYNC();
        if (mfma)
            fwd_dct32_mfma(c, 0);
        else
            fwd_dct<5, (int)sizeof(s_h32)>(c, 1, 0, (LDS_AS int32_t*)s_h32);
    }
    for (int i = threadIdx.x; i < 1024; i += 64) out[(size_t)blockIdx.x * 1024 + i] = SH.r1[i];
}

// the same for the inverse 32x32 transform: dequantised blocks in (row-major), residuals out
__global__ __launch_bounds__(64) void test_inv_dct32_kernel(const DevConst* __restrict__ k, const int16_t* in, int16_t* out,
                                                           int mfma, int reps) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = threadIdx.x; i < 1024; i += 64) // transposed load: dT[x][i] = d[i][x]
            ((int16_t*)SH.r2)[(i & 31) * 32 + (i >> 5)] = in[(size_t)blockIdx.x * 1024 + i];
        WSYNC();
        if (mfma)
            inv_dct32_mfma(c, 0);
        else
            inv_dct<5>(c, 1, 0);
    }
    for (int i = threadIdx.x; i < 1024; i += 64) out[(size_t)blockIdx.x * 1024 + i] = SH.r1[i];
}

__global__ __launch_bounds__(64) void test_inv_dct_kernel(const DevConst* __restrict__ k,
                                                          const int16_t* in, int lg, int nb, int o1, int16_t* out,
                                                          int arm, int reps) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    const int n = 1 << lg, nn = n * n, total = nb * nn;
    for (int rep = 0; rep < reps; ++rep) {
        for (int i = threadIdx.x; i < total; i += 64) { // transposed load, block by block: dT[blk][x][i] = d[blk][i][x]
            const int ii = i & (nn - 1);
            ((int16_t*)SH.r2)[(i - ii) + (ii & (n - 1)) * n + (ii >> lg)] = in[(size_t)blockIdx.x * total + i];
        }
        WSYNC();
        if (arm == DCT_VDOT2)
            inv_dct_lg<DCT_VDOT2>(c, lg, nb, o1);
        else if (arm == DCT_MFMA)
            inv_dct_lg<DCT_MFMA>(c, lg, nb, o1);
        else
            inv_dct_lg(c, lg, nb, o1);
    }
    for (int i = threadIdx.x; i < total; i += 64) out[(size_t)blockIdx.x * total + i] = SH.r1[o1 + i];
}

// quantize_solo: nb = 1 (a luma block) or 2 (the Cb + Cr pair) blocks at r1[0 ..]; per group the summed level cost and the
// *any_level the function reported
__global__ __launch_bounds__(64) void test_quantize_kernel(const DevConst* __restrict__ k,
                                                           const int16_t* in, int lg, int nb, int16_t* out,
                                                           long long* cost, int* any_level, int* overflow) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    load_tables(c);
    const int total = nb << (2 * lg);
    for (int i = threadIdx.x; i < total; i += 64) SH.r1[i] = in[(size_t)blockIdx.x * total + i];
    WSYNC();
    int ovf = 0;
    bool any = false;
    const long long lc = quantize_solo(c, lg, nb, &ovf, &any);
    for (int i = threadIdx.x; i < total; i += 64) out[(size_t)blockIdx.x * total + i] = SH.r1[i];
    if (threadIdx.x == 0) {
        cost[blockIdx.x] = lc;
        any_level[blockIdx.x] = any ? 1 : 0;
        if (ovf) atomicOr(overflow, 1);
    }
}

// DevConst::head_rng against the functions it stands for, over every 16-bit coefficient (grid: 1024 blocks of 64 lanes;
// block size and DC flag in blockIdx.y): out[0] += coefficients the range lets into the region that head_alpha ends it
// at (never allowed), out[1] += coefficients the range ends the region at that head_alpha would let in (allowed, not
// expected), out[2] += coefficients whose "quotient >= 2" differs from the range's, out[3] += alpha differences
__global__ __launch_bounds__(64) void test_head_ranges_kernel(const DevConst* __restrict__ kk, int* out) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)kk;
    load_tables(c);
    const CONST_AS DevConst* k = c.k;
    const int lg = 2 + (int)(blockIdx.y >> 1);
    const bool dcn = blockIdx.y & 1;
    const int tc = (int)(blockIdx.x * 64 + threadIdx.x) - 32768;
    const int sh = lg + 4, off = (1 << sh) >> 1;
    const HeadK hk = head_consts(sh, off, k->lsc);
    const HeadT ht = head_ranges(k, lg);
    const int qd = quotient(k, tc, sh, off);
    bool bad;
    const int alpha = head_alpha(tc, qd, dcn, hk, &bad);
    const bool rbad = head_bad(tc, dcn, ht);
    if (bad && !rbad) atomicAdd(out + 0, 1);
    if (!bad && rbad) atomicAdd(out + 1, 1);
    if ((qd >= 2) != head_sig(tc, ht)) atomicAdd(out + 2, 1);
    if (alpha != head_alpha1(tc, hk)) atomicAdd(out + 3, 1);
}

// DevConst::avail_tab + the picture's edges (block_avail_mask) against the formulas (block_avail_formula): one block per
// thread -- blockIdx.x = CTU, threadIdx.x = 4x4 position, blockIdx.y = size -- for luma and chroma spacing; *out +=
// differences
__global__ __launch_bounds__(64) void test_avail_tab_kernel(const DevConst* __restrict__ kk, int* out) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)kk;
    c.W = kk->W;
    c.ctu_x = 32 * (int)(blockIdx.x % (unsigned)kk->ctu_cols);
    c.ctu_y = 32 * (int)(blockIdx.x / (unsigned)kk->ctu_cols);
    const int lg = 2 + (int)blockIdx.y;
    const int bx = 4 * (int)(threadIdx.x & 7), by = 4 * (int)(threadIdx.x >> 3);
    if ((bx | by) & ((1 << lg) - 1)) return;
    for (int st = 1; st <= 2; ++st)
        if (block_avail_formula(c, bx, by, lg, st) != block_avail_mask(c, bx, by, lg, st)) atomicAdd(out, 1);
    // what cclm_params reads off the mask
    const int m = block_avail_mask(c, bx, by, lg, 1), tn = 1 << lg, gx = c.ctu_x + bx, gy = c.ctu_y + by;
    if (above_right_avail(c, bx, by, lg) != (((m >> 4) & 1) != 0)) atomicAdd(out, 1);
    if (below_left_avail(c, bx, by, lg) != ((m & 1) != 0)) atomicAdd(out, 1);
    if (nb_avail(c, gx, gy, tn, gx - 1, gy, false, false) != (((m >> 1) & 1) != 0)) atomicAdd(out, 1);
    if (nb_avail(c, gx, gy, tn, gx, gy - 1, false, false) != (((m >> 3) & 1) != 0)) atomicAdd(out, 1);
}

// quantize_p16_reg (the packed 4x4 leaf search's quantiser): each wave takes up to four consecutive 4x4 blocks
__global__ __launch_bounds__(64) void test_quantize_p16_kernel(const DevConst* __restrict__ k, const int16_t* in, int count,
                                                               int16_t* out, long long* cost, int* overflow) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    load_tables(c);
    const int first = 4 * blockIdx.x;
    const int nb = min(4, count - first);
    const bool mine = threadIdx.x < 16 * nb;
    int ovf = 0, any = 0;
    long long lvl[4];
    // the lane's coefficient in, the lane's level out
    const int level = quantize_p16_reg(c, nb, mine ? (int)in[(size_t)first * 16 + threadIdx.x] : 0, &ovf, lvl, &any);
    if (mine) out[(size_t)first * 16 + threadIdx.x] = (int16_t)level;
    if (threadIdx.x == 0) {
        for (int b = 0; b < nb; ++b) cost[first + b] = lvl[b];
        if (ovf) atomicOr(overflow, 1);
    }
}

// The register transforms of the 4x4 passes (dev_transform.h): four consecutive 4x4 blocks per wave, lane = (block,
// sample); forward: residuals -> fwd_dct4_reg; inverse: levels -> dequantize4_lane -> inv_dct4_reg.  Every lane runs the
// transform (rows past the last block carry zeros) and only the lanes of a block load and store.
__global__ __launch_bounds__(64) void test_dct4_reg_kernel(const DevConst* __restrict__ k, const int16_t* in, int count, int inverse,
                                                           int16_t* out) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    const size_t at = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool mine = at < (size_t)count * 16;
    const int v = mine ? (int)in[at] : 0;
    const int r = inverse ? inv_dct4_reg(dequantize4_lane(c, v)) : fwd_dct4_reg(v);
    if (mine) out[at] = (int16_t)r;
}

// quantize_pk (the packed leaf searches' quantiser): one wave per pack of nc candidates
__global__ __launch_bounds__(64) void test_quantize_pk_kernel(const DevConst* __restrict__ k, const int16_t* in, int lgl, int nc,
                                                              int16_t* out, long long* cost, int* overflow) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    load_tables(c);
    const int total = nc * 3 * (1 << (2 * lgl)) / 2;
    for (int i = threadIdx.x; i < total; i += 64) SH.r1[i] = in[(size_t)blockIdx.x * total + i];
    WSYNC();
    int ovf = 0;
    bool any_y = false, any_c = false;
    long long ly[3], lc[3];
    if (lgl == 3)
        quantize_pk<3>(c, nc, &ovf, ly, lc, &any_y, &any_c);
    else
        quantize_pk<4>(c, nc, &ovf, ly, lc, &any_y, &any_c);
    for (int i = threadIdx.x; i < total; i += 64) out[(size_t)blockIdx.x * total + i] = SH.r1[i];
    if (threadIdx.x == 0) {
        for (int b = 0; b < nc; ++b) {
            cost[((size_t)blockIdx.x * nc + b) * 2] = ly[b];
            cost[((size_t)blockIdx.x * nc + b) * 2 + 1] = lc[b];
        }
        if (ovf) atomicOr(overflow, 1);
    }
}

__global__ __launch_bounds__(64) void test_dequantize_kernel(const DevConst* __restrict__ k,
                                                             const int16_t* in, int lg, int nb, int o1, int16_t* out) {
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    const int n = 1 << lg, nn = n * n, total = nb * nn;
    for (int i = threadIdx.x; i < total; i += 64) SH.r1[o1 + i] = in[(size_t)blockIdx.x * total + i];
    WSYNC();
    dequantize_t(c, lg, nb, o1);
    for (int i = threadIdx.x; i < total; i += 64) { // undo the transpose, block by block
        const int ii = i & (nn - 1);
        out[(size_t)blockIdx.x * total + i] = ((const int16_t*)SH.r2)[(i - ii) + (ii & (n - 1)) * n + (ii >> lg)];
    }
}

// Prediction of single blocks in the environment of given reconstruction planes (one wave per item):
// the CTU's reconstruction tile and border are loaded from the planes, then reference samples +
// prediction run exactly as in a full evaluation of the final pass (prediction bytes to scratch).
// item = {x, y (luma, picture), log2 luma size, comp (0 luma block, 1 Cb+Cr pair), mode, output offset}
// comp 3 + comps (comps: bit 0 luma, bit 1 the chroma pair): a SAD LIST (sad_list_angular) of the block against its own samples
// in the planes as "originals"; mode = m0 | entries << 8 | stride << 16, entry j = m0 + j * stride (kNoMode beyond 66); the
// output is the 16 accumulators of lanes 0..15 (u32 each); comp 7: the CCLM SAD list of the chroma pair (mode 0), same output
// comp 8 / 9: a FULL candidate (predict_full) of the luma block / the chroma pair into the recon tile, residuals against the
// block's own samples in the planes as originals (a CTU tile of originals is staged for c.org, and stage_org_leaf runs for
// blocks <= 16x16, as in the search); comp 10: the luma part of an 8x8 pack (predict_pack8_luma) into PRED_PARK, mode =
// m0 | m1 << 8 | m2 << 16 | candidates << 24; comp 11: a 16x16 pack, luma and chroma pair (pack16_predict), into
// PRED_PARK16, mode = m0 | m1 << 8 | candidates << 24 (a candidate mode of 255 = kNoMode rides along as zeros).  The output
// is the prediction bytes read back from the destination, in the layout of the destination, then the i16 residuals of r1.
constexpr int kTestPredictScratch = 1024 + kOrgTile; // per item: PRED_SCRATCH | the CTU's tile of originals
__global__ __launch_bounds__(64) void test_predict_kernel(const DevConst* __restrict__ k, const uint8_t* planes,
                                                          const int* items, uint8_t* scratch, uint8_t* out) {
    const int* it = items + 6 * blockIdx.x;
    const int x = it[0], y = it[1], tlg = it[2], comp = it[3], mode = it[4];
    Ctx c = {};
    c.k = (const CONST_AS DevConst*)k;
    c.org = (const GLOBAL_AS uint8_t*)planes; // residuals are computed against these and ignored
    c.W = k->W;
    c.WH = k->W * k->H;
    c.pred_scratch = scratch + (size_t)blockIdx.x * kTestPredictScratch;
    c.ctu_x = x & ~31;
    c.ctu_y = y & ~31;
    c.write = 1;
    load_tables(c);
    const int W = c.W, Wc = W >> 1;
    const GLOBAL_AS uint8_t* rec = (const GLOBAL_AS uint8_t*)planes;
    for (int i = LANE; i < 72; i += 64) {
        const int gx = c.ctu_x - 4 + i, gy = c.ctu_y - 1;
        SH.recYtop[i] = (gx >= 0 && gx < W && gy >= 0) ? rec[(size_t)gy * W + gx] : 0;
    }
    for (int i = LANE; i < 32 * 36; i += 64) {
        const int yy = i / 36, xx = i % 36 - 4;
        const int gx = c.ctu_x + xx, gy = c.ctu_y + yy;
        SH.recY[yy * 36 + xx + 4] = gx >= 0 ? rec[(size_t)gy * W + gx] : 0;
    }
    for (int pc = 1; pc < 3; ++pc) {
        for (int i = LANE; i < 40; i += 64) {
            const int gx = (c.ctu_x >> 1) - 4 + i, gy = (c.ctu_y >> 1) - 1;
            SH.recCtop[pc - 1][i] = (gx >= 0 && gx < Wc && gy >= 0) ? rec[plane_off(c, pc) + (size_t)gy * Wc + gx] : 0;
        }
        for (int i = LANE; i < 16 * 20; i += 64) {
            const int yy = i / 20, xx = i % 20 - 4;
            const int gx = (c.ctu_x >> 1) + xx, gy = (c.ctu_y >> 1) + yy;
            SH.recC[pc - 1][yy * 20 + xx + 4] = gx >= 0 ? rec[plane_off(c, pc) + (size_t)gy * Wc + gx] : 0;
        }
    }
    WSYNC();
    const int tx = x & 31, ty = y & 31;
    if (comp == 2) {
        // the packed predictor of the 4x4 leaf search: the item's mode in row 0, other modes in the rows next to it
        build_refs(c, 0, tx, ty, 2);
        const int row = LANE >> 4;
        const int v = predict4_lane(c, row == 0 ? mode : (mode + 1 + 22 * row) % 67);
        if (LANE < 16) out[it[5] + LANE] = (uint8_t)v;
        return;
    }
    if (comp == 7) { // the CCLM SAD list of the chroma pair (sad_list_cclm): lanes 0..2 = LT_CCLM, T_CCLM, L_CCLM
        uint8_t* oc = (uint8_t*)SH.r2 + org_byte(1, tlg);
        const int nc = 1 << (tlg - 1);
        for (int i = LANE; i < 2 * nc * nc; i += 64) {
            const int pl = i >= nc * nc ? 1 : 0, ii = i - pl * nc * nc;
            oc[i] = rec[plane_off(c, 1 + pl) + (size_t)((y >> 1) + ii / nc) * Wc + (x >> 1) + ii % nc];
        }
        WSYNC();
        const unsigned acc = sad_list_cclm(c, tx, ty, tlg);
        if (LANE < 16) ((uint32_t*)(out + it[5]))[LANE] = acc;
        return;
    }
    if (comp >= 4 && comp < 8) {
        const int comps = comp - 3, m0 = mode & 255, nm = (mode >> 8) & 255, stride = mode >> 16;
        // the originals where a SAD list reads them (stage_org / stage_org_leaf's layout): luma, then Cb | Cr
        uint8_t* ol = (uint8_t*)SH.r2 + org_byte(0, tlg);
        uint8_t* oc = (uint8_t*)SH.r2 + org_byte(1, tlg);
        const int n = 1 << tlg, nc = n >> 1;
        for (int i = LANE; i < n * n; i += 64) ol[i] = rec[(size_t)(y + (i >> tlg)) * W + x + (i & (n - 1))];
        if (comps & 2)
            for (int i = LANE; i < 2 * nc * nc; i += 64) {
                const int pl = i >= nc * nc ? 1 : 0, ii = i - pl * nc * nc;
                oc[i] = rec[plane_off(c, 1 + pl) + (size_t)((y >> 1) + ii / nc) * Wc + (x >> 1) + ii % nc];
            }
        WSYNC();
        if (comps & 1) build_refs(c, 0, tx, ty, tlg);
        if (comps & 2) build_refs(c, 1, tx, ty, tlg);
        unsigned long long lo = 0, hi = 0;
        for (int j = 0; j < nm; ++j) {
            const int m = m0 + j * stride;
            const unsigned long long e = (unsigned long long)(m <= 66 ? m : kNoMode) << (8 * (j & 7));
            if (j < 8) lo |= e; else hi |= e;
        }
        const unsigned acc = sad_list_angular(c, comps, tx, ty, tlg, nm, lo, hi);
        if (LANE < 16) ((uint32_t*)(out + it[5]))[LANE] = acc;
        return;
    }
    if (comp >= 8) {
        // the CTU's originals as retile_kernel lays them out: Y 32x32 | Cb 16x16 | Cr 16x16 (samples outside the picture: 0)
        uint8_t* tile = c.pred_scratch + 1024;
        for (int i = LANE; i < kOrgTile; i += 64) {
            const int pc = i < 1024 ? 0 : 1 + ((i - 1024) >> 8);
            const int ii = pc ? (i - 1024) & 255 : i;
            const int lgw = pc ? 4 : 5;
            const int gx = (pc ? c.ctu_x >> 1 : c.ctu_x) + (ii & ((1 << lgw) - 1)), gy = (pc ? c.ctu_y >> 1 : c.ctu_y) + (ii >> lgw);
            const int pw = pc ? Wc : W, ph = pc ? k->H >> 1 : k->H;
            tile[i] = (gx < pw && gy < ph) ? rec[plane_off(c, pc) + (size_t)gy * pw + gx] : 0;
        }
        __threadfence_block();
        WSYNC();
        c.org = (const GLOBAL_AS uint8_t*)tile;
        const int comps = comp == 8 ? 1 : (comp == 9 ? 2 : (comp == 10 ? 1 : 3));
        if (tlg <= 4) stage_org_leaf(c, comps, tx, ty, tlg);
        uint8_t* op = out + it[5];
        if (comp <= 9) {
            const int cmp = comp - 8;
            if (mode < LT_CCLM) build_refs(c, cmp, tx, ty, tlg);
            predict_full(c, cmp, tx, ty, tlg, mode, 0, PRED_TILE);
            const int lg = tlg - cmp, n = 1 << lg, total = (cmp ? 2 : 1) * n * n;
            for (int i = LANE; i < total; i += 64) {
                const int blk = i >> (2 * lg), ii = i & (n * n - 1);
                op[i] = (uint8_t)rec_get(cmp + blk, (tx >> cmp) + (ii & (n - 1)), (ty >> cmp) + (ii >> lg));
                ((int16_t*)(op + total))[i] = SH.r1[i];
            }
            return;
        }
        const int nc = mode >> 24, m0 = mode & 255, m1 = (mode >> 8) & 255, m2 = (mode >> 16) & 255;
        if (comp == 10) {
            build_refs(c, 0, tx, ty, 3);
            predict_pack8_luma(c, nc, m0, m1, m2);
            WSYNC();
            const uint8_t* park = (const uint8_t*)SH.decw + kParkByte;
            for (int i = LANE; i < 64 * nc; i += 64) {
                op[i] = park[i];
                ((int16_t*)(op + 64 * nc))[i] = SH.r1[i];
            }
            return;
        }
        build_refs(c, 0, tx, ty, 4);
        build_refs(c, 1, tx, ty, 4);
        pack16_predict(c, tx, ty, nc, m0, m1);
        WSYNC();
        for (int i = LANE; i < 384 * nc; i += 64) {
            op[i] = *park16(i, 256 * nc);
            ((int16_t*)(op + 384 * nc))[i] = SH.r1[i];
        }
        return;
    }
    if (mode < LT_CCLM) build_refs(c, comp, tx, ty, tlg);
    predict_full(c, comp, tx, ty, tlg, mode, 0, PRED_SCRATCH);
    const int n = 1 << (tlg - (comp ? 1 : 0));
    const int total = (comp ? 2 : 1) * n * n;
    __threadfence_block();
    for (int i = LANE; i < total; i += 64) out[it[5] + i] = c.pred_scratch[i];
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

struct wrenc_gpu_ctx {
    wrenc_gpu_config cfg;
    long long wave_slots = 0;                  // waves of the search kernel the device holds at once
    long long device_wave_slots = 0;           // (wave_slots can be overridden by a test: wrenc_gpu_test_set_wave_slots)
    // Device memory, streams and events belong to DevBuf, HipStream and HipEvent members (host_mem.h): `delete ctx`
    // releases them, wrenc_gpu_destroy lists none of them.
    HipStream stream;                          // lane 0 of the encode; timing events
    HipStream copy_stream;                     // uploads and downloads: they overlap the search of other slots
    HipEvent ev_uploaded;                      // end of the uploads an encode call has to wait for
    bool uploads_pending = false;
    std::vector<HipEvent> enc_events;          // ring: one "this encode call is done" event per call in flight
    size_t enc_event_next = 0;
    std::vector<hipEvent_t> slot_event;        // per slot: the event (of enc_events) of the encode call that last searched it
    std::vector<HipStream> lanes;              // extra encode lanes (pictures are independent)
    std::vector<HipEvent> lane_done;
    HipEvent ev_fork;
    hipEvent_t last_done = nullptr;            // completion event (of enc_events) of the most recent encode call
    // One constant block per QP in use: the context's from wrenc_gpu_create, the others from wrenc_gpu_set_slot_qp on first
    // use.  A block is never changed or freed while the context lives (a call in flight may read it); the lambdas it was
    // built from are what a later config for the same QP must repeat.
    struct QpConst {
        DevBuf<DevConst> d;
        int64_t lambda_q = 0;
        float lambda_rd = 0.f, lambda_rd_chroma = 0.f;
    };
    QpConst qconst[64];
    const DevConst* ctx_const() const { return qconst[cfg.qp].d.get(); }
    // per-picture QP (wrenc_gpu_set_slot_qp): the QP of every slot; per encode call in flight (ring of enc_events), the
    // call's picture list and its groups (grown on demand), host copy kept until the call is done
    std::vector<int> slot_qp;
    struct CallList {
        DevBuf<PicBufs> d_pics;
        DevBuf<CallGroup> d_groups;             // (one per WPB entries of d_pics)
        std::vector<PicBufs> pics;
        std::vector<CallGroup> groups;
    };
    std::vector<CallList> call_lists;
    // what a slot's PicBufs points into: Y | Cb | Cr as one slab each for originals, reconstruction and levels
    struct SlotMem {
        DevBuf<uint8_t> org, org_t, border, rec;
        DevBuf<int16_t> lev;
        DevBuf<uint32_t> lev_dirty;
        DevBuf<uint8_t> cu_log2, luma_mode, chroma_mode;
        DevBuf<float> ctu_cost;
    };
    std::vector<SlotMem> slot_mem;
    DevBuf<PicBufs> d_slots;
    std::vector<PicBufs> slots;
    std::vector<int> state; // 0 empty, 1 uploaded, 2 encoded
    // the size of the caller's pictures (wrenc_gpu_set_visible_size); the coded size unless one is set
    int vis_w = 0, vis_h = 0;
    bool any_upload = false;
    // a scaling context (wrenc_gpu_set_source_size): the size of the caller's pictures (0: none set, the visible size), the
    // staging planes the upload copies them into (one set per context: copies, scaler, pad and retile of every slot run
    // on copy_stream, in order, so a picture is scaled out of them before the next one is copied in), the filter's tables
    // (one allocation) and the kernel's arguments but for the slot
    int src_w = 0, src_h = 0;
    DevBuf<uint8_t> d_stage, d_scale_tab;
    ScaleArgs scale_args = {};
    // the format of the caller's pictures (wrenc_gpu_set_source_format; 0: planar 8-bit 4:2:0, the plain upload) and the raw
    // staging planes wrenc_gpu_upload_planes copies them into as they come: one set per context, like the scaler's and by
    // the same argument, allocated when the format is set or, where the sizes came later, at the first upload
    int src_format = 0;
    DevBuf<uint8_t> d_raw;
    DevBuf<unsigned long long> d_mismatch;
    DevBuf<int> d_overflow;
    // made by the first encode call, both or neither:
    DevBuf<uint8_t> d_pred_scratch; // kScratchSlots x WPB x kWaveScratch: saved reconstructions (dev_search.h copy_block)
    DevBuf<unsigned long long> d_slot_map; // kScratchSlots bits: scratch regions in use
    HipEvent ev_begin, ev_end;
    std::vector<HipEvent> ev_pool;             // two per span of the plan (encode_plan.h): around a lane's launches of a diagonal
    Plan plan;                                 // of the most recent encode call; its vectors are reused from call to call
    std::vector<int> call_qp;                  // ... and the QPs of its pictures, what the plan was made from
    bool stats_enabled = false; // per-launch timing events: bench / profiling only (wrenc_gpu_stats_enable)
    // Per-call scratch of the read-backs that wait for the search, grown on demand: each call asks its buffers for what
    // its pictures need (DevBuf::grow), and a buffer that is large enough stays.
    // compact read-back: masks, payloads with room for every block, counts
    DevBuf<uint32_t> d_cmask;
    DevBuf<int16_t> d_cpayload;
    DevBuf<unsigned> d_ccount;
    // token read-back: the page pool of one call, its allocation counter, the CTUs' first pages
    DevBuf<uint32_t> d_tok_pool;
    DevBuf<unsigned> d_tok_counter;
    DevBuf<uint32_t> d_tok_first;
    // metrics read-back: the waves' partial sums of one call and the pictures' totals
    DevBuf<MetricsPartial> d_mpartial;
    DevBuf<MetricsSums> d_msums;
    // hash read-back (made on first use: a context that never asks launches and allocates what it always did): a stream
    // of its own -- an MD5 pass is long, and on the copy stream it would stand in front of the next batch's uploads --,
    // the CRC's tables, the waves' partials of one call and the pictures' values, grown on demand
    HipStream hash_stream;
    DevBuf<HashTables> d_htables;
    DevBuf<uint32_t> d_hpartial;
    DevBuf<wrenc_picture_hash> d_hvalues;
    HipEvent hash_ev[2];                        // measurement mode (stats_enabled): around the last hash pass
    bool hash_timed = false;
    // complexity read-back: the waves' triples, the pictures' totals and CTU maps of one call, for every slot at once
    // (allocated on first use and never again: a later call must not free device memory under a search in flight)
    DevBuf<ComplexityPartial> d_xpartial, d_xsums;
    DevBuf<uint32_t> d_xmap;
    // rate histogram read-back: the waves' counts of one call and the pictures' tables, for every slot at once (allocated
    // on first use and never again, as the complexity scratch)
    DevBuf<RateHistPartial> d_rpartial;
    DevBuf<RateHistCounts> d_rsums;
    int schedule = WRENC_GPU_SCHEDULE_AUTO;
    bool stats_valid = false;
    std::string err;
    int ctu_cols = 0, ctu_rows = 0;
};

namespace {

int fail(wrenc_gpu_ctx* ctx, int code, const std::string& msg) {
    if (ctx)
        ctx->err = msg;
    else
        g_create_error = msg;
    return code;
}

// returns WRENC_GPU_EHIP where `expr` fails.  HIP's last error is cleared then, so that the next call's launch check
// (hipGetLastError) does not report this failure as its own; what the caller holds in DevBufs is freed by the return.
#define HIP_TRY(ctx, expr)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (void)hipGetLastError();                                                              \
            return fail(ctx, WRENC_GPU_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
        }                                                                                         \
    } while (0)

size_t plane_bytes(const wrenc_gpu_config& c, int comp, size_t elem) {
    const size_t w = comp ? c.width / 2 : c.width, h = comp ? c.height / 2 : c.height;
    return w * h * elem;
}

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

} // namespace

namespace {
// `count` groups of `nb` blocks to the device, launch(d_in, d_out) on the context's stream, as many blocks back.
// kernel_ms: NULL, or where the HIP-event duration of what `launch` queued goes (the 32x32 micro-benchmark)
template <class Launch>
int run_block_test(wrenc_gpu_ctx* ctx, const int16_t* in, int log2n, int count, int16_t* out, Launch launch, int nb = 1,
                   float* kernel_ms = nullptr) {
    if (!ctx || !in || !out) return WRENC_GPU_EINVAL;
    if (log2n < 2 || log2n > 5 || count < 1 || nb < 1) return fail(ctx, WRENC_GPU_EINVAL, "log2n must be 2..5 and count >= 1");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t)count * nb << (2 * log2n);
    HipEvent e0, e1;
    DevBuf<int16_t> d_in, d_out;
    HIP_TRY(ctx, d_in.alloc(n));
    HIP_TRY(ctx, d_out.alloc(n));
    if (kernel_ms) {
        *kernel_ms = 0.f;
        HIP_TRY(ctx, e0.create());
        HIP_TRY(ctx, e1.create());
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_in.get(), in, n * sizeof(int16_t), hipMemcpyHostToDevice, ctx->stream.get()));
    if (kernel_ms) HIP_TRY(ctx, hipEventRecord(e0.get(), ctx->stream.get()));
    launch(d_in.get(), d_out.get());
    HIP_TRY(ctx, hipGetLastError());
    if (kernel_ms) HIP_TRY(ctx, hipEventRecord(e1.get(), ctx->stream.get()));
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out.get(), n * sizeof(int16_t), hipMemcpyDeviceToHost, ctx->stream.get()));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
    if (kernel_ms) HIP_TRY(ctx, hipEventElapsedTime(kernel_ms, e0.get(), e1.get()));
    return WRENC_GPU_OK;
}

// A picture of a test entry's own (never a slot of the context): up to two sets of three planes of the context's size, Y |
// Cb | Cr as one slab each like a slot's, in `slab`.  `pic`: NULL, or where the device's PicBufs of it goes.
int load_test_picture(wrenc_gpu_ctx* ctx, const uint8_t* const org[3], const uint8_t* const rec[3], DevBuf<uint8_t>& slab,
                      DevBuf<PicBufs>* pic) {
    const wrenc_gpu_config& c = ctx->cfg;
    const size_t wh = (size_t)c.width * c.height;
    HIP_TRY(ctx, slab.alloc(((org ? 1 : 0) + (rec ? 1 : 0)) * (wh + wh / 2)));
    PicBufs pb = {};
    uint8_t* at = slab.get();
    for (int p = 0; p < 6; ++p) {
        const uint8_t* const* from = p < 3 ? org : rec;
        if (!from) continue;
        const int comp = p % 3;
        if (p < 3) pb.org[comp] = at; else pb.rec[comp] = at;
        HIP_TRY(ctx, hipMemcpy(at, from[comp], plane_bytes(c, comp, 1), hipMemcpyHostToDevice));
        at += plane_bytes(c, comp, 1);
    }
    if (!pic) return WRENC_GPU_OK;
    HIP_TRY(ctx, pic->alloc(1));
    HIP_TRY(ctx, hipMemcpy(pic->get(), &pb, sizeof(pb), hipMemcpyHostToDevice));
    return WRENC_GPU_OK;
}

// the quantiser test entries' own overflow word (d_overflow[1]), read once the entry's kernel has finished and cleared
// again whatever `rc`, the entry's status so far, is: the call that raised it fails with WRENC_GPU_ELEVEL -- or with the
// earlier failure `rc` names --, and the next call on the context starts clean either way
// (include/wrenc_gpu.h: "keep a word of their own and never poison a context")
int take_test_overflow(wrenc_gpu_ctx* ctx, int rc) {
    int ovf = 0;
    hipError_t e = hipMemcpyAsync(&ovf, ctx->d_overflow.get() + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream.get());
    if (e == hipSuccess) e = hipMemsetAsync(ctx->d_overflow.get() + 1, 0, sizeof(int), ctx->stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream.get());
    if (rc != WRENC_GPU_OK) return rc;
    if (e != hipSuccess) return fail(ctx, WRENC_GPU_EHIP, hipGetErrorString(e));
    if (!ovf) return WRENC_GPU_OK;
    return fail(ctx, WRENC_GPU_ELEVEL, "a quantised level reached 1024 (reference panics: block_splitter.rs:453)");
}
} // namespace

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

// the metrics pass over n pictures of `slots` from `first` on, on `st`: the waves' partial sums, then the pictures' totals
// (maps: the test entry's per-window values, else NULL)
// vw x vh: the rectangle that is measured, the coded size or a context's visible size (the window variant of the kernel)
static hipError_t launch_metrics(const wrenc_gpu_config& c, int vw, int vh, hipStream_t st, const PicBufs* slots, int first, int n,
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

static void fill_metrics(int vw, int vh, const MetricsSums& s, wrenc_gpu_metrics& m) {
    for (int p = 0; p < 3; ++p) {
        m.sse[p] = s.sse[p];
        m.ssim_sum[p] = s.ssim[p];
        m.ssim_windows[p] = (uint32_t)met_plane(vw, vh, p ? 1 : 0).windows;
    }
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

int wrenc_gpu_test_metrics(wrenc_gpu_ctx* ctx, const uint8_t* const org[3], const uint8_t* const rec[3], wrenc_gpu_metrics* out,
                           float* const ssim_map[3]) {
    if (!ctx || !org || !rec || !out) return WRENC_GPU_EINVAL;
    for (int p = 0; p < 3; ++p)
        if (!org[p] || !rec[p]) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_metrics: null plane");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const wrenc_gpu_config& c = ctx->cfg;
    const MetPlane L = met_plane(c.width, c.height, 0), C = met_plane(c.width, c.height, 1);
    const size_t n_win = (size_t)L.windows + 2 * (size_t)C.windows;
    DevBuf<uint8_t> d_planes;
    DevBuf<PicBufs> d_pic;
    DevBuf<MetricsPartial> d_part;
    DevBuf<MetricsSums> d_sums;
    DevBuf<float> d_map;
    MetricsSums sums = {};
    std::vector<float> map(ssim_map ? n_win : 0);
    if (const int rc = load_test_picture(ctx, org, rec, d_planes, &d_pic)) return rc;
    HIP_TRY(ctx, d_part.alloc((size_t)(L.waves + 2 * C.waves)));
    HIP_TRY(ctx, d_sums.alloc(1));
    if (ssim_map) HIP_TRY(ctx, d_map.alloc(n_win));
    HIP_TRY(ctx, launch_metrics(c, c.width, c.height, 0, d_pic.get(), 0, 1, d_part.get(), d_sums.get(), d_map.get()));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(&sums, d_sums.get(), sizeof(sums), hipMemcpyDeviceToHost));
    if (ssim_map) HIP_TRY(ctx, hipMemcpy(map.data(), d_map.get(), n_win * sizeof(float), hipMemcpyDeviceToHost));
    fill_metrics(c.width, c.height, sums, *out);
    if (ssim_map) {
        const size_t at[3] = {0, (size_t)L.windows, (size_t)L.windows + (size_t)C.windows};
        for (int p = 0; p < 3; ++p)
            if (ssim_map[p]) memcpy(ssim_map[p], map.data() + at[p], (size_t)(p ? C.windows : L.windows) * sizeof(float));
    }
    return WRENC_GPU_OK;
}

// the hash pass over n pictures of `slots` from `first` on, on `st` (dev_hash.h): an MD5 lane per plane, or the waves'
// partials and the finish; `tables` is read by the CRC only
static hipError_t launch_hashes(const wrenc_gpu_config& c, hipStream_t st, const PicBufs* slots, int first, int n, int hash_type,
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

static size_t hash_partials(const wrenc_gpu_config& c) {
    return (size_t)hash_plane(c.width, c.height, 0).pieces + 2 * (size_t)hash_plane(c.width, c.height, 1).pieces;
}

// the CRC's tables, in place before anything queued on `st` after this call reads them
static hipError_t upload_hash_tables(HashTables* d_tables, hipStream_t st) {
    HashTables t;
    hash_fill_tables(t);
    const hipError_t e = hipMemcpyAsync(d_tables, &t, sizeof(t), hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
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

int wrenc_gpu_test_hash(wrenc_gpu_ctx* ctx, const uint8_t* const rec[3], int hash_type, wrenc_picture_hash* out) {
    if (!ctx || !rec || !out) return WRENC_GPU_EINVAL;
    if (hash_type != WRENC_HASH_MD5 && hash_type != WRENC_HASH_CRC && hash_type != WRENC_HASH_CHECKSUM)
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_hash: unknown hash type");
    for (int p = 0; p < 3; ++p)
        if (!rec[p]) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_hash: null plane");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const wrenc_gpu_config& c = ctx->cfg;
    DevBuf<uint8_t> d_planes;
    DevBuf<PicBufs> d_pic;
    DevBuf<HashTables> d_tables;
    DevBuf<uint32_t> d_part;
    DevBuf<wrenc_picture_hash> d_values;
    if (const int rc = load_test_picture(ctx, nullptr, rec, d_planes, &d_pic)) return rc;
    HIP_TRY(ctx, d_tables.alloc(1));
    HIP_TRY(ctx, d_part.alloc(hash_partials(c)));
    HIP_TRY(ctx, d_values.alloc(1));
    HIP_TRY(ctx, upload_hash_tables(d_tables.get(), 0));
    HIP_TRY(ctx, launch_hashes(c, 0, d_pic.get(), 0, 1, hash_type, d_tables.get(), d_part.get(), d_values.get()));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out, d_values.get(), sizeof(*out), hipMemcpyDeviceToHost));
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

int wrenc_gpu_test_head_ranges(wrenc_gpu_ctx* ctx, int counts[4], int ranges[24]) {
    if (!ctx || !counts) return WRENC_GPU_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    DevBuf<int> d;
    HIP_TRY(ctx, d.alloc(4));
    HIP_TRY(ctx, hipMemset(d.get(), 0, 4 * sizeof(int)));
    hipLaunchKernelGGL(test_head_ranges_kernel, dim3(1024, 8), dim3(64), 0, 0, ctx->ctx_const(), d.get());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(counts, d.get(), 4 * sizeof(int), hipMemcpyDeviceToHost));
    if (ranges) {
        DevConst* hk = new DevConst;
        fill_dev_const(ctx->cfg, *hk);
        memcpy(ranges, hk->head_rng, sizeof(hk->head_rng));
        delete hk;
    }
    return WRENC_GPU_OK;
}

int wrenc_gpu_test_avail_tab(wrenc_gpu_ctx* ctx, int* differences) {
    if (!ctx || !differences) return WRENC_GPU_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    DevBuf<int> d;
    HIP_TRY(ctx, d.alloc(1));
    HIP_TRY(ctx, hipMemset(d.get(), 0, sizeof(int)));
    hipLaunchKernelGGL(test_avail_tab_kernel, dim3(ctx->ctu_cols * ctx->ctu_rows, 4), dim3(64), 0, 0, ctx->ctx_const(), d.get());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(differences, d.get(), sizeof(int), hipMemcpyDeviceToHost));
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

// ---- building-block entry points ----

// the 32x32 forward transform runs as i8 MFMAs on two base-256 digits of the residual (fwd_dct32_mfma): exact for
// |residual| <= 255, which is all the search can produce; the test entries refuse anything else
static bool residuals_fit_9_bits(const int16_t* res, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (res[i] < -255 || res[i] > 255) return false;
    return true;
}

// What the group entries refuse, before anything is allocated or launched: a group the device functions are not written
// for or that does not fit the wave's buffers (r1: 1024 i16 from o1 on; r2: the 1024 i16 of the scan-order or transposed
// blocks).  nb_max: 2 for the quantiser (a luma block or the Cb + Cr pair).  nullptr = fine.
static const char* group_shape_error(int log2n, int nb, int o1, int nb_max) {
    if (log2n < 2 || log2n > 5) return "log2n must be 2..5";
    if (nb < 1 || nb > nb_max) return "nb outside what the device function takes";
    if (log2n == 5 && nb > 1) return "a 32x32 block is always alone";
    if (o1 < 0 || (o1 & 1)) return "o1 must be even and >= 0";
    if ((nb << (2 * log2n)) > 1024) return "the group does not fit r2";
    if (o1 + (nb << (2 * log2n)) > 1024) return "the group does not fit r1 behind o1";
    return nullptr;
}
constexpr int kGroupMaxBlocks = 64; // (1024 / 16: group_shape_error's size rules are what bounds a transform group)

// The 8x8 and 16x16 transforms exist as i8 MFMAs too (fwd_dct_mfma / inv_dct_mfma; the search runs them at 16x16):
// 16-byte row reads, so o1 a multiple of 8, and for the forward transform |residual| <= 255.  The search has both by
// construction; a test group that has not runs the retained v_dot2 templates (the host decides before the launch: no
// data-dependent branch on the device).
static bool group_takes_mfma(const int16_t* res, int log2n, int nb, int o1, int count, bool inverse) {
    if (o1 & 7) return false;
    return inverse || count < 1 || residuals_fit_9_bits(res, (size_t)count * ((size_t)nb << (2 * log2n)));
}
// use_mfma: -1 = the plain entries: what the search runs at this size where the group meets its preconditions, else the
// v_dot2 templates; 0 = the v_dot2 templates; 1 = the MFMA versions, or EINVAL
static int run_dct_group(wrenc_gpu_ctx* ctx, const int16_t* in, int log2n, int nb, int o1, int count, int16_t* out,
                         int use_mfma, int reps, float* kernel_ms, bool inverse) {
    if (!ctx || !in || !out || reps < 1) return WRENC_GPU_EINVAL;
    if (const char* why = group_shape_error(log2n, nb, o1, kGroupMaxBlocks)) return fail(ctx, WRENC_GPU_EINVAL, why);
    if (!inverse && log2n == 5 && count >= 1 && !residuals_fit_9_bits(in, (size_t)count * 1024))
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_fwd_dct: a 32x32 residual lies outside +-255");
    int arm = DCT_SEARCH; // (4x4 and 32x32: nothing to choose)
    if (log2n == 3 || log2n == 4) {
        const bool takes = group_takes_mfma(in, log2n, nb, o1, count, inverse);
        if (use_mfma == 1 && !takes)
            return fail(ctx, WRENC_GPU_EINVAL, "the MFMA transforms take residuals within +-255 and an o1 that is a multiple of 8");
        arm = use_mfma == 1 ? DCT_MFMA : (use_mfma == 0 || !takes ? DCT_VDOT2 : DCT_SEARCH);
    }
    float ms = 0.f;
    const int rc = run_block_test(ctx, in, log2n, count, out, [&](int16_t* i, int16_t* o) {
        if (inverse)
            hipLaunchKernelGGL(test_inv_dct_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, log2n, nb, o1, o, arm, reps);
        else
            hipLaunchKernelGGL(test_fwd_dct_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, log2n, nb, o1, o, arm, reps);
    }, nb, kernel_ms ? &ms : nullptr);
    if (kernel_ms) *kernel_ms = ms;
    return rc;
}
int wrenc_gpu_test_fwd_dct_nb(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int nb, int o1, int count, int16_t* coef) {
    return run_dct_group(ctx, res, log2n, nb, o1, count, coef, -1, 1, nullptr, false);
}
int wrenc_gpu_test_fwd_dct_mfma(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int nb, int o1, int count, int16_t* coef,
                                int use_mfma, int reps, float* kernel_ms) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (log2n != 3 && log2n != 4) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_fwd_dct_mfma: log2n must be 3 or 4");
    return run_dct_group(ctx, res, log2n, nb, o1, count, coef, use_mfma ? 1 : 0, reps, kernel_ms, false);
}
int wrenc_gpu_test_inv_dct_mfma(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int nb, int o1, int count, int16_t* res,
                                int use_mfma, int reps, float* kernel_ms) {
    if (!ctx) return WRENC_GPU_EINVAL;
    if (log2n != 3 && log2n != 4) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_inv_dct_mfma: log2n must be 3 or 4");
    return run_dct_group(ctx, deq, log2n, nb, o1, count, res, use_mfma ? 1 : 0, reps, kernel_ms, true);
}
int wrenc_gpu_test_fwd_dct(wrenc_gpu_ctx* ctx, const int16_t* res, int log2n, int count, int16_t* coef) {
    return wrenc_gpu_test_fwd_dct_nb(ctx, res, log2n, 1, 0, count, coef);
}
// a 32x32 transform micro-benchmark: `count` blocks, `reps` repetitions each, HIP-event duration of the one kernel
static int run_dct32_bench(wrenc_gpu_ctx* ctx, const int16_t* in, int count, int16_t* out, int use_mfma, int reps,
                           float* kernel_ms, bool inverse) {
    if (!ctx || !in || !out || count < 1 || reps < 1) return WRENC_GPU_EINVAL;
    if (!inverse && use_mfma && !residuals_fit_9_bits(in, (size_t)count * 1024))
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_fwd_dct32: a residual lies outside +-255 (MFMA path)");
    float ms = 0.f;
    const int rc = run_block_test(ctx, in, 5, count, out, [&](int16_t* i, int16_t* o) {
        if (inverse)
            hipLaunchKernelGGL(test_inv_dct32_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, o, use_mfma, reps);
        else
            hipLaunchKernelGGL(test_fwd_dct32_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, o, use_mfma, reps);
    }, 1, &ms);
    if (kernel_ms) *kernel_ms = ms;
    return rc;
}
int wrenc_gpu_test_fwd_dct32(wrenc_gpu_ctx* ctx, const int16_t* res, int count, int16_t* coef, int use_mfma, int reps,
                             float* kernel_ms) {
    return run_dct32_bench(ctx, res, count, coef, use_mfma, reps, kernel_ms, false);
}
int wrenc_gpu_test_inv_dct32(wrenc_gpu_ctx* ctx, const int16_t* deq, int count, int16_t* res, int use_mfma, int reps,
                             float* kernel_ms) {
    return run_dct32_bench(ctx, deq, count, res, use_mfma, reps, kernel_ms, true);
}
int wrenc_gpu_test_inv_dct_nb(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int nb, int o1, int count, int16_t* res) {
    return run_dct_group(ctx, deq, log2n, nb, o1, count, res, -1, 1, nullptr, true);
}
int wrenc_gpu_test_inv_dct(wrenc_gpu_ctx* ctx, const int16_t* deq, int log2n, int count, int16_t* res) {
    return wrenc_gpu_test_inv_dct_nb(ctx, deq, log2n, 1, 0, count, res);
}
int wrenc_gpu_test_fwd_dct4_reg(wrenc_gpu_ctx* ctx, const int16_t* res, int count, int16_t* coef) {
    return run_block_test(ctx, res, 2, count, coef, [&](int16_t* i, int16_t* o) {
        hipLaunchKernelGGL(test_dct4_reg_kernel, dim3((count + 3) / 4), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, count, 0, o);
    });
}
int wrenc_gpu_test_inv_dct4_reg(wrenc_gpu_ctx* ctx, const int16_t* levels, int count, int16_t* res) {
    return run_block_test(ctx, levels, 2, count, res, [&](int16_t* i, int16_t* o) {
        hipLaunchKernelGGL(test_dct4_reg_kernel, dim3((count + 3) / 4), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, count, 1, o);
    });
}
int wrenc_gpu_test_dequantize_nb(wrenc_gpu_ctx* ctx, const int16_t* levels, int log2n, int nb, int o1, int count, int16_t* deq) {
    if (!ctx || !levels || !deq) return WRENC_GPU_EINVAL;
    if (const char* why = group_shape_error(log2n, nb, o1, kGroupMaxBlocks)) return fail(ctx, WRENC_GPU_EINVAL, why);
    return run_block_test(ctx, levels, log2n, count, deq, [&](int16_t* i, int16_t* o) {
        hipLaunchKernelGGL(test_dequantize_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, log2n, nb, o1, o);
    }, nb);
}
int wrenc_gpu_test_dequantize(wrenc_gpu_ctx* ctx, const int16_t* levels, int log2n, int count, int16_t* deq) {
    return wrenc_gpu_test_dequantize_nb(ctx, levels, log2n, 1, 0, count, deq);
}
// (any_level may be null: the one-block entry does not hand it on)
int wrenc_gpu_test_quantize_nb(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int nb, int count, int16_t* levels,
                               int64_t* level_cost, int32_t* any_level) {
    if (!ctx || !coef || !levels || !level_cost) return WRENC_GPU_EINVAL;
    if (const char* why = group_shape_error(log2n, nb, 0, 2)) return fail(ctx, WRENC_GPU_EINVAL, why);
    if (count < 1) return fail(ctx, WRENC_GPU_EINVAL, "count must be >= 1");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    DevBuf<long long> d_cost;
    DevBuf<int> d_any;
    return take_test_overflow(ctx, [&]() -> int {
        HIP_TRY(ctx, d_cost.alloc((size_t)count));
        HIP_TRY(ctx, d_any.alloc((size_t)count));
        const int rc = run_block_test(ctx, coef, log2n, count, levels, [&](int16_t* i, int16_t* o) {
            hipLaunchKernelGGL(test_quantize_kernel, dim3(count), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, log2n, nb, o,
                               d_cost.get(), d_any.get(), ctx->d_overflow.get() + 1);
        }, nb);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpy(level_cost, d_cost.get(), sizeof(long long) * count, hipMemcpyDeviceToHost));
        if (any_level) HIP_TRY(ctx, hipMemcpy(any_level, d_any.get(), sizeof(int) * count, hipMemcpyDeviceToHost));
        return WRENC_GPU_OK;
    }());
}
int wrenc_gpu_test_quantize(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int count, int16_t* levels,
                            int64_t* level_cost) {
    return wrenc_gpu_test_quantize_nb(ctx, coef, log2n, 1, count, levels, level_cost, nullptr);
}

int wrenc_gpu_test_quantize_p16(wrenc_gpu_ctx* ctx, const int16_t* coef, int count, int16_t* levels, int64_t* level_cost) {
    if (!ctx || !level_cost) return WRENC_GPU_EINVAL;
    if (count < 1) return fail(ctx, WRENC_GPU_EINVAL, "count must be >= 1");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    DevBuf<long long> d_cost;
    return take_test_overflow(ctx, [&]() -> int {
        HIP_TRY(ctx, d_cost.alloc((size_t)count));
        const int rc = run_block_test(ctx, coef, 2, count, levels, [&](int16_t* i, int16_t* o) {
            hipLaunchKernelGGL(test_quantize_p16_kernel, dim3((count + 3) / 4), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), i, count, o,
                               d_cost.get(), ctx->d_overflow.get() + 1);
        });
        if (rc) return rc;
        HIP_TRY(ctx, hipMemcpy(level_cost, d_cost.get(), sizeof(long long) * count, hipMemcpyDeviceToHost));
        return WRENC_GPU_OK;
    }());
}

int wrenc_gpu_test_quantize_pk(wrenc_gpu_ctx* ctx, const int16_t* coef, int log2n, int nc, int n_packs, int16_t* levels,
                               int64_t* level_cost) {
    if (!ctx || !coef || !levels || !level_cost) return WRENC_GPU_EINVAL;
    if (!((log2n == 3 && nc >= 1 && nc <= 3) || (log2n == 4 && nc >= 1 && nc <= 2)) || n_packs < 1)
        return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_quantize_pk: log2n 3 with nc 1..3 or log2n 4 with nc 1..2");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const size_t total = (size_t)n_packs * nc * 3 * ((size_t)1 << (2 * log2n)) / 2;
    const size_t n_costs = (size_t)2 * nc * n_packs;
    DevBuf<int16_t> d_in, d_out;
    DevBuf<long long> d_cost;
    return take_test_overflow(ctx, [&]() -> int {
        HIP_TRY(ctx, d_in.alloc(total));
        HIP_TRY(ctx, d_out.alloc(total));
        HIP_TRY(ctx, d_cost.alloc(n_costs));
        HIP_TRY(ctx, hipMemcpy(d_in.get(), coef, total * sizeof(int16_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(test_quantize_pk_kernel, dim3(n_packs), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), d_in.get(), log2n, nc,
                           d_out.get(), d_cost.get(), ctx->d_overflow.get() + 1);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
        HIP_TRY(ctx, hipMemcpy(levels, d_out.get(), total * sizeof(int16_t), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(level_cost, d_cost.get(), sizeof(long long) * n_costs, hipMemcpyDeviceToHost));
        return WRENC_GPU_OK;
    }());
}

int wrenc_gpu_test_predict(wrenc_gpu_ctx* ctx, const uint8_t* rec_y, const uint8_t* rec_cb, const uint8_t* rec_cr,
                           int n_items, const int32_t* items, uint8_t* out, size_t out_bytes) {
    if (!ctx || !rec_y || !rec_cb || !rec_cr || !items || !out || n_items < 1) return WRENC_GPU_EINVAL;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    // operand shapes are checked on the host: a bad item must never reach the kernel
    std::vector<int> dev_items((size_t)n_items * 6);
    size_t total = 0;
    for (int i = 0; i < n_items; ++i) {
        const int32_t* q = items + 5 * i;
        const int x = q[0], y = q[1], lg = q[2], comp = q[3], mode = q[4];
        const int n = 1 << lg;
        const bool list = comp >= 4 && comp <= 6; // a SAD list: mode = m0 | entries << 8 | stride << 16
        const int m0 = mode & 255, nm = (mode >> 8) & 255, stride = mode >> 16;
        bool ok = lg >= 2 && lg <= 5 && x >= 0 && y >= 0 && x + n <= W && y + n <= H && !(x & (n - 1)) && !(y & (n - 1));
        const bool pack = comp == 10 || comp == 11; // mode = m0 | m1 << 8 | m2 << 16 | candidates << 24, 255 = kNoMode
        const int pk_nc = mode >> 24;
        if (pack) {
            ok = ok && mode >= 0 && lg == (comp == 10 ? 3 : 4) && pk_nc >= 1 && pk_nc <= (comp == 10 ? 3 : 2);
            for (int j = 0; ok && j < pk_nc; ++j) {
                const int m = (mode >> (8 * j)) & 255;
                ok = m <= 66 || m == kNoMode;
            }
        } else if (comp == 8 || comp == 9) {
            ok = ok && (comp == 8 || lg >= 3) && ((mode >= 0 && mode <= 66) || (comp == 9 && mode >= LT_CCLM && mode <= T_CCLM));
        } else {
            ok = ok && (comp == 0 || (comp == 1 && lg >= 3) || (comp == 2 && lg == 2) || (comp == 4) || (list && lg >= 3) ||
                        (comp == 7 && lg >= 3)) &&
                 (comp == 7 ? mode == 0 : list ? (mode >= 0 && m0 >= 2 && m0 <= 66 && nm >= 1 && nm <= 16 && stride >= 1 && stride <= 64)
                       : ((mode >= 0 && mode <= 66) || (comp == 1 && mode >= LT_CCLM && mode <= T_CCLM)));
        }
        if (!ok) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_predict: bad item");
        int* d = &dev_items[(size_t)i * 6];
        d[0] = x; d[1] = y; d[2] = lg; d[3] = comp; d[4] = mode; d[5] = (int)total;
        // (the full-candidate items: prediction bytes, then as many i16 residuals)
        total += (list || comp == 7) ? 64 : comp == 8 ? 3 * (size_t)n * n : comp == 9 ? 3 * (size_t)n * n / 2
                 : comp == 10 ? 3 * 64 * (size_t)pk_nc : comp == 11 ? 3 * 384 * (size_t)pk_nc
                 : (comp == 1 ? (size_t)n * n / 2 : (size_t)n * n);
    }
    if (total != out_bytes) return fail(ctx, WRENC_GPU_EINVAL, "wrenc_gpu_test_predict: output size does not match the items");
    HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
    const uint8_t* const rec[3] = {rec_y, rec_cb, rec_cr};
    DevBuf<uint8_t> d_planes, d_scratch, d_out;
    DevBuf<int> d_items;
    if (const int rc = load_test_picture(ctx, nullptr, rec, d_planes, nullptr)) return rc;
    HIP_TRY(ctx, d_scratch.alloc((size_t)n_items * kTestPredictScratch));
    HIP_TRY(ctx, d_out.alloc(total));
    HIP_TRY(ctx, d_items.alloc(dev_items.size()));
    HIP_TRY(ctx, hipMemcpy(d_items.get(), dev_items.data(), dev_items.size() * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(test_predict_kernel, dim3(n_items), dim3(64), 0, ctx->stream.get(), ctx->ctx_const(), d_planes.get(), d_items.get(),
                       d_scratch.get(), d_out.get());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream.get()));
    HIP_TRY(ctx, hipMemcpy(out, d_out.get(), total, hipMemcpyDeviceToHost));
    return WRENC_GPU_OK;
}

} // extern "C"
