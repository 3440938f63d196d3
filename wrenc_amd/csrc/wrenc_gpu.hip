// wrenc_gpu.hip -- the search of the MI355X all-intra RD-search path: its kernels and the entries of the C ABI
// (include/wrenc_gpu.h) that create a context, queue an encode call and report on it.  Built for gfx950 only, together with
// the library's other units, each a code object (or plain host code) of its own, so nothing there reaches the code of the
// kernels here:
//   wrenc_gpu_io.hip    pictures in and results out: every upload path and every read-back, with their kernels
//   const_block.cpp     host only: the constant block (DevConst) and the rate model, from a config alone
//   wrenc_gpu_test.hip  the block tests: the kernels and entries of include/wrenc_gpu_test.h
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -o libwrenc_gpu.so wrenc_gpu.hip wrenc_gpu_io.hip
//         const_block.cpp wrenc_gpu_test.hip
//
// Scheduling: a picture's CTUs depend on their left, above-left, above and
// above-right neighbours (encoder_context.rs:934-948), so CTU (r, c) can run once
// every CTU on anti-diagonal c + 2r - 1 is done.  One launch processes one
// anti-diagonal of every picture of the batch (one wave per CTU); stream order
// between launches is the only synchronisation between CTUs.  (The one in-kernel
// wait is a workgroup's acquire of a scratch region from a bitmap that always has
// more regions than workgroups can be resident, see ctu_search_kernel.)
#include "wrenc_dev.h"
#include "gpu_ctx.h"

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

extern "C" {

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
    std::string msg;
    const int rc = config_extra_params(cfg, extra_params, msg);
    return rc ? fail(nullptr, rc, msg) : WRENC_GPU_OK;
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
    if (ctx->recon_stream) (void)hipStreamSynchronize(ctx->recon_stream.get());
    delete ctx; // (frees the device memory and destroys the streams and events: every stream has been synchronised above)
}

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
    // a wrenc_gpu_download_recon_device queued without a host wait may still be reading a reconstruction this call rewrites
    if (ctx->recon_read_pending) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream.get(), ctx->ev_recon_read.get(), 0));
        ctx->recon_read_pending = false;
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
