// gpu_ctx.h -- what the HIP units of libwrenc_gpu.so share (private to them): the context, the error path and the host
// functions that more than one of the search's entry points (wrenc_gpu.hip), the picture I/O (wrenc_gpu_io.hip) and the
// block tests (wrenc_gpu_test.hip) call.  Each of those functions is defined once, in the unit named at its declaration,
// and stays inside the library (hidden visibility).  The device headers come from the units themselves: this file needs
// dev_common.h alone, and the read-backs' device types by name only.
#pragma once
#include "../../include/wrenc_gpu.h"
#include "../../include/wrenc_scale.h"
#include "../../include/wrenc_format.h"
#include "../../include/wrenc_rgb.h"
#include "../../include/wrenc_recon.h"
#include "../../include/wrenc_hash.h"
#include "../../include/wrenc_ratecurve.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.h"
#include "scale_args.h"
#include "const_block.h"
#include "encode_plan.h"
#include "host_mem.h"

#include <string>
#include <vector>

using namespace wrenc;

namespace wrenc {
// what the read-backs' scratch holds (dev_metrics.h, dev_hash.h, dev_complexity.h, dev_ratecurve.h, dev_distcurve.h): complete in
// wrenc_gpu_io.hip, names only in the search unit.  The context has the same layout in both because a DevBuf<T> is a
// pointer and a count whatever T is (host_mem.h), and destroying or moving one needs no complete T.
struct MetricsPartial;
struct MetricsSums;
struct HashTables;
struct ComplexityPartial;
struct RateHistPartial;
struct RateHistCounts;
struct DistCurveSums;
} // namespace wrenc

// A mixed-QP encode call (wrenc_gpu_set_slot_qp) runs its pictures from a per-call list, ordered by QP and padded so that
// every group of WPB consecutive entries holds ONE QP: load_tables fills the workgroup's LDS tables (lambda_q x dq_table)
// with each thread reading its own wave's constant block, so a workgroup must never mix blocks.  Per group: the QP's
// constant block and how many of its WPB entries are pictures (the rest are padding: same work, no stores).
struct CallGroup {
    const DevConst* k;
    int n_real;
};

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
    // an RGB source (wrenc_gpu_set_source_rgb; layout -1: none): exclusive with a non-zero format, the same raw staging
    // planes, dev_rgb.h's converter in the place of dev_format.h's
    int src_rgb = -1, rgb_matrix = 0, rgb_range = 0;
    // device-resident planes (wrenc_gpu_upload_planes_device; made on first use): "the producer stream has written the
    // planes" for copy_stream to wait for, and "the copies have read them" for the producer stream to wait for
    HipEvent ev_producer, ev_copied;
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
    // reconstruction out (wrenc_gpu_download_recon, _download_recon_device; all made on first use): a stream of its own, as
    // the hashes have and for the same reason; the staging planes the kernels of dev_recon.h write, one set per context
    // with room for the largest output format, reused by the next call behind this one's copies (one stream, in order);
    // the device entry's events: "the consumer stream has reached the call" for the copies to wait for, "the copies are
    // done" for the consumer stream to wait for, and "the kernel has read the slot's reconstruction", which the next
    // encode call waits for while recon_read_pending (the host entry returns behind its kernel and leaves nothing pending)
    HipStream recon_stream;
    DevBuf<uint8_t> d_recon;
    HipEvent ev_consumer, ev_recon_copied, ev_recon_read;
    bool recon_read_pending = false;
    // complexity read-back: the waves' triples, the pictures' totals and CTU maps of one call, for every slot at once
    // (allocated on first use and never again: a later call must not free device memory under a search in flight)
    DevBuf<ComplexityPartial> d_xpartial, d_xsums;
    DevBuf<uint32_t> d_xmap;
    // rate histogram read-back: the waves' counts of one call and the pictures' tables, for every slot at once (allocated
    // on first use and never again, as the complexity scratch)
    DevBuf<RateHistPartial> d_rpartial;
    DevBuf<RateHistCounts> d_rsums;
    // distortion curve read-back: the waves' sums of one call and the pictures' tables, by the same rule
    DevBuf<DistCurveSums> d_dpartial, d_dsums;
    int schedule = WRENC_GPU_SCHEDULE_AUTO;
    bool stats_valid = false;
    std::string err;
    int ctu_cols = 0, ctu_rows = 0;
};

// wrenc_gpu.hip: the message goes to the context, or (ctx NULL: wrenc_gpu_create) to the thread's creation error; returns `code`
WRENC_HIDDEN int fail(wrenc_gpu_ctx* ctx, int code, const std::string& msg);

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

WRENC_HIDDEN size_t plane_bytes(const wrenc_gpu_config& c, int comp, size_t elem); // wrenc_gpu.hip
// (fill_dev_const, which the block tests call too, and the rate model: const_block.h)
// wrenc_gpu_io.hip: the slots of a call exist and are uploaded (min_state 1) or searched (2)
WRENC_HIDDEN int check_slots(wrenc_gpu_ctx* ctx, int first, int n, int min_state, const char* range_msg);
// wrenc_gpu_io.hip: the metrics and hash passes over pictures of any PicBufs array, on any stream (comments at the definitions)
WRENC_HIDDEN hipError_t launch_metrics(const wrenc_gpu_config& c, int vw, int vh, hipStream_t st, const PicBufs* slots, int first, int n,
                                       MetricsPartial* partials, MetricsSums* sums, float* maps);
WRENC_HIDDEN void fill_metrics(int vw, int vh, const MetricsSums& s, wrenc_gpu_metrics& m);
WRENC_HIDDEN hipError_t launch_hashes(const wrenc_gpu_config& c, hipStream_t st, const PicBufs* slots, int first, int n, int hash_type,
                                      const HashTables* tables, uint32_t* partials, wrenc_picture_hash* values);
WRENC_HIDDEN size_t hash_partials(const wrenc_gpu_config& c);
