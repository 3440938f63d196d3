// dev_search.h -- evaluation requests and the evaluator, the leaf / CTU search state machines, CTU entry (block_splitter.rs, ctu_encoder.rs:1421-1461)
// Part of the gfx950 device code of the RD-search path; see wrenc_dev.h for the overall model.
#pragma once

namespace wrenc {

// ---------------------------------------------------------------------------
// RD search building blocks (block_splitter.rs)
// ---------------------------------------------------------------------------
// Evaluation requests and the evaluator
// ---------------------------------------------------------------------------
// (the numbers index the profile build's counters, tools/phase_profile.py: 6 stays free)
enum { K_SADLIST = 0, K_FULL = 1, K_NOP = 2, K_SADSEARCH = 3, K_CCLMSEARCH = 4, K_SERVE8 = 5, K_LEAF8 = 7, K_LEAF16 = 8, K_SPLIT8 = 9, K_SERVE4 = 10,
       K_NODE8 = 11, K_LEAF32 = 12 };
enum { COPY_NONE = 0, COPY_SAVE = 1, COPY_RESTORE = 2, COPY_PULL = 3 };

// Split cut (wave schedule): a node's children are searched only until their partial cost, summed in z-order in f32 from
// 0.0 as the full sum is (:1116-1123), with every child still to come counted at its floor (split_floor_cut below), is
// strictly greater than the node's unsplit cost.  Every child costs at least its floor, every floor is >= 0 and f32
// addition is monotone in either operand, so the final sum is >= this bound: the
// comparison of :1125-1145 is decided (a tie would still go to the split, so equality searches on), the unsplit
// candidate is restored over the whole node exactly as after the last child, and what the skipped children would have
// written is never read.  Off in the trace build, which exists to pin the candidates that lose (tests/test_gpu_trace.py),
// and with -DWRENC_EXHAUSTIVE_SPLITS (A/B measurements, tools/README.md).  The team / level schedule stays exhaustive
// whatever the build: its members search a node and its subtree at the same time, so a node's unsplit cost is not
// known when its children start.
#if defined(WRENC_TRACE) || defined(WRENC_EXHAUSTIVE_SPLITS)
constexpr bool kSplitCut = false;
#else
constexpr bool kSplitCut = true;
#endif

// Candidate cut (wave schedule, leaf4_search): a full candidate of a 4x4 DUAL_TREE_LUMA leaf costs rd_cost(ssd, level cost
// + hb_luma[1][0][cls], lambda) with ssd >= 0 and level cost >= 0, and its class is known from the MPM list before anything
// is evaluated.  rd_cost is monotone in both integer arguments for lambda >= 0 (conversion to f32, the product and the
// sum each are, contraction being off), so rd_cost(0, hb_luma[1][0][cls], lambda) -- DevConst::cand_floor, formed by the
// host with the same operations -- is <= that candidate's cost.  The leaf takes the first minimum as a running
// strict-less update, so a candidate whose floor is >= the running best cannot win: it is not evaluated, and the leaf
// returns what it returns when that candidate loses.  Off in the trace build, which records every candidate, and with
// -DWRENC_EXHAUSTIVE_CANDIDATES (A/B measurements, tools/README.md); the team and level schedules, whose members run
// pack A may come from the pack-A server, stay exhaustive.
#if defined(WRENC_TRACE) || defined(WRENC_EXHAUSTIVE_CANDIDATES)
constexpr bool kCandidateCut = false;
#else
constexpr bool kCandidateCut = true;
#endif

struct Req {
    int kind;       // K_FULL: predict .. reconstruct (block_splitter.rs:146-185) of a 32x32 candidate of the team schedule or a
                    // final-pass block;
                    // K_NOP: nothing but the pre_copy;
                    // K_SADSEARCH (team kernels): the whole SAD part of a 32x32 leaf search in
                    // one request -- the 13 directional candidates, their first minimum and the two step-search
                    // rounds around it (:899-973): returns the mode (Res::imin) and its SAD (Res::vmin);
                    // K_CCLMSEARCH: the CCLM part of a 16x16 / 32x32 leaf search in one request -- the SADs of LT / T / L_CCLM, the
                    // pick (:847-854) and the full evaluation of the chroma pair with it: Res::imin = the mode, + parts;
                    // K_SADLIST: the SAD of the chroma pair under the one CCLM mode mc (:476-522; the team's 32x32
                    // candidate at max-split-depth 0, a probe per member): Res::v0;
                    // K_LEAF8: the whole search of an 8x8 SINGLE_TREE leaf (:886-1078) in one request, its full candidates
                    // evaluated in packs of two and three (leaf8_search): Res::imin / imin2 = luma / chroma mode, vmin = the cost;
                    // K_SERVE8 / K_SERVE4 (team kernel, member 0): pack {planar, DC} of member 2's 8x8 leaf / member 3's 4x4
                    // luma leaf at (tx, ty), results in this wave's LDS (serve_pack8 / serve_pack4);
                    // K_SPLIT8: the split candidate of an 8x8 CU in one request: its four DUAL_TREE_LUMA 4x4 leaf searches, then the
                    // DUAL_TREE_CHROMA one (split8_search); Res::vmin = the split cost (:1116-1123)
                    // K_LEAF16: the five full candidates of a 16x16 SINGLE_TREE leaf and its SAD search in one request, the
                    // candidates in packs of two (leaf16_search): Res::imin = the best luma mode, vmin = its cost, + its parts
                    // K_NODE8 (wave kernel at max-split-depth 3): one 8x8 node decided inside the request -- its unsplit
                    // candidate, its split, the comparison and the restore (node8_search): Res::vmin = the node's cost
                    // K_LEAF32 (wave kernels): the whole search of the CTU's 32x32 SINGLE_TREE leaf in one request, its
                    // candidates one after the other (full_search); its best candidate is kept in slot copy_slot:
                    // Res::vmin = the cost, imin / imin2 = luma / chroma mode
    int comps;     // bit 0: luma block, bit 1: Cb+Cr pair
    int tx, ty, tlg;
    int ml, mc;     // K_FULL: luma / chroma mode; K_SADLIST: mc = the CCLM mode
    bool active;    // false: the request computes nothing (a candidate the reference skips keeps its place in the sequence)
    bool refs0, refs1; // (re)build the luma / chroma reference samples of the block first
    bool final;     // final pass: store the levels, count reconstruction changes
    int stage;      // before anything else: stage the block's originals in LDS (component bits; blocks <= 16x16 only)
    // team schedule only (leaf_step_team): COPY_PULL copies the block from the LDS tile of member copy_from into
    // this member's tile (every member issues it, the source included, and all meet at a barrier behind it);
    // xchg: the team exchanges results after this request
    int copy_from;
    bool xchg;
    int tree;       // tree type of the leaf that asks (diagnostic trace only)
    // before the evaluation: save the block's reconstruction to a slot / restore it from there
    // (the reference's cache_reconsts / restore_reconsts, block_splitter.rs:807-840, 1085-1145)
    int pre_copy, copy_comps, copy_slot, copy_tx, copy_ty, copy_tlg;
    float fcur;     // K_SPLIT8: the 8x8 node's unsplit cost, the search stops once the split's partial cost is greater
                    // (kSplitCut; +inf = search every leaf)
};

struct Res {
    // K_FULL, K_CCLMSEARCH, K_LEAF8, K_LEAF16: SSD and level cost of the luma block and of the chroma pair
    uint32_t ssd_y, ssd_c;
    long long lvl_y, lvl_c;
    float v0;       // K_SADLIST: the SAD
    float vmin;     // K_SADSEARCH: the SAD of the mode found; the packed searches: the cost
    int imin;       // the mode found (K_SADSEARCH, K_CCLMSEARCH) / the luma mode (K_LEAF8, K_LEAF16)
    int imin2;      // K_LEAF8: the chroma mode
};
// nothing evaluated: no parts, f32::MAX, PLANAR
__device__ __forceinline__ Res res_none() {
    Res r;
    r.ssd_y = 0;
    r.ssd_c = 0;
    r.lvl_y = 0;
    r.lvl_c = 0;
    r.v0 = r.vmin = 3.40282347e+38f;
    r.imin = 0;
    r.imin2 = 0;
    return r;
}

__device__ __forceinline__ float uni_f(float v) { return __int_as_float(uni(__float_as_int(v))); }

// The final pass's self-check ("the final pass reproduces the search" as a property to test): a
// position-weighted sum, mod 2^32, of the samples of a block's reconstruction in the tile (comp 0: luma block, 1: chroma
// pair).  Every weight is odd, so a change of any ONE sample changes the sum; changes of several samples cancel with
// probability 2^-32.  (Until round 3 the final pass kept its prediction in global scratch so that the tile still held
// the search's reconstruction when the new one was made, and compared them sample by sample: 1.5 KB per CTU written to
// memory and read back, per block a store -> load round trip through L2.)
__device__ __forceinline__ unsigned checksum_weight(int i) { return (2u * (unsigned)i + 1u) * 0x9E3779B1u; }
__device__ __forceinline__ unsigned tile_checksum(int comp, int cx, int cy, int lg) {
    const int n = 1 << lg, nn = n * n, nb = comp ? 2 : 1;
    unsigned h = 0;
    for (int i = 4 * LANE; i < nb * nn; i += 256) { // a row of four samples per lane: one dword of the tile
        const int blk = i >> (2 * lg), ii = i & (nn - 1);
        const uint32_t w = rec_get4(comp + blk, cx + (ii & (n - 1)), cy + (ii >> lg));
#pragma unroll
        for (int k = 0; k < 4; ++k) h += ((w >> (8 * k)) & 255u) * checksum_weight(i + k);
    }
    return (unsigned)wave_sum_i32((int)h);
}

// First half of a full evaluation of one component (comp 0: luma block, 1: chroma pair): reference
// samples, prediction, forward transform.  Residual / coefficients at r1[rbase ..], prediction bytes
// in the tile (the final pass first takes the checksum of what the search left there).
__device__ __forceinline__ void full_front(const Ctx& c, const Req& q, int comp, int mode, int rbase,
                                           CclmPick pick = CclmPick{}) {
    const int cs = comp ? 1 : 0;
    const int nb = comp ? 2 : 1;
    const int lg = q.tlg - cs;
    PROF_MARK(tr0_);
    if ((comp ? q.refs1 : q.refs0) && mode < LT_CCLM) build_refs(c, comp, q.tx, q.ty, q.tlg);
    if (q.final) {
        const unsigned h = tile_checksum(comp, q.tx >> cs, q.ty >> cs, lg);
        if (LANE == 0) SH.fsum = h;
        WSYNC();
    }
    PROF_MARK(t0_);
    PROF_ADD2(PH_REFS, tr0_, t0_);
    if (comp == 0)
        predict_full<0>(c, q.tx, q.ty, q.tlg, mode, rbase, PRED_TILE, 0, pick);
    else
        predict_full<1>(c, q.tx, q.ty, q.tlg, mode, rbase, PRED_TILE, 0, pick);
    PROF_MARK(t1_);
    PROF_ADD2(PH_PREDICT, t0_, t1_);
    PROF_ADD2(PH_PRED + (mode >= LT_CCLM ? 5 : (q.tlg == 5 ? 0 : (q.tlg == 4 ? 1 : 6))), t0_, t1_);
    fwd_dct_lg(c, lg, nb, rbase);
    PROF_MARK(t2_);
    PROF_ADD2(PH_FDCT, t1_, t2_);
}

// Second half: levels at r1[rbase ..] -> (final pass: store them) -> dequantise, inverse transform,
// reconstruct into the tile; returns the SSD against the originals (block_splitter.rs:146-185)
__device__ __forceinline__ uint32_t full_back(const Ctx& c, const PicBufs& pb, const Req& q, int comp, int rbase,
                                              bool any_level) {
    const int cs = comp ? 1 : 0;
    const int nb = comp ? 2 : 1;
    const int lg = q.tlg - cs;
    const int n = 1 << lg;
    const int nn = n * n;
    const int cx = q.tx >> cs, cy = q.ty >> cs;
    const int obyte = org_byte(comp, q.tlg);
    const bool olds = q.tlg <= 4;
    PROF_MARK(t3_);
    // Final pass: the levels go to the slot's planes -- the 4x4 blocks of them that have any.  A block of zeros is only
    // written where the planes may still hold levels of the slot's previous picture (PicBufs::lev_dirty, loaded into
    // Lds::lev_was when the final pass began): nearly every 4x4 block of nearly all content is zero, and was.
    // A lane takes one row of a 4x4 block (four levels, one 8-byte store), the four rows of a block sit in one quad.
    if (q.final && c.store) {
        const int stride = c.W >> cs;
        const size_t at = (size_t)((c.ctu_y + q.ty) >> cs) * stride + ((c.ctu_x + q.tx) >> cs);
        GLOBAL_AS int16_t* lev0 = AS_GLOBAL(int16_t, pb.lev[0]) + plane_off(c, comp) + at;
        GLOBAL_AS int16_t* lev1 = AS_GLOBAL(int16_t, pb.lev[0]) + plane_off(c, 2) + at;
        const int lgb = lg - 2;                                  // 4x4 blocks per side of the transform block, log2
        const int u0x = (q.tx >> cs) >> 2, u0y = (q.ty >> cs) >> 2; // its place among the CTU's 4x4 blocks of the plane
        const uint32_t w0 = (uint32_t)uni((int)SH.lev_was[0]), w1 = (uint32_t)uni((int)SH.lev_was[1]),
                       w2 = (uint32_t)uni((int)SH.lev_was[2]), w3 = (uint32_t)uni((int)SH.lev_was[3]);
        for (int j = LANE; j < (nb << (2 * lg - 2)); j += 64) {
            const int bq_ = j >> 2, r = j & 3;
            const int pl = bq_ >> (2 * lgb), bq = bq_ & ((1 << (2 * lgb)) - 1);
            const int bby = bq >> lgb, bbx = bq & ((1 << lgb) - 1);
            const int y = 4 * bby + r, x = 4 * bbx;
            const unsigned long long v = *(const unsigned long long*)&SH.r1[rbase + (pl << (2 * lg)) + (y << lg) + x];
            const unsigned long long rows = __ballot(v != 0ULL);
            const bool nzb = ((rows >> (LANE & 60)) & 15ULL) != 0; // the block has a level
            const int ux = u0x + bbx, uy = u0y + bby;
            const int quad = comp ? (uy >> 1) * 2 + (ux >> 1) : (uy >> 2) * 2 + (ux >> 2);
            const int bit = comp ? 16 + (uy & 1) * 2 + (ux & 1) : (uy & 3) * 4 + (ux & 3);
            const uint32_t wq = quad == 0 ? w0 : (quad == 1 ? w1 : (quad == 2 ? w2 : w3));
            if (nzb && r == 0) atomicOr(&SH.lev_now[quad], 1u << bit);
            if (nzb || ((wq >> bit) & 1u)) *(GLOBAL_AS unsigned long long*)&(pl ? lev1 : lev0)[(size_t)y * stride + x] = v;
        }
    }
    // all levels zero: the residual is zero too, and r1 (the levels) already says so
    if (any_level) dequantize_t(c, lg, nb, rbase);
    PROF_MARK(t4_);
    if (any_level) inv_dct_lg(c, lg, nb, rbase);
    PROF_MARK(t5_);
    PROF_ADD2(PH_DEQ, t3_, t4_);
    PROF_ADD2(PH_IDCT, t4_, t5_);
    unsigned int part = 0;
    unsigned hs = 0;
    for (int i = 4 * LANE; i < nb * nn; i += 256) { // a row of four samples per lane (recon_row4)
        const int blk = i >> (2 * lg), ii = i & (nn - 1);
        const int x = ii & (n - 1), y = ii >> lg;
        const int pc = comp + blk;
        const uint32_t org = org_row4(c, comp, blk, cx + x, cy + y, obyte, i, olds);
        int v[4];
        const uint32_t rec = recon_row4(rec_get4(pc, cx + x, cy + y), *(const uint2*)&SH.r1[rbase + i], org, v, part);
        if (q.final) {
#pragma unroll
            for (int k = 0; k < 4; ++k) hs += (unsigned)v[k] * checksum_weight(i + k);
        }
        rec_put4(pc, cx + x, cy + y, rec);
    }
    const uint32_t ssd = (uint32_t)wave_sum_i32((int)part); // <= 1024 * 255^2: fits 32 bits
    if (q.final) { // the block's reconstruction must be what the search left in the tile (tile_checksum, full_front)
        const bool changed = (unsigned)wave_sum_i32((int)hs) != (unsigned)uni((int)SH.fsum);
        if (changed && LANE == 0 && c.store) atomicAdd(c.mismatch, 1ULL);
    }
    WSYNC();
    PROF_MARK(t6_);
    PROF_ADD2(PH_RECON, t5_, t6_);
    PROF_ADD2(PH_REC + 0, t5_, t6_);
    return ssd;
}

// Save the reconstruction of a block (comps bit 0: luma n x n, bit 1: Cb and Cr (n/2) x (n/2)) from
// the LDS tile to a slot in global scratch, or restore it from there.  Dwords: block corners are
// multiples of 4 samples in every plane that takes part.
__device__ __forceinline__ void copy_block(const Ctx& c, int mode, int comps, int slot, int tx, int ty, int tlg,
                                           int from_member = -1) {
    if (mode == COPY_PULL) { // tile to tile inside the workgroup's LDS (team schedule)
        if (from_member != c.member) {
            const Lds& src = SHW[(WAVE & ~(kTeam - 1)) + from_member];
            if (comps & 1) {
                const int words = 1 << (2 * tlg - 2);
                for (int w = LANE; w < words; w += 64) {
                    const int row = (4 * w) >> tlg, col = (4 * w) & ((1 << tlg) - 1);
                    const int at = (ty + row) * 36 + tx + col + 4;
                    *(uint32_t*)&SH.recY[at] = *(const uint32_t*)&src.recY[at];
                }
            }
            if (comps & 2) {
                const int lg = tlg - 1;
                const int words = 1 << (2 * lg - 2); // per plane
                for (int w = LANE; w < 2 * words; w += 64) {
                    const int pl = w >= words ? 1 : 0;
                    const int ww = w - pl * words;
                    const int row = (4 * ww) >> lg, col = (4 * ww) & ((1 << lg) - 1);
                    const int at = ((ty >> 1) + row) * 20 + (tx >> 1) + col + 4;
                    *(uint32_t*)&SH.recC[pl][at] = *(const uint32_t*)&src.recC[pl][at];
                }
            }
        }
        __syncthreads(); // nobody writes its tile again before every member has pulled
        return;
    }
    GLOBAL_AS uint32_t* g = (GLOBAL_AS uint32_t*)(c.slots + slot_offset(slot));
    const int cbase = 1 << (2 * tlg - 2); // the chroma planes follow the block's luma words
    if (comps & 1) {
        const int words = 1 << (2 * tlg - 2);
        for (int w = LANE; w < words; w += 64) {
            const int row = (4 * w) >> tlg, col = (4 * w) & ((1 << tlg) - 1);
            uint32_t* l = (uint32_t*)&SH.recY[(ty + row) * 36 + tx + col + 4];
            if (mode == COPY_SAVE)
                g[w] = *l;
            else
                *l = g[w];
        }
    }
    if (comps & 2) {
        const int lg = tlg - 1;
        const int words = 1 << (2 * lg - 2); // per plane
        for (int w = LANE; w < 2 * words; w += 64) {
            const int pl = w >= words ? 1 : 0;
            const int ww = w - pl * words;
            const int row = (4 * ww) >> lg, col = (4 * ww) & ((1 << lg) - 1);
            uint32_t* l = (uint32_t*)&SH.recC[pl][((ty >> 1) + row) * 20 + (tx >> 1) + col + 4];
            if (mode == COPY_SAVE)
                g[cbase + w] = *l;
            else
                *l = g[cbase + w];
        }
    }
    WSYNC();
}

// The SAD part of a luma / single-tree leaf search: the 13 directional candidates, their first minimum and the two
// step-search rounds around it (block_splitter.rs:899-973).  cm: the mode found, smin: its SAD.
// ONE copy of the list code (sad_list_angular is a couple of thousand instructions, inlined): the rounds are iterations
// of one loop that differ in the list they ask for and in what they do with its SADs.  (Until round 4 the three kinds of
// round were three inlined copies at each of four call sites: a fifth of the kernel's code, in an instruction cache that
// misses on 2.6 % of its fetches -- profiles/r04_issue_model.md.)
__device__ __forceinline__ void sad_search(const Ctx& c, const Req& q, int& cm_out, unsigned& smin_out) {
    constexpr unsigned kNoSad = 0xFFFFFFFFu;
    // Small blocks (8x8 single-tree and 4x4 luma leaves): a list of two entries costs nearly what a list of six does
    // (parameters, tables, reductions: two thirds of it), so BOTH step-search rounds' probes come from ONE list -- round 1's
    // cm -+ 2 and the four modes round 2 can ask for around cm - 2, cm or cm + 2: cm - 3, cm - 1, cm + 1, cm + 3.  A
    // mode's SAD does not depend on the list it is in; the decisions below are the two rounds' in their order, an
    // entry the reference would not evaluate (Q12) is kNoMode here as there, and only the probes the reference makes
    // are traced.
    const bool six = q.tlg <= 3;
    const int rounds = six ? 2 : 3;
    int cm = 0;
    unsigned cur = kNoSad;
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        // ---- the round's list ----
        int n;
        unsigned long long lo, hi = 0;
        int e0 = kNoMode, e1 = kNoMode, e2 = kNoMode, e3 = kNoMode, e4 = kNoMode, e5 = kNoMode;
        const int st = r == 1 ? 2 : 1; // (the step of a two-probe round)
        if (r == 0) {
            // the 13 directional candidates {2,7,13,18,23,29,34,39,45,50,55,60,66} (:899-904)
            n = 13;
            lo = 2ULL | (7ULL << 8) | (13ULL << 16) | (18ULL << 24) | (23ULL << 32) | (29ULL << 40) | (34ULL << 48) | (39ULL << 56);
            hi = 45ULL | (50ULL << 8) | (55ULL << 16) | (60ULL << 24) | (66ULL << 32);
        } else if (six) {
            e0 = !(cm < 4) ? cm - 2 : kNoMode;
            e1 = !(cm + 2 > 66) ? cm + 2 : kNoMode;
            e2 = !(cm < 5) ? cm - 3 : kNoMode;
            e3 = !(cm < 3) ? cm - 1 : kNoMode;
            e4 = !(cm + 1 > 66) ? cm + 1 : kNoMode;
            e5 = !(cm + 3 > 66) ? cm + 3 : kNoMode;
            n = 6;
            lo = (unsigned long long)e0 | ((unsigned long long)e1 << 8) | ((unsigned long long)e2 << 16) | ((unsigned long long)e3 << 24) |
                 ((unsigned long long)e4 << 32) | ((unsigned long long)e5 << 40);
        } else {
            // step_search(mode, 2, cost, aux = true) (:905-973): rounds with step 2 and 1; a probe outside 2..66 is f32::MAX
            e0 = !(cm < 2 + st) ? cm - st : kNoMode;
            e1 = !(cm + st > 66) ? cm + st : kNoMode;
            n = 2;
            lo = (unsigned long long)e0 | ((unsigned long long)e1 << 8);
        }
        const unsigned acc = sad_list_angular(c, q.comps, q.tx, q.ty, q.tlg, n, lo, hi);
        const int my_mode = LANE < n ? (int)(((LANE < 8 ? lo : hi) >> (8 * (LANE & 7))) & 255u) : kNoMode;
        const unsigned s0 = (unsigned)__builtin_amdgcn_readlane((int)acc, 0), s1 = (unsigned)__builtin_amdgcn_readlane((int)acc, 1);
        // ---- what the round does with the SADs.  They are integers < 2^20, so comparing them as integers is comparing the
        // reference's f32 values; keep the current mode on ties, then the lower probe (Q12) ----
        bool traced = my_mode != kNoMode;
        if (r == 0) {
            // first minimum = smallest (sad, index) pair
            const int key = my_mode != kNoMode ? (int)((acc << 4) | (unsigned)LANE) : 0x7FFFFFFF;
            const int kmin = wave_min_i32(key);
            const int j = (kmin & 15) + 2; // entry i = candidate i + 2 of the 15, 7 bits each
            cm = j < 8 ? (int)((0x3A5C90D0E08080ULL >> (7 * j)) & 127) : (int)((0x109E3764B53A2ULL >> (7 * (j - 8))) & 127);
            cur = (unsigned)kmin >> 4;
        } else if (six) {
            const unsigned s2 = (unsigned)__builtin_amdgcn_readlane((int)acc, 2), s3 = (unsigned)__builtin_amdgcn_readlane((int)acc, 3);
            const unsigned s4 = (unsigned)__builtin_amdgcn_readlane((int)acc, 4), s5 = (unsigned)__builtin_amdgcn_readlane((int)acc, 5);
            // round 1, step 2
            const unsigned c0 = e0 != kNoMode ? s0 : kNoSad, c1 = e1 != kNoMode ? s1 : kNoSad;
            const unsigned mn = min(min(cur, c0), c1);
            int d = 0; // cm' - cm
            if (cur == mn) {
            } else if (c0 == mn) {
                d = -2;
                cur = c0;
            } else {
                d = 2;
                cur = c1;
            }
            // round 2, step 1, around cm' = cm + d: its probes are entries 2 + (d + 2) / 2 and 3 + (d + 2) / 2
            const int elo = d < 0 ? e2 : (d == 0 ? e3 : e4), ehi = d < 0 ? e3 : (d == 0 ? e4 : e5);
            const unsigned slo = d < 0 ? s2 : (d == 0 ? s3 : s4), shi = d < 0 ? s3 : (d == 0 ? s4 : s5);
            const unsigned p0 = elo != kNoMode ? slo : kNoSad, p1 = ehi != kNoMode ? shi : kNoSad;
            cm += d;
            const unsigned mn2 = min(min(cur, p0), p1);
            if (cur == mn2) {
            } else if (p0 == mn2) {
                cm -= 1;
                cur = p0;
            } else {
                cm += 1;
                cur = p1;
            }
            const int ilo = d < 0 ? 2 : (d == 0 ? 3 : 4);
            traced = traced && (LANE < 2 || LANE == ilo || LANE == ilo + 1);
        } else {
            const unsigned c0 = e0 != kNoMode ? s0 : kNoSad, c1 = e1 != kNoMode ? s1 : kNoSad;
            const unsigned mn = min(min(cur, c0), c1);
            if (cur == mn) {
            } else if (c0 == mn) {
                cm -= st;
                cur = c0;
            } else {
                cm += st;
                cur = c1;
            }
        }
        if (c.trace && traced)
            TRACE_REC(c.ctu_x + q.tx, c.ctu_y + q.ty, q.tlg, q.tree, (q.comps & 1) ? 0 : 2, (q.comps & 1) ? my_mode : 0, my_mode,
                      __float_as_int((float)acc));
    }
    cm_out = cm;
    smin_out = cur;
}

__device__ __forceinline__ Res leaf8_search(const Ctx& c, const Req& q, int* overflow);
__device__ __forceinline__ Res leaf16_search(const Ctx& c, const Req& q, int* overflow);
__device__ __forceinline__ Res split8_search(const Ctx& c, const Req& q, int* overflow, int* leaves = nullptr);
__device__ __forceinline__ void fill_maps(int bx, int by, int lg, int luma_mode, int chroma_mode, bool luma, bool chroma);
__device__ __forceinline__ void serve_pack4(const Ctx& c, const Req& q, int* overflow);
__device__ __forceinline__ void serve_pack8(const Ctx& c, const Req& q, int* overflow);
template <bool TEAM, bool L32>
__device__ __forceinline__ Res full_search(const Ctx& c, const PicBufs& pb, const Req& q, int* overflow);

// The CCLM probe of a block's chroma pair: get_chroma_intra_pred_aux_cost of LT, T, L_CCLM in one sample pass, their trace
// records, then the pick of block_splitter.rs:847-854 (SADs are integers < 2^20: comparing them is comparing the
// reference's f32 values).  Returns the picked mode; *all = the model parameters of the three modes (cclm_pick takes the
// picked mode's from there).
__device__ __forceinline__ int cclm_probe(const Ctx& c, int tx, int ty, int lg, int tree, CclmParams* all) {
    const int lane = lane_fresh();
    const unsigned acc = sad_list_cclm(c, tx, ty, lg, all);
    const unsigned lt = (unsigned)__builtin_amdgcn_readlane((int)acc, 0), t = (unsigned)__builtin_amdgcn_readlane((int)acc, 1),
                   l = (unsigned)__builtin_amdgcn_readlane((int)acc, 2);
    if (c.trace && lane < 3)
        TRACE_REC(c.ctu_x + tx, c.ctu_y + ty, lg, tree, 2, 0, lane == 0 ? LT_CCLM : (lane == 1 ? T_CCLM : L_CCLM),
                  __float_as_int((float)acc));
    return (lt <= t && lt <= l) ? LT_CCLM : (t <= l ? T_CCLM : L_CCLM);
}

// the CCLM prediction of sample (x, y) of plane pl of the 4x4 chroma pair of q's 8x8 block, in the lane's registers
__device__ __forceinline__ int cclm_pred4_lane(const Ctx& c, const Req& q, const CclmPick& pick, int pl, int x, int y) {
    int v = 128;
    if (!pick.flat128) {
        const int ds = cclm_ds6(c, q.tx, q.ty, 2 * y, 2 * x, pick.avail_l);
        v = (M24(ds, pl ? pick.a1 : pick.a0) >> (pl ? pick.k1 : pick.k0)) + (pl ? pick.b1 : pick.b0);
        v = min(max(v, 0), 255);
    }
    return v;
}

// One 8x8 node of the wave schedule at max-split-depth 3, decided without leaving the request (K_NODE8): the
// SINGLE_TREE leaf search, whose winner with its final DM-or-CCLM chroma is then in the tile; the maps of the unsplit
// candidate; the split's search against the unsplit cost (split8_search, its cuts and floors as they are); the comparison
// of :1125-1145.  The unsplit candidate's reconstruction waits in ONE register per lane meanwhile -- luma sample
// (lane & 7, lane >> 3), and in lanes 0..31 the Cb / Cr sample of the 4x4 pair -- where the walk used to save it to a slot
// in global scratch in front of K_SPLIT8 and to fetch it back with a request of its own: 96 bytes out and in, two
// requests and three control steps per node.  A split that is cut before its first leaf has touched neither the tile
// nor the maps, so nothing is put back.  Returns the node's cost.
__device__ __forceinline__ float node8_search(const Ctx& c, int tx, int ty, int* overflow) {
    Req qn = {}; // (only what the two searches read)
    qn.comps = 3;
    qn.tx = tx;
    qn.ty = ty;
    qn.tlg = 3;
    qn.refs0 = true;
    qn.refs1 = true;
    qn.tree = TREE_SINGLE;
    stage_org_leaf(c, 3, tx, ty, 3);
    const Res ru = leaf8_search(c, qn, overflow);
    const float ns = ru.vmin;
    const int ml = ru.imin, mc = ru.imin2;
    fill_maps(tx, ty, 3, ml, mc, true, true);
    unsigned kept;
    {
        const int lane = lane_fresh();
        kept = (unsigned)rec_get(0, tx + (lane & 7), ty + (lane >> 3));
        if (lane < 32) kept |= (unsigned)rec_get(1 + (lane >> 4), (tx >> 1) + (lane & 3), (ty >> 1) + ((lane & 15) >> 2)) << 8;
    }
    qn.fcur = ns; // (kSplitCut)
    int leaves = 0;
    const float split8 = split8_search(c, qn, overflow, &leaves).vmin;
    if (!(split8 > ns)) return split8; // (a tie is a split)
    if (leaves) { // :1125-1145: the unsplit 8x8 wins, put it back
        const int lane = lane_fresh();
        rec_put(0, tx + (lane & 7), ty + (lane >> 3), (int)(kept & 255u));
        if (lane < 32) rec_put(1 + (lane >> 4), (tx >> 1) + (lane & 3), (ty >> 1) + ((lane & 15) >> 2), (int)(kept >> 8));
        fill_maps(tx, ty, 3, ml, mc, true, true); // (ends in a WSYNC)
    }
    return ns;
}

// The evaluator: every block evaluation of the search, of the regeneration and of the final pass
// goes through this one inlined copy (the search logic below is a state machine that hands out
// evaluation requests; no function calls in the hot path).
// D3: the kernel serves max-split-depth 3 (the only depth at which an 8x8 CU splits into 4x4 leaves): the kernels for
// the smaller depths are built without that code.  TEAM: the team kernel, the only one with a pack-A server.
template <bool TEAM, bool D3>
__device__ __forceinline__ Res evaluate(const Ctx& c, const PicBufs& pb, const Req& q, int* overflow) {
    Res r = res_none();
    PROF_MARK(tcp0_);
    if (q.pre_copy != COPY_NONE)
        copy_block(c, q.pre_copy, q.copy_comps, q.copy_slot, q.copy_tx, q.copy_ty, q.copy_tlg, q.copy_from);
    PROF_MARK(tcp1_);
    PROF_ADD2(PH_COPY, tcp0_, tcp1_);
    if (q.kind == K_NOP) return r;
    if (q.stage) stage_org_leaf(c, q.stage, q.tx, q.ty, q.tlg);
    // (4x4 leaves are searched inside K_SPLIT8 only: nothing asks for one by itself)
    // The wave kernel at max-split-depth 3 searches an 8x8 block only as a node that may split (K_NODE8): its one copy
    // of leaf8_search and its one copy of split8_search are node8_search's
    constexpr bool kNodes = !TEAM && D3;
    if (kNodes && q.kind == K_NODE8) {
        r.vmin = node8_search(c, q.tx, q.ty, overflow);
        return r;
    }
    if (!kNodes && q.kind == K_LEAF8) return leaf8_search(c, q, overflow);
    if (q.kind == K_LEAF16) return leaf16_search(c, q, overflow);
    if (TEAM && D3 && q.kind == K_SPLIT8) return split8_search(c, q, overflow);
    if (TEAM && q.kind == K_SERVE8) { // (member 0 only)
        serve_pack8(c, q, overflow);
        return r;
    }
    if (TEAM && D3 && q.kind == K_SERVE4) { // (the same)
        serve_pack4(c, q, overflow);
        return r;
    }
    // the full evaluations, one by one: a single candidate, the CCLM part of a 16x16 leaf, or (wave kernels) the whole
    // 32x32 leaf -- one copy of the stages for the three (full_search)
    if (!TEAM && q.kind == K_LEAF32) return full_search<TEAM, true>(c, pb, q, overflow);
    if (q.kind == K_FULL || q.kind == K_CCLMSEARCH) return full_search<TEAM, false>(c, pb, q, overflow);
    // K_SADSEARCH / K_SADLIST: get_intra_pred_aux_cost / get_chroma_intra_pred_aux_cost.  Only the team kernels ask for
    // them (leaf_step_team): the wave kernels' 32x32 SAD search runs inside K_LEAF32, so they are built without this copy.
    if constexpr (!TEAM) return r;
    PROF_MARK(tr0_);
    if (q.refs0 && (q.comps & 1)) build_refs(c, 0, q.tx, q.ty, q.tlg);
    if (q.refs1 && (q.comps & 2)) build_refs(c, 1, q.tx, q.ty, q.tlg);
    if (q.tlg > 4) stage_org(c, q.comps, q.tx, q.ty, q.tlg); // smaller blocks: staged once per leaf
    PROF_MARK(t0_);
    PROF_ADD2(PH_REFS, tr0_, t0_);
    // SADs stay integers (< 2^20, so the f32 the reference compares is exact and ordered the same
    // way); they become floats once, at the end.
    if (q.kind == K_SADSEARCH) {
        constexpr unsigned kNoSad = 0xFFFFFFFFu;
        int cm;
        unsigned smin = kNoSad;
        sad_search(c, q, cm, smin);
        r.imin = uni(cm);
        r.vmin = smin == kNoSad ? 3.40282347e+38f : uni_f((float)smin);
    } else { // K_SADLIST: the chroma pair under the CCLM mode q.mc
        PROF_MARK(tp0_);
        const unsigned sad = (unsigned)wave_sum_i32(predict_sad(c, 1, q.tx, q.ty, q.tlg, q.mc));
        PROF_MARK(tp1_);
        PROF_ADD2(PH_PSZ + ((q.tlg - 2) * 2 + 1), tp0_, tp1_);
        PROF_ADD2(PH_PCNT + ((q.tlg - 2) * 2 + 1), 0, 1);
        if (c.trace && LANE == 0)
            TRACE_REC(c.ctu_x + q.tx, c.ctu_y + q.ty, q.tlg, q.tree, 2, 0, q.mc, __float_as_int((float)sad));
        r.v0 = uni_f((float)sad);
    }
    PROF_MARK(t1_);
    PROF_ADD2(PH_PREDICT, t0_, t1_);
    PROF_ADD2(PH_PRED + 7, t0_, t1_);
    return r;
}

// luma mode of the CU covering picture position (CTU-local x, y), as the search sees it
// (SURVEY.md Q7): inside the CTU -> root CU's mode; left CTU -> its final map; else none.
__device__ __forceinline__ int nb_luma_mode(Ctx c, int x, int y, bool* exists) {
    if (x >= 0 && y >= 0) {
        *exists = true;
        return c.cu32_mode;
    }
    if (y >= 0 && x < 0 && c.ctu_x > 0) {
        *exists = true;
        return uni((int)SH.left_mode[y >> 2]);
    }
    *exists = false;
    return PLANAR;
}

// mode class index for the header-bit table: 0 planar, 1..5 mpm_idx, 6..66 remainder
// (ctu.rs:1498-1635)
// The MPM list of a block (ctu.rs:1498-1635) depends on the block alone, not on the candidate mode: the packed leaf
// searches derive it once per leaf (mpm_list) and classify their five candidates against it (mpm_class_of).
struct MpmList {
    int k0, k1, k2, k3, k4;
};
__device__ __forceinline__ MpmList mpm_list(const Ctx& c, int bx, int by, int lg) {
    const int n = 1 << lg;
    bool le, ae;
    int left = nb_luma_mode(c, bx - 1, by + n - 1, &le);
    if (!le) left = PLANAR;
    int above;
    if (by - 1 < 0) {
        // above the CTU: either no CU (picture edge) or forced PLANAR across the CTU row (:1518-1523)
        above = PLANAR;
    } else {
        above = nb_luma_mode(c, bx + n - 1, by - 1, &ae);
        if (!ae) above = PLANAR;
    }
    int k0, k1, k2, k3, k4;
    if (left == above && left > DC) {
        const int m = left;
        k0 = m;
        k1 = 2 + (m + 61) % 64;
        k2 = 2 + (m - 1) % 64;
        k3 = 2 + (m + 60) % 64;
        k4 = 2 + m % 64;
    } else if (left != above && (left > DC || above > DC)) {
        const int mn = min(left, above), mx = max(left, above);
        if (mn > DC) {
            const int d = mx - mn;
            k0 = left;
            k1 = above;
            if (d == 1) {
                k2 = 2 + (mn + 61) % 64;
                k3 = 2 + (mx - 1) % 64;
                k4 = 2 + (mn + 60) % 64;
            } else if (d >= 62) {
                k2 = 2 + (mn - 1) % 64;
                k3 = 2 + (mx + 61) % 64;
                k4 = 2 + mn % 64;
            } else if (d == 2) {
                k2 = 2 + (mn - 1) % 64;
                k3 = 2 + (mn + 61) % 64;
                k4 = 2 + (mx - 1) % 64;
            } else {
                k2 = 2 + (mn + 61) % 64;
                k3 = 2 + (mn - 1) % 64;
                k4 = 2 + (mx + 61) % 64;
            }
        } else {
            k0 = mx;
            k1 = 2 + (mx + 61) % 64;
            k2 = 2 + (mx - 1) % 64;
            k3 = 2 + (mx + 60) % 64;
            k4 = 2 + mx % 64;
        }
    } else {
        k0 = DC;
        k1 = 50;
        k2 = 18;
        k3 = 46;
        k4 = 54;
    }
    MpmList l;
    l.k0 = k0;
    l.k1 = k1;
    l.k2 = k2;
    l.k3 = k3;
    l.k4 = k4;
    return l;
}
// mode class index for the header-bit table: 0 planar, 1..5 mpm_idx, 6..66 remainder
__device__ __forceinline__ int mpm_class_of(const MpmList& l, int mode) {
    if (mode == PLANAR) return 0;
    if (l.k0 == mode) return 1;
    if (l.k1 == mode) return 2;
    if (l.k2 == mode) return 3;
    if (l.k3 == mode) return 4;
    if (l.k4 == mode) return 5;
    // remainder = mode - 1 - #(candidates below mode) after sorting (:1613-1628)
    const int smaller = (l.k0 < mode) + (l.k1 < mode) + (l.k2 < mode) + (l.k3 < mode) + (l.k4 < mode);
    return 6 + (mode - 1 - smaller);
}
__device__ __forceinline__ int mpm_class(const Ctx& c, int bx, int by, int lg, int mode) {
    if (mode == PLANAR) return 0;
    return mpm_class_of(mpm_list(c, bx, by, lg), mode);
}

__device__ __forceinline__ float rd_cost(unsigned long long ssd, long long level, float lambda) {
    // block_splitter.rs:472-473: ssd as f32 + lambda * (level as f32 / 16384.0).  Rust never
    // contracts a*b+c into an FMA; HIP's default -ffp-contract=fast would, so contraction is
    // switched off here (and with -ffp-contract=off on the command line).
#pragma clang fp contract(off)
    const float lv = (float)level * (1.0f / 16384.0f);
    const float prod = lambda * lv;
    return (float)ssd + prod;
}

// SSD and level cost of the luma and of the chroma pair of one evaluated candidate.  Evaluations
// are deterministic functions of (block, mode, neighbourhood[, luma recon for CCLM]), so where the
// reference re-runs an evaluation it has already done (block_splitter.rs:1040,1068-1075) the
// parts are re-used and only the cost is re-assembled.
// get_intra_pred_cost (block_splitter.rs:110-474) from already evaluated parts, modes [ml, mc, mc]
__device__ __forceinline__ float assemble_cost(const Ctx& c, int tree, int cls, int mc, const EvalParts& e) {
    const bool single = tree == TREE_SINGLE;
    const int cc = (single && mc >= LT_CCLM) ? 1 + (mc - LT_CCLM) : 0;
    const unsigned long long ssd = (unsigned long long)e.ssd_y + (single ? (unsigned long long)e.ssd_c : 0ULL);
    const long long level = e.lvl_y + (single ? e.lvl_c : 0LL) + c.k->hb_luma[single ? 0 : 1][cc][cls];
    return rd_cost(ssd, level, c.k->lambda_rd);
}

// get_chroma_intra_pred_cost (block_splitter.rs:524-780) from already evaluated parts
__device__ __forceinline__ float assemble_chroma_cost(const Ctx& c, int mc, const EvalParts& e) {
    const long long level = e.lvl_c + c.k->hb_chroma[mc >= LT_CCLM ? 1 + (mc - LT_CCLM) : 0];
    return rd_cost((unsigned long long)e.ssd_c, level, c.k->lambda_rd_chroma);
}

__device__ __forceinline__ int pick_cclm(float lt, float t, float l) {
    // block_splitter.rs:847-854
    if (lt <= t && lt <= l) return LT_CCLM;
    if (t <= l) return T_CCLM;
    return L_CCLM;
}

// ---------------------------------------------------------------------------
// leaf4_search: the whole search of a 4x4 DUAL_TREE_LUMA leaf in one go (block_splitter.rs:886-1078 with 16 samples
// per candidate).  A full evaluation of a 4x4 block is a chain of fixed-latency stages that keeps 16 of the wave's
// 64 lanes busy, and at max-split-depth 3 these leaves are 61 % of a CTU.  The full candidates of a leaf do not
// depend on each other (they read only neighbours outside the block, :887-898, :974), so they are evaluated SIDE BY
// SIDE, one candidate per 16-lane row: pack A = {planar, DC}, then the SAD search (sad_search), then pack B =
// {cm, cm - 1, cm + 1}.  Every stage computes what the single evaluation's computes, written for rows: a candidate's
// block stays in its 16 lanes' registers from predict4_lane to the reconstruction (pass4_reg below).  The decisions are
// the reference's, in its order: first minimum of [planar, DC, cm, cm - 1, cm + 1] as a running strict-less update; a candidate outside
// 2..66 is not evaluated (f32::MAX there).  The best candidate's reconstruction goes to the tile when its pack is
// done (nothing reads the block's own area meanwhile: the reference samples are cached); no save / restore at all.
// ---------------------------------------------------------------------------
// the LDS working set of member m of this wave's team
__device__ __forceinline__ const Lds& team_lds(const Ctx& c, int m) { return SHW[(WAVE & ~(kTeam - 1)) + m]; }

// Level schedule, the pack-A server (see lv_decide for the schedule): polled LDS words, bounded like lv_meet
__device__ __forceinline__ unsigned lv_word(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lv_word_add(uint32_t* p) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (LANE == 0) __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lv_word_wait(const uint32_t* p, unsigned target) {
    if (LANE == 0) {
        int polls = 0;
        while (lv_word(p) < target) {
            __builtin_amdgcn_s_sleep(2);
            if (++polls > (1 << 23)) {
                SHT.lvb.pad_ = 1;
                break;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    WSYNC();
}

// The 4x4 passes -- pack4_eval, leafc4_search, the chroma blocks of pack8_eval and the CCLM pair of leaf8_search -- keep
// a block in registers from the prediction to the reconstruction: lane = (block, sample), fwd_dct4_reg, quantize_p16_reg
// (quantize_pk for pack8_eval, which takes the coefficients from r1 and leaves the levels there), dequantize4_lane,
// inv_dct4_reg.  All but pack8_eval's run the same function, pass4_reg; evaluate() and the final pass send every 4x4
// block through r1 / r2 with fwd_dct<2>, dequantize_t and inv_dct<2>.
// the lane's residual from its level; "no level of the pass is non-zero" (wave-uniform) gives zero without the transform
__device__ __forceinline__ int residual4_reg(const Ctx& c, int level, bool any_level) {
    int res = 0;
    if (any_level) res = inv_dct4_reg(dequantize4_lane(c, level));
    return res;
}

// One pass of four 4x4 blocks, lane = (block LANE / 16, sample LANE % 16): v = the lane's prediction, org its original,
// on = the lane's block is evaluated (a block that is not, and a row past nb, ride along as zero blocks and count no
// error).  Residual, transform, quantisation of the nb blocks side by side, and back: the lane's reconstruction (pred as
// i16 + res, clamp: :178), its block's SSD summed over the row, the blocks' level costs and "has a non-zero level" bits.
struct Pass4Out {
    int rec, row_ssd;
    long long lvl[4];
    int any_mask;
};
__device__ __forceinline__ Pass4Out pass4_reg(const Ctx& c, int nb, bool on, int v, int org, int* overflow) {
    Pass4Out o;
    PROF_MARK(t1_);
    const int coef = fwd_dct4_reg(on ? org - v : 0);
    PROF_MARK(t2_);
    PROF_ADD2(PH_FDCT, t1_, t2_);
    o.any_mask = 0;
    const int level = quantize_p16_reg(c, nb, coef, overflow, o.lvl, &o.any_mask);
    PROF_MARK(t3_);
    const int res = residual4_reg(c, level, o.any_mask != 0);
    PROF_MARK(t4_);
    PROF_ADD2(PH_IDCT, t3_, t4_);
    const int rec = min(max((int)(int16_t)(v + res), 0), 255);
    const int d = rec - org;
    o.rec = rec;
    o.row_ssd = row_sum_i32(on ? M24(d, d) : 0);
    PROF_MARK(t5_);
    PROF_ADD2(PH_RECON, t4_, t5_);
    PROF_ADD2(PH_REC + 3, t4_, t5_);
    return o;
}

struct Pack4Out {
    uint32_t ssd[3];
    long long lvl[3];
    int rec; // per lane: the reconstructed sample of (candidate LANE / 16, sample LANE % 16)
};
__device__ __forceinline__ Pack4Out pack4_eval(const Ctx& c, const Req& q, int nb, int m0, int m1, int m2, int* overflow) {
    Pack4Out o;
    const int lane = lane_fresh();
    const int s = lane >> 4, i = lane & 15;
    const int mode = s == 0 ? m0 : (s == 1 ? m1 : (s == 2 ? m2 : kNoMode));
    const bool on = s < nb && mode != kNoMode;
    PROF_MARK(t0_);
    const int v = predict4_lane(c, on ? mode : kNoMode);
    const int org = ((const uint8_t*)SH.r2)[kOrgLeaf + i];
    PROF_MARK(t1_);
    PROF_ADD2(PH_PREDICT, t0_, t1_);
    PROF_ADD2(PH_PRED + 4, t0_, t1_);
    const Pass4Out p = pass4_reg(c, nb, on, v, org, overflow);
    PROF_MARK(t5_);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        o.ssd[b] = (uint32_t)__builtin_amdgcn_readlane(p.row_ssd, 16 * b);
        o.lvl[b] = p.lvl[b];
    }
    o.rec = p.rec;
    WSYNC();
    PROF_MARK(t6_);
    PROF_ADD2(PH_RECON, t5_, t6_); // (the pass's PH_RECON ends at the row sums)
    PROF_ADD2(PH_REC + 3, t5_, t6_);
    return o;
}

// The end of a SINGLE_TREE leaf search (block_splitter.rs:1040-1072): the winner keeps its DM chroma unless the picked
// CCLM mode is strictly cheaper (DM on a tie, :857-873 and :1062); cur / cclm_cost = get_chroma_intra_pred_cost of the two
__device__ __forceinline__ bool dm_keeps(float cur, float cclm_cost) {
    return cur == fminf(cclm_cost, fminf(cur, 3.40282347e+38f));
}
// ... and the final get_intra_pred_cost: the winner's luma (mode ml, class cls) with its own chroma (parts eb) or with
// the CCLM chroma (mode cm, parts e = eb with the CCLM evaluation's chroma parts)
struct ChromaFinal {
    bool dm_wins;
    float cost;
    int mc;
};
__device__ __forceinline__ ChromaFinal chroma_final(const Ctx& c, float cur, float cclm_cost, const EvalParts& eb, const EvalParts& e,
                                                    int cls, int ml, int cm) {
    ChromaFinal f;
    f.dm_wins = dm_keeps(cur, cclm_cost);
    f.cost = f.dm_wins ? uni_f(assemble_cost(c, TREE_SINGLE, cls, ml, eb)) : uni_f(assemble_cost(c, TREE_SINGLE, cls, cm, e));
    f.mc = f.dm_wins ? ml : cm;
    return f;
}

// The running best of a leaf's full candidates: the reference's "first minimum wins" over [planar, DC, cm, cm - 1,
// cm + 1], kept as a strict-less running update in that order.  win = the winner's index in the pack that is being
// merged (-1: none of this pack so far); first = no candidate yet (the first one is taken whatever it costs).
struct LeafBest {
    float cost;
    int mode, cls;
    EvalParts e;
    int win;
    bool first;
};
__device__ __forceinline__ LeafBest leaf_best_init(int mode) {
    LeafBest b;
    b.cost = 3.40282347e+38f;
    b.mode = mode;
    b.cls = 0;
    b.e.ssd_y = b.e.ssd_c = 0;
    b.e.lvl_y = b.e.lvl_c = 0;
    b.win = -1;
    b.first = true;
    return b;
}
// one candidate of a pack that has come back (index k in its pack, luma and chroma mode `mode`, parts e): its cost, the
// trace record, the running first minimum; returns whether it is the new best
__device__ __forceinline__ bool leaf_candidate(const Ctx& c, int bx, int by, int lg, int tree, const MpmList& mpl, LeafBest& b,
                                               int k, int mode, const EvalParts& e) {
    const int cls = mpm_class_of(mpl, mode);
    const float val = uni_f(assemble_cost(c, tree, cls, mode, e));
    if (c.trace && lane_fresh() == 0) TRACE_REC(c.ctu_x + bx, c.ctu_y + by, lg, tree, 1, mode, mode, __float_as_int(val));
    const bool take = b.first || val < b.cost;
    if (take) {
        b.cost = val;
        b.mode = mode;
        b.cls = cls;
        b.e = e;
        b.win = k;
    }
    b.first = false;
    return take;
}

// candidate k of a 4x4 luma pack as parts: no chroma (DUAL_TREE_LUMA)
__device__ __forceinline__ EvalParts pack4_parts(const Pack4Out& p, int k) {
    EvalParts e;
    e.ssd_y = p.ssd[k];
    e.ssd_c = 0;
    e.lvl_y = p.lvl[k];
    e.lvl_c = 0;
    return e;
}

__device__ __forceinline__ Res leaf4_search(const Ctx& c, const Req& q, int* overflow) {
    Res r = res_none();
    const int lane = lane_fresh();
    if (q.refs0) build_refs(c, 0, q.tx, q.ty, 2);
    const int x = lane & 3, y = (lane >> 2) & 3, row = lane >> 4;
    LeafBest best = leaf_best_init(PLANAR);
    const MpmList mpl_ = mpm_list(c, q.tx, q.ty, 2);
    // level schedule (team kernel): member 3's 4x4 luma leaves get their pack A from member 0, the server (serve_pack4;
    // the same protocol as for member 2's 8x8 leaves, leaf8_search)
    constexpr int kSrv4Byte = 448; // in the server's decw: 2 x 16 reconstructed samples, then ssd[2] (u32), lvl[2] (i64)
    const bool served = c.solo && c.member == 3 && lv_word(&SHT.lvb.srv_ready) != 0;
    unsigned my_job = 0;
    if (served) {
        if (lane == 0) {
            SHT.lvb.job4_bx = (uint8_t)q.tx;
            SHT.lvb.job4_by = (uint8_t)q.ty;
        }
        my_job = uni((int)lv_word(&SHT.lvb.job4_posted)) + 1u;
        lv_word_add(&SHT.lvb.job4_posted);
    } else {
        // pack A: planar and DC (:887-898)
        PROF_MARK(l4a0_);
        const Pack4Out a = pack4_eval(c, q, 2, PLANAR, DC, kNoMode, overflow);
        leaf_candidate(c, q.tx, q.ty, 2, TREE_DUAL_LUMA, mpl_, best, 0, PLANAR, pack4_parts(a, 0));
        leaf_candidate(c, q.tx, q.ty, 2, TREE_DUAL_LUMA, mpl_, best, 1, DC, pack4_parts(a, 1));
        if (row == best.win) rec_put(0, q.tx + x, q.ty + y, a.rec);
        WSYNC();
        PROF_MARK(l4a1_);
        PROF_ADD2(PH_L4 + 1, l4a0_, l4a1_);
    }
    // Candidate cut (kCandidateCut): where this wave has pack A's best before the rest of the search starts.  Every
    // angular candidate costs at least the smallest floor an angular mode's class can have under this MPM list: mpm_idx
    // 1 .. 4 and the remainders always (cand_floor_ang), mpm_idx 0 where it is not DC, which pack A has evaluated.  With
    // best <= that floor no later candidate is strictly cheaper: neither the SAD search nor pack B can change the leaf.
    const bool cut_on_ = kCandidateCut && c.solo == 0;
    bool cut_ = false;
    if (cut_on_) {
        float fa = c.k->cand_floor_ang;
        const float f1 = c.k->cand_floor[1];
        if (mpl_.k0 > DC && f1 < fa) fa = f1;
        cut_ = uni((int)(best.cost <= fa)) != 0; // (every lane holds the same scalars: a scalar branch)
        if (cut_) PROF_ADD2(PH_CUT + 6, 0, 1);
    }
    if (!cut_) {
        int cm;
        unsigned smin;
        PROF_MARK(l4s0_);
        sad_search(c, q, cm, smin);
        PROF_MARK(l4s1_);
        PROF_ADD2(PH_L4 + 2, l4s0_, l4s1_);
        cm = uni(cm);
        // pack B: step_search(mode, 1, _, aux = false) on {cm, cm - 1, cm + 1} (:974)
        const int lo = !(cm < 3) ? cm - 1 : kNoMode, hi = !(cm + 1 > 66) ? cm + 1 : kNoMode;
        // the same with the real classes of the three candidates: pack B runs unless every candidate it would evaluate
        // has a floor >= best (a pack of two costs what a pack of three costs, so no part of a pack is cut)
        if (cut_on_) {
            const CONST_AS float* const cf = c.k->cand_floor;
            cut_ = uni((int)(cf[mpm_class_of(mpl_, cm)] >= best.cost && (lo == kNoMode || cf[mpm_class_of(mpl_, lo)] >= best.cost) &&
                             (hi == kNoMode || cf[mpm_class_of(mpl_, hi)] >= best.cost))) != 0;
            if (cut_) PROF_ADD2(PH_CUT + 7, 0, 1);
        }
        if (!cut_) {
            const Pack4Out b = pack4_eval(c, q, 3, cm, lo, hi, overflow);
            best.win = -1;
            leaf_candidate(c, q.tx, q.ty, 2, TREE_DUAL_LUMA, mpl_, best, 0, cm, pack4_parts(b, 0));
            if (lo != kNoMode) leaf_candidate(c, q.tx, q.ty, 2, TREE_DUAL_LUMA, mpl_, best, 1, lo, pack4_parts(b, 1));
            if (hi != kNoMode) leaf_candidate(c, q.tx, q.ty, 2, TREE_DUAL_LUMA, mpl_, best, 2, hi, pack4_parts(b, 2));
            if (row == best.win) rec_put(0, q.tx + x, q.ty + y, b.rec);
            WSYNC();
        }
        PROF_MARK(l4b1_);
        PROF_ADD2(PH_L4 + 3, l4s1_, l4b1_);
    }
    if (served) {
        // [planar, DC] from the server against pack B's first minimum, which wins only if strictly cheaper
        PROF_MARK(sw0_);
        lv_word_wait(&SHT.lvb.job4_done, my_job);
        PROF_MARK(sw1_);
        PROF_ADDM(3, sw0_, sw1_); // (profile build: mem_nop_m3 = what member 3 waits for the server)
        const uint8_t* sv = (const uint8_t*)team_lds(c, 0).decw + kSrv4Byte;
        const LeafBest bestB = best;
        Pack4Out a;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            a.ssd[k2] = (uint32_t)uni((int)((const uint32_t*)(sv + 32))[k2]);
            a.lvl[k2] = uni_i64(((const long long*)(sv + 40))[k2]);
        }
        best.first = true;
        leaf_candidate(c, q.tx, q.ty, 2, TREE_DUAL_LUMA, mpl_, best, 0, PLANAR, pack4_parts(a, 0));
        leaf_candidate(c, q.tx, q.ty, 2, TREE_DUAL_LUMA, mpl_, best, 1, DC, pack4_parts(a, 1));
        if (bestB.cost < best.cost) {
            best = bestB;
        } else {
            if (lane < 16) rec_put(0, q.tx + x, q.ty + y, sv[16 * best.win + lane]);
            WSYNC();
        }
        lv_word_add(&SHT.lvb.job4_ack);
    }
    r.vmin = best.cost;
    r.imin = best.mode;
    return r;
}

// The server's side of a 4x4 leaf (level schedule, q.kind K_SERVE4): reference samples and originals of the block from
// member 3's LDS, pack {planar, DC}, the two candidates' reconstructions and parts to decw[448 ..] of this wave.
__device__ __forceinline__ void serve_pack4(const Ctx& c, const Req& q, int* overflow) {
    const int lane = lane_fresh();
    const Lds& own = team_lds(c, 3);
    for (int w = lane; w < 98; w += 64) ((uint32_t*)SH.refs)[w] = ((const uint32_t*)own.refs)[w];
    if (lane < 4) ((uint32_t*)SH.r2)[kOrgLeaf / 4 + lane] = ((const uint32_t*)own.r2)[kOrgLeaf / 4 + lane];
    WSYNC();
    const Pack4Out a = pack4_eval(c, q, 2, PLANAR, DC, kNoMode, overflow);
    uint8_t* sv = (uint8_t*)SH.decw + 448;
    if (lane < 32) sv[lane] = (uint8_t)a.rec;
    if (lane < 2) {
        ((uint32_t*)(sv + 32))[lane] = lane ? a.ssd[1] : a.ssd[0];
        ((long long*)(sv + 40))[lane] = lane ? a.lvl[1] : a.lvl[0];
    }
    WSYNC();
    lv_word_add(&SHT.lvb.job4_done);
}

// leafc4_search: the DUAL_TREE_CHROMA leaf of a split 8x8 CU (block_splitter.rs:794-885) in one go.  The three CCLM
// SADs and the pick (:847-854) as in K_CCLMSEARCH, then the picked CCLM mode and the DM mode (q.mc) are evaluated SIDE
// BY SIDE: rows 0 / 1 = Cb / Cr of the CCLM candidate, rows 2 / 3 = Cb / Cr of the DM candidate, four 4x4 blocks
// through the stages of pack4_eval.  The winner's rows (DM on a tie, :857-873) write their reconstruction to the tile.
__device__ __forceinline__ Res leafc4_search(const Ctx& c, const Req& q, int* overflow) {
    Res r = res_none();
    const int lane = lane_fresh();
    const int dm = q.mc;
    CclmParams call_;
    const int cm = cclm_probe(c, q.tx, q.ty, 3, q.tree, &call_);
    if (q.refs1) build_refs(c, 1, q.tx, q.ty, 3);
    PROF_MARK(t0_);
    // model parameters of both planes of the picked mode: derived with the SAD list's
    const CclmPick cpk_ = cclm_pick(call_, 2 * cclm_mode_index(cm));
    const int row = lane >> 4, i = lane & 15, x = i & 3, y = i >> 2;
    const int pl = row & 1;
    int v = predict4_lane(c, row >= 2 ? dm : kNoMode, pl); // rows 2, 3: the DM candidate (every lane passes the WSYNC inside)
    if (row < 2) v = cclm_pred4_lane(c, q, cpk_, pl, x, y);
    const int org = ((const uint8_t*)SH.r2)[kOrgLeaf + 256 + 16 * pl + i];
    PROF_MARK(t1_);
    PROF_ADD2(PH_PREDICT, t0_, t1_);
    PROF_ADD2(PH_PRED + 5, t0_, t1_);
    const Pass4Out p = pass4_reg(c, 4, true, v, org, overflow);
    EvalParts ec, ed;
    ec.ssd_y = ed.ssd_y = 0;
    ec.lvl_y = ed.lvl_y = 0;
    ec.ssd_c = (uint32_t)(__builtin_amdgcn_readlane(p.row_ssd, 0) + __builtin_amdgcn_readlane(p.row_ssd, 16));
    ed.ssd_c = (uint32_t)(__builtin_amdgcn_readlane(p.row_ssd, 32) + __builtin_amdgcn_readlane(p.row_ssd, 48));
    ec.lvl_c = p.lvl[0] + p.lvl[1];
    ed.lvl_c = p.lvl[2] + p.lvl[3];
    const float c0 = uni_f(assemble_chroma_cost(c, cm, ec));
    const float dm_cost = uni_f(assemble_chroma_cost(c, dm, ed));
    if (c.trace && lane == 0) {
        TRACE_REC(c.ctu_x + q.tx, c.ctu_y + q.ty, 3, q.tree, 3, 0, cm, __float_as_int(c0));
        TRACE_REC(c.ctu_x + q.tx, c.ctu_y + q.ty, 3, q.tree, 3, 0, dm, __float_as_int(dm_cost));
    }
    // (the leaf's cost is the chroma cost itself: only the tie rule of chroma_final fits here)
    const bool dm_wins = dm_keeps(dm_cost, c0);
    if ((row >= 2) == dm_wins) rec_put(1 + pl, (q.tx >> 1) + x, (q.ty >> 1) + y, p.rec);
    WSYNC();
    r.vmin = dm_wins ? dm_cost : c0;
    r.imin = dm_wins ? dm : cm;
    return r;
}

// ---------------------------------------------------------------------------
// K_LEAF8: the whole search of an 8x8 SINGLE_TREE leaf in one request (block_splitter.rs:886-1078 with a luma 8x8 block
// and a Cb + Cr 4x4 pair per candidate).  At max-split-depth 2 these leaves are two thirds of a CTU's evaluations and
// each one was a chain of short stages between control steps: 64 + 32 samples per candidate, a pooled 64-step trellis
// walk per candidate between two workgroup barriers.  The full candidates of a leaf read only neighbours outside the
// block (:887-898, :974), so they are evaluated in PACKS: pack A = {planar, DC}, then the SAD search, then pack B =
// {cm, cm - 1, cm + 1}; a pack's candidates go through every stage together -- luma blocks one pass each, the 4x4
// chroma blocks of all candidates four to a pass (predict4_lane, transformed in registers), the luma
// transforms over nb blocks, and ONE trellis pass
// for the pack's six or nine chains walked side by side by this wave alone (quantize_pk: no workgroup barrier).
// Predictions and reconstructions of the pack are parked in LDS (PRED_PARK); the running best candidate's
// reconstruction goes to the tile when its pack is done, so there is no save / restore through global scratch.
// Then the CCLM part (:1040-1072) as in K_CCLMSEARCH, the CCLM candidate's prediction and reconstruction in
// registers: the tile keeps the DM chroma unless CCLM wins.  The decisions are the reference's, in its order: first
// minimum of [planar, DC, cm, cm - 1, cm + 1] as a running strict-less update; DM on a tie with CCLM.
// ---------------------------------------------------------------------------
struct Pack8Out {
    uint32_t ssd_y[3], ssd_c[3];
    long long lvl_y[3], lvl_c[3];
};
// candidate k of an 8x8 or 16x16 pack (Pack8Out, Pack16Out) as parts
template <class P>
__device__ __forceinline__ EvalParts pack_parts(const P& p, int k) {
    EvalParts e;
    e.ssd_y = p.ssd_y[k];
    e.ssd_c = p.ssd_c[k];
    e.lvl_y = p.lvl_y[k];
    e.lvl_c = p.lvl_c[k];
    return e;
}
__device__ __forceinline__ Pack8Out pack8_eval(const Ctx& c, const Req& q, int nc, int m0, int m1, int m2, int* overflow) {
    Pack8Out o;
    const int lane = lane_fresh();
    const int row = lane >> 4, i16 = lane & 15;
    const int nL = 64 * nc;
    uint8_t* park = (uint8_t*)SH.decw + kParkByte;
    const uint8_t* org = (const uint8_t*)SH.r2 + kOrgLeaf;
    PROF_MARK(t0_);
    predict_pack8_luma(c, nc, m0, m1, m2); // luma: the candidates side by side, one pass
    PROF_MARK(tl_);
    // chroma: the 4x4 blocks of all candidates, four to a pass (row = block 2 cand + plane)
#pragma unroll 1
    for (int ps = 0; ps < 2; ++ps) {
        if (4 * ps >= 2 * nc) continue;
        const int blk = 4 * ps + row;
        const int cd = blk >> 1, pl = blk & 1;
        const int mode = cd == 0 ? m0 : (cd == 1 ? m1 : m2);
        const bool in = blk < 2 * nc;
        const bool on = in && mode != kNoMode;
        const int v = predict4_lane(c, on ? mode : kNoMode, pl);
        int rc = on ? (int)org[256 + 16 * pl + i16] - v : 0;
        // the block's coefficients straight from the registers, to where quantize_pk takes them (every lane runs the
        // transform; a row without a block carries zeros and stores nothing)
        rc = fwd_dct4_reg(rc);
        if (in) {
            SH.r1[nL + 16 * blk + i16] = (int16_t)rc;
            park[nL + 16 * blk + i16] = (uint8_t)v;
        }
        WSYNC();
    }
    PROF_MARK(t1_);
    PROF_ADD2(PH_PREDICT, t0_, t1_);
    PROF_ADD2(PH_PRED + 3, t0_, tl_);
    PROF_ADD2(PH_PRED + 4, tl_, t1_);
    fwd_dct_lg(c, 3, nc, 0);
    PROF_MARK(t2_);
    PROF_ADD2(PH_FDCT, t1_, t2_);
    bool any_y = false, any_c = false;
    quantize_pk<3>(c, nc, overflow, o.lvl_y, o.lvl_c, &any_y, &any_c);
    PROF_MARK(t3_);
    if (any_y) { // (all levels zero: the residuals are zero too, and r1 already says so)
        dequantize_t(c, 3, nc, 0);
        inv_dct_lg(c, 3, nc, 0);
    }
    PROF_MARK(t4_);
    PROF_ADD2(PH_IDCT, t3_, t4_);
    // reconstruction (pred as i16 + res, clamp: :178) and SSD; the reconstruction takes the prediction's place
#pragma unroll
    for (int cd = 0; cd < 3; ++cd) {
        o.ssd_y[cd] = 0;
        o.ssd_c[cd] = 0;
        if (cd < nc) {
            int rec = (int16_t)((int)park[64 * cd + lane] + (int)SH.r1[64 * cd + lane]);
            rec = min(max(rec, 0), 255);
            park[64 * cd + lane] = (uint8_t)rec;
            const int d = rec - (int)org[lane];
            o.ssd_y[cd] = (uint32_t)wave_sum_i32(M24(d, d));
        }
    }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        if (4 * ps >= 2 * nc) continue;
        const int blk = 4 * ps + row;
        const bool in = blk < 2 * nc;
        int dd = 0;
        // r1 holds the block's levels: the lane dequantises and inverts its own in registers
        const int res = residual4_reg(c, in ? (int)SH.r1[nL + 16 * blk + i16] : 0, any_c);
        if (in) {
            int rec = (int16_t)((int)park[nL + 16 * blk + i16] + res);
            rec = min(max(rec, 0), 255);
            park[nL + 16 * blk + i16] = (uint8_t)rec;
            const int d = rec - (int)org[256 + 16 * (blk & 1) + i16];
            dd = M24(d, d);
        }
        const int rs = row_sum_i32(dd);
        const uint32_t s01 = (uint32_t)(__builtin_amdgcn_readlane(rs, 0) + __builtin_amdgcn_readlane(rs, 16));
        const uint32_t s23 = (uint32_t)(__builtin_amdgcn_readlane(rs, 32) + __builtin_amdgcn_readlane(rs, 48));
        if (ps == 0) {
            o.ssd_c[0] = s01;
            o.ssd_c[1] = s23;
        } else {
            o.ssd_c[2] = s01;
        }
    }
    WSYNC();
    PROF_MARK(t5_);
    PROF_ADD2(PH_RECON, t4_, t5_);
    PROF_ADD2(PH_REC + 2, t4_, t5_);
    return o;
}

// candidate cd's reconstruction from the park of a pack of nc (this wave's or the server's) into the tile (luma 8x8, Cb
// and Cr 4x4)
__device__ __forceinline__ void pack8_to_tile(const Req& q, const uint8_t* park, int nc, int cd) {
    const int lane = lane_fresh();
    rec_put(0, q.tx + (lane & 7), q.ty + (lane >> 3), park[64 * cd + lane]);
    if (lane < 32) {
        const int pl = lane >> 4, i = lane & 15;
        rec_put(1 + pl, (q.tx >> 1) + (i & 3), (q.ty >> 1) + (i >> 2), park[64 * nc + 32 * cd + lane]);
    }
    WSYNC();
}

__device__ __forceinline__ Res leaf8_search(const Ctx& c, const Req& q, int* overflow) {
    Res r = res_none();
    const int lane = lane_fresh();
    if (q.refs0) build_refs(c, 0, q.tx, q.ty, 3);
    if (q.refs1) build_refs(c, 1, q.tx, q.ty, 3);
    LeafBest best = leaf_best_init(q.ml);
    const MpmList mpl_ = mpm_list(c, q.tx, q.ty, 3);
    // Level schedule (team kernel): member 0, idle once the CTU's 32x32 candidate is done, SERVES pack A of member 2's 8x8
    // leaves (serve_pack8).  Member 2 of a team in the level schedule, and the server is polling: post the job (the
    // block's reference samples and originals are ready and stay untouched until the leaf is decided), skip pack A
    // here, merge its results below
    const bool served = c.solo && c.member == 2 && lv_word(&SHT.lvb.srv_ready) != 0;
    unsigned my_job = 0;
    if (served) {
        if (lane == 0) {
            SHT.lvb.job_bx = (uint8_t)q.tx;
            SHT.lvb.job_by = (uint8_t)q.ty;
        }
        my_job = uni((int)lv_word(&SHT.lvb.job_posted)) + 1u;
        lv_word_add(&SHT.lvb.job_posted);
    } else {
        // pack A: planar and DC (:887-898)
        PROF_MARK(la0_);
        const Pack8Out a = pack8_eval(c, q, 2, PLANAR, DC, kNoMode, overflow);
        leaf_candidate(c, q.tx, q.ty, 3, TREE_SINGLE, mpl_, best, 0, PLANAR, pack_parts(a, 0));
        leaf_candidate(c, q.tx, q.ty, 3, TREE_SINGLE, mpl_, best, 1, DC, pack_parts(a, 1));
        pack8_to_tile(q, (const uint8_t*)SH.decw + kParkByte, 2, best.win);
        PROF_MARK(la1_);
        PROF_ADD2(PH_LEAF + 0, la0_, la1_);
    }
    {
        int cm;
        unsigned smin;
        PROF_MARK(ls0_);
        sad_search(c, q, cm, smin);
        PROF_MARK(ls1_);
        PROF_ADD2(PH_LEAF + 1, ls0_, ls1_);
        cm = uni(cm);
        // pack B: step_search(mode, 1, _, aux = false) on {cm, cm - 1, cm + 1} (:974)
        const int lo = !(cm < 3) ? cm - 1 : kNoMode, hi = !(cm + 1 > 66) ? cm + 1 : kNoMode;
        const Pack8Out b = pack8_eval(c, q, 3, cm, lo, hi, overflow);
        best.win = -1;
        leaf_candidate(c, q.tx, q.ty, 3, TREE_SINGLE, mpl_, best, 0, cm, pack_parts(b, 0));
        if (lo != kNoMode) leaf_candidate(c, q.tx, q.ty, 3, TREE_SINGLE, mpl_, best, 1, lo, pack_parts(b, 1));
        if (hi != kNoMode) leaf_candidate(c, q.tx, q.ty, 3, TREE_SINGLE, mpl_, best, 2, hi, pack_parts(b, 2));
        if (best.win >= 0) pack8_to_tile(q, (const uint8_t*)SH.decw + kParkByte, 3, best.win);
        PROF_MARK(lb1_);
        PROF_ADD2(PH_LEAF + 2, ls1_, lb1_);
    }
    if (served) {
        // the server's pack A: first minimum of [planar, DC] against the first minimum of pack B found above; the
        // reference's order is [planar, DC, cm, cm - 1, cm + 1], so pack B's best wins only if strictly cheaper
        PROF_MARK(sw0_);
        lv_word_wait(&SHT.lvb.job_done, my_job);
        PROF_MARK(sw1_);
        PROF_ADDM(3, sw0_, sw1_); // (mem_nop_m2)
        const Lds& srv = team_lds(c, 0);
        const LeafBest bestB = best;
        best.first = true;
        Pack8Out a;
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
            const XRes& x = srv.xr[k2];
            a.ssd_y[k2] = (uint32_t)uni((int)x.ssd_y);
            a.ssd_c[k2] = (uint32_t)uni((int)x.ssd_c);
            a.lvl_y[k2] = uni_i64(x.lvl_y);
            a.lvl_c[k2] = uni_i64(x.lvl_c);
        }
        leaf_candidate(c, q.tx, q.ty, 3, TREE_SINGLE, mpl_, best, 0, PLANAR, pack_parts(a, 0));
        leaf_candidate(c, q.tx, q.ty, 3, TREE_SINGLE, mpl_, best, 1, DC, pack_parts(a, 1));
        if (bestB.cost < best.cost) // pack B's best stays (its reconstruction is in the tile already)
            best = bestB;
        else                        // a candidate of pack A: its reconstruction from the server's park
            pack8_to_tile(q, (const uint8_t*)srv.decw + kParkByte, 2, best.win);
        lv_word_add(&SHT.lvb.job_ack);
    }
    const int best_mode = best.mode;
    const EvalParts eb = best.e;
    r.imin = best_mode;
    r.ssd_y = eb.ssd_y;
    r.ssd_c = eb.ssd_c;
    r.lvl_y = eb.lvl_y;
    r.lvl_c = eb.lvl_c;
    // ---- the CCLM part on the winner, whose reconstruction is in the tile (:1040-1072) ----
    // :1040 get_chroma_intra_pred_cost(mode) repeats the winner's chroma evaluation: its parts are at hand
    const float cur = uni_f(assemble_chroma_cost(c, best_mode, eb));
    if (c.trace && lane == 0)
        TRACE_REC(c.ctu_x + q.tx, c.ctu_y + q.ty, 3, TREE_SINGLE, 3, 0, best_mode, __float_as_int(cur));
    PROF_MARK(lc0_);
    CclmParams call_;
    const int cm = cclm_probe(c, q.tx, q.ty, 3, TREE_SINGLE, &call_);
    PROF_MARK(t0_);
    PROF_ADD2(PH_LEAF + 11, lc0_, t0_);
    const CclmPick cpk_ = cclm_pick(call_, 2 * cclm_mode_index(cm)); // (derived with the SAD list's)
    const int row = lane >> 4, i = lane & 15, x = i & 3, y = i >> 2;
    const int pl = row & 1;
    const bool mine = row < 2; // rows 0 / 1 = Cb / Cr; rows 2, 3 ride along as zero blocks
    int v = 128;
    if (mine) v = cclm_pred4_lane(c, q, cpk_, pl, x, y);
    const int org = ((const uint8_t*)SH.r2)[kOrgLeaf + 256 + 16 * pl + i];
    PROF_MARK(t1_);
    PROF_ADD2(PH_PREDICT, t0_, t1_);
    PROF_ADD2(PH_PRED + 5, t0_, t1_);
    const Pass4Out p = pass4_reg(c, 2, mine, v, org, overflow);
    EvalParts e = eb;
    e.ssd_c = (uint32_t)(__builtin_amdgcn_readlane(p.row_ssd, 0) + __builtin_amdgcn_readlane(p.row_ssd, 16));
    e.lvl_c = p.lvl[0] + p.lvl[1];
    const float cclm_cost = uni_f(assemble_chroma_cost(c, cm, e));
    if (c.trace && lane == 0) TRACE_REC(c.ctu_x + q.tx, c.ctu_y + q.ty, 3, TREE_SINGLE, 3, 0, cm, __float_as_int(cclm_cost));
    // :1062-1072 final get_intra_pred_cost: the winner's luma with the DM chroma (still in the tile) or the CCLM chroma
    const ChromaFinal f = chroma_final(c, cur, cclm_cost, eb, e, best.cls, best_mode, cm);
    if (!f.dm_wins && mine) rec_put(1 + pl, (q.tx >> 1) + x, (q.ty >> 1) + y, p.rec);
    WSYNC();
    PROF_MARK(lc9_);
    PROF_ADD2(PH_LEAF + 3, lc0_, lc9_);
    r.vmin = f.cost;
    r.imin2 = f.mc;
    return r;
}

// The server's side of an 8x8 leaf (level schedule, q.kind K_SERVE8): reference samples and originals of the block from
// member 2's LDS, pack {planar, DC}, the candidates' parts to xr[0 .. 1], their reconstructions stay in this wave's park.
__device__ __forceinline__ void serve_pack8(const Ctx& c, const Req& q, int* overflow) {
    const int lane = lane_fresh();
    const Lds& own = team_lds(c, 2);
    for (int w = lane; w < 98; w += 64) ((uint32_t*)SH.refs)[w] = ((const uint32_t*)own.refs)[w];
    for (int w = lane; w < 96; w += 64) ((uint32_t*)SH.r2)[kOrgLeaf / 4 + w] = ((const uint32_t*)own.r2)[kOrgLeaf / 4 + w];
    WSYNC();
    const Pack8Out a = pack8_eval(c, q, 2, PLANAR, DC, kNoMode, overflow);
    if (lane < 2) {
        XRes x;
        x.ssd_y = lane ? a.ssd_y[1] : a.ssd_y[0];
        x.ssd_c = lane ? a.ssd_c[1] : a.ssd_c[0];
        x.lvl_y = lane ? a.lvl_y[1] : a.lvl_y[0];
        x.lvl_c = lane ? a.lvl_c[1] : a.lvl_c[0];
        SH.xr[lane] = x;
    }
    WSYNC();
    lv_word_add(&SHT.lvb.job_done);
}

// ---------------------------------------------------------------------------
// K_LEAF16: the full candidates of a 16x16 SINGLE_TREE leaf in one request (block_splitter.rs:886-1037), in packs of
// TWO: {planar, DC}, the SAD search, {cm, cm - 1}, {cm + 1}.  Two candidates' residuals (2 x (256 + 2 x 64) i16) are
// what r1 holds; a pack goes through prediction, transforms and reconstruction block after block as the single
// evaluation does, and through ONE trellis pass for its six chains (quantize_pk<4>: the two luma chains side by side,
// the four chroma chains riding along, this wave alone, no workgroup barrier) -- three walks of 256 steps per leaf
// instead of five pooled ones, and one control step instead of six.  The two candidates' predictions (768 B) are parked in
// the three corners of LDS the pack leaves free (PRED_PARK16, dev_predict.h); the running best candidate's reconstruction
// goes from there to the tile when its pack is done.  The CCLM part follows as its own request (leaf_step, C_WINNER): its DM-chroma
// restore takes the winner from slot 0, where the request after this one saves it.
// ---------------------------------------------------------------------------
struct Pack16Out {
    uint32_t ssd_y[2], ssd_c[2];
    long long lvl_y[3], lvl_c[3];
};
// predictions and residuals of the pack's nc candidates, luma block and chroma pair: prediction bytes to park16,
// residuals to r1 in the same layout (luma [cand][256], then chroma [cand][Cb | Cr][64])
__device__ __forceinline__ void pack16_predict(const Ctx& c, int tx, int ty, int nc, int m0, int m1) {
    const int lane = lane_fresh();
    const int nL = 256 * nc;
#pragma unroll 1
    for (int cd = 0; cd < nc; ++cd) {
        const int mode = cd == 0 ? m0 : m1;
        if (mode != kNoMode) {
            predict_full<0>(c, tx, ty, 4, mode, 256 * cd, PRED_PARK16, nL);
            predict_full<1>(c, tx, ty, 4, mode, nL + 128 * cd, PRED_PARK16, nL);
        } else { // a candidate outside 2..66 rides along as a zero block
            for (int i = lane; i < 256; i += 64) {
                SH.r1[256 * cd + i] = 0;
                *park16(256 * cd + i, nL) = 0;
            }
            for (int i = lane; i < 128; i += 64) {
                SH.r1[nL + 128 * cd + i] = 0;
                *park16(nL + 128 * cd + i, nL) = 0;
            }
            WSYNC();
        }
    }
}
__device__ __forceinline__ Pack16Out pack16_eval(const Ctx& c, const Req& q, int nc, int m0, int m1, int* overflow) {
    Pack16Out o;
    const int lane = lane_fresh();
    const int nL = 256 * nc;
    const uint8_t* org = (const uint8_t*)SH.r2 + kOrgLeaf; // luma 256 | Cb 64 | Cr 64
    PROF_MARK(t0_);
    pack16_predict(c, q.tx, q.ty, nc, m0, m1);
    PROF_MARK(t1_);
    PROF_ADD2(PH_PREDICT, t0_, t1_);
    PROF_ADD2(PH_PRED + 2, t0_, t1_);
    fwd_dct_lg(c, 4, nc, 0);
    fwd_dct_lg(c, 3, 2 * nc, nL);
    PROF_MARK(t2_);
    PROF_ADD2(PH_FDCT, t1_, t2_);
    bool any_y = false, any_c = false;
    quantize_pk<4>(c, nc, overflow, o.lvl_y, o.lvl_c, &any_y, &any_c);
    PROF_MARK(t3_);
    if (any_y) {
        dequantize_t(c, 4, nc, 0);
        inv_dct_lg(c, 4, nc, 0);
    }
    if (any_c) {
        dequantize_t(c, 3, 2 * nc, nL);
        inv_dct_lg(c, 3, 2 * nc, nL);
    }
    PROF_MARK(t4_);
    PROF_ADD2(PH_IDCT, t3_, t4_);
#pragma unroll
    for (int cd = 0; cd < 2; ++cd) {
        o.ssd_y[cd] = 0;
        o.ssd_c[cd] = 0;
        if (cd < nc) {
            // a row of four samples per lane (recon_row4): the luma block is one pass of the wave, the chroma pair half of one
            unsigned py = 0, pc = 0;
            int v[4];
            {
                const int i = 4 * lane;
                uint32_t* pk = (uint32_t*)park16(256 * cd + i, nL);
                *pk = recon_row4(*pk, *(const uint2*)&SH.r1[256 * cd + i], *(const uint32_t*)(org + i), v, py);
            }
            if (lane < 32) {
                const int i = 4 * lane;
                uint32_t* pk = (uint32_t*)park16(nL + 128 * cd + i, nL);
                *pk = recon_row4(*pk, *(const uint2*)&SH.r1[nL + 128 * cd + i], *(const uint32_t*)(org + 256 + i), v, pc);
            }
            o.ssd_y[cd] = (uint32_t)wave_sum_i32((int)py);
            o.ssd_c[cd] = (uint32_t)wave_sum_i32((int)pc);
        }
    }
    WSYNC();
    PROF_MARK(t5_);
    PROF_ADD2(PH_RECON, t4_, t5_);
    PROF_ADD2(PH_REC + 1, t4_, t5_);
    return o;
}

// a pack candidate's reconstruction from its park (park16) into the tile (luma 16x16, Cb and Cr 8x8)
__device__ __forceinline__ void pack16_to_tile(const Ctx& c, const Req& q, int nc, int cd) {
    const int lane = lane_fresh();
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
        const int i = lane + 64 * kq;
        rec_put(0, q.tx + (i & 15), q.ty + (i >> 4), *park16(256 * cd + i, 256 * nc));
    }
#pragma unroll
    for (int kq = 0; kq < 2; ++kq) {
        const int i = lane + 64 * kq;
        rec_put(1 + (i >> 6), (q.tx >> 1) + (i & 7), (q.ty >> 1) + ((i & 63) >> 3), *park16(256 * nc + 128 * cd + i, 256 * nc));
    }
    WSYNC();
}

__device__ __forceinline__ Res leaf16_search(const Ctx& c, const Req& q, int* overflow) {
    Res r = res_none();
    const int lane = lane_fresh();
    if (q.refs0) build_refs(c, 0, q.tx, q.ty, 4);
    if (q.refs1) build_refs(c, 1, q.tx, q.ty, 4);
    LeafBest best = leaf_best_init(PLANAR);
    const MpmList mpl_ = mpm_list(c, q.tx, q.ty, 4);
    {
        // planar and DC (:887-898)
        PROF_MARK(la0_);
        const Pack16Out a = pack16_eval(c, q, 2, PLANAR, DC, overflow);
        leaf_candidate(c, q.tx, q.ty, 4, TREE_SINGLE, mpl_, best, 0, PLANAR, pack_parts(a, 0));
        leaf_candidate(c, q.tx, q.ty, 4, TREE_SINGLE, mpl_, best, 1, DC, pack_parts(a, 1));
        pack16_to_tile(c, q, 2, best.win);
        PROF_MARK(la1_);
        PROF_ADD2(PH_LEAF + 4, la0_, la1_);
    }
    int cm;
    unsigned smin;
    PROF_MARK(ls0_);
    sad_search(c, q, cm, smin);
    PROF_MARK(ls1_);
    PROF_ADD2(PH_LEAF + 5, ls0_, ls1_);
    cm = uni(cm);
    // step_search(mode, 1, _, aux = false) on {cm, cm - 1, cm + 1} (:974): {cm, cm - 1}, then cm + 1
    const int lo = !(cm < 3) ? cm - 1 : kNoMode, hi = !(cm + 1 > 66) ? cm + 1 : kNoMode;
    {
        const Pack16Out b = pack16_eval(c, q, 2, cm, lo, overflow);
        best.win = -1;
        leaf_candidate(c, q.tx, q.ty, 4, TREE_SINGLE, mpl_, best, 0, cm, pack_parts(b, 0));
        if (lo != kNoMode) leaf_candidate(c, q.tx, q.ty, 4, TREE_SINGLE, mpl_, best, 1, lo, pack_parts(b, 1));
        if (best.win >= 0) pack16_to_tile(c, q, 2, best.win);
    }
    PROF_MARK(lb1_);
    PROF_ADD2(PH_LEAF + 6, ls1_, lb1_);
    if (hi != kNoMode) {
        const Pack16Out b = pack16_eval(c, q, 1, hi, kNoMode, overflow);
        best.win = -1;
        leaf_candidate(c, q.tx, q.ty, 4, TREE_SINGLE, mpl_, best, 0, hi, pack_parts(b, 0));
        if (best.win >= 0) pack16_to_tile(c, q, 1, best.win);
    }
    PROF_MARK(lc1_);
    PROF_ADD2(PH_LEAF + 7, lb1_, lc1_);
    r.vmin = best.cost;
    r.imin = best.mode;
    r.imin2 = best.mode;
    r.ssd_y = best.e.ssd_y;
    r.ssd_c = best.e.ssd_c;
    r.lvl_y = best.e.lvl_y;
    r.lvl_c = best.e.lvl_c;
    return r;
}

// ---------------------------------------------------------------------------
// full_search: the full evaluations that go through r1 / r2 one component at a time -- a 32x32 candidate, a chroma pair
// alone, a final-pass block -- as STEPS of one loop around one copy of the stages (full_front, quantize_solo, full_back).
//   K_FULL:       one step, the request's candidate.
//   K_CCLMSEARCH: one step: the three CCLM probes and the pick (cclm_probe), then the chroma pair under the picked mode.
//   K_LEAF32 (wave kernels): the whole search of the CTU's 32x32 SINGLE_TREE leaf (block_splitter.rs:794-1078) in one
//       request, six steps: planar, DC, [the SAD search: sad_search] cm, cm - 1, cm + 1, [the winner's luma back, the
//       probes and the pick] the chroma pair under the picked CCLM mode.  The decisions are the reference's in its order:
//       the first minimum of [planar, DC, cm, cm - 1, cm + 1] as a running strict-less update, a neighbour outside 2..66
//       not evaluated (f32::MAX there: never a new minimum), DM chroma unless the CCLM candidate is strictly cheaper
//       (dm_keeps).  Made once per leaf: both reference builds (step 0), the MPM list, the staged originals of the SAD
//       lists; the chroma pair is staged again in front of the probes because the three candidates in between run
//       their transforms through r2, where the staged originals live.  The running best -- cost, mode, class, parts --
//       stays in scalars across the steps.  A new best goes to slot q.copy_slot straight after its evaluation (the
//       unsplit slot 1 + level when the node's split is searched next, ctu_step), luma and DM chroma; the winner's luma
//       comes back from there unless the tile still holds it, and its DM chroma when DM wins.  Until round 20 every step
//       was a request of its own with a control step of leaf_step in between, every save or restore rode on the next
//       request or on an empty one, and the SAD search and the CCLM part were two more kinds of request.
// Res of K_LEAF32: vmin = the leaf's cost, imin / imin2 = its luma / chroma mode.
// L32: the instantiation that serves K_LEAF32 and nothing else -- six steps, the block's place and size known when it is
// built (the CTU's 32x32 block: tx = ty = 0, log2 size 5); the other one serves K_FULL / K_CCLMSEARCH in one step and
// compiles to what evaluate()'s branch was.  One instantiation for all three behind a run-time step count cost the
// wave kernels 165 more spilled scalars and 1.5 % of the headline.
// (A round per component, the stages in loops over the round's components: the shape is kept for the register
// allocator's sake -- one flat loop cost the wave kernels 6 KB of reloaded scalars and 1 % of their speed)
// ---------------------------------------------------------------------------
template <bool TEAM, bool L32>
__device__ __forceinline__ Res full_search(const Ctx& c, const PicBufs& pb, const Req& q, int* overflow) {
    Res r = res_none();
    constexpr bool l32 = !TEAM && L32;
    // (the CTU's 32x32 block: its place and size are known when the code is built)
    const int tx = l32 ? 0 : q.tx, ty = l32 ? 0 : q.ty, tlg = l32 ? 5 : q.tlg;
    Req qe = {}; // the step's candidate (only what the stages and sad_search read)
    qe.tx = tx;
    qe.ty = ty;
    qe.tlg = tlg;
    qe.tree = q.tree;
    qe.final = q.final;
    qe.comps = q.comps;
    qe.ml = q.ml;
    qe.active = q.active;
    qe.refs0 = q.refs0;
    qe.refs1 = q.refs1;
    int mc = q.mc;
    CclmPick cpick_ = CclmPick{};
    // K_LEAF32: the running best, the directional mode of the SAD search, "the tile holds the best candidate", the
    // winner's DM chroma cost (:1040)
    LeafBest best = leaf_best_init(PLANAR);
    MpmList mpl_ = {};
    int cm = 0;
    bool tile_best = false;
    float dm_cost = 0.0f;
    if (l32) mpl_ = mpm_list(c, tx, ty, tlg);
    constexpr int steps = l32 ? 6 : 1;
#pragma unroll 1
    for (int k = 0; k < steps; ++k) {
        PROF_MARK(lk0_);
        bool probe = !l32 && q.kind == K_CCLMSEARCH;
        if (l32 && (k == 3 ? cm < 3 : (k == 4 && cm + 1 > 66))) continue;
        if (l32) {
            if (k == 2) {
                // the 13 directional candidates, their first minimum and both step-search rounds (:899-973)
                PROF_MARK(ls0_);
                stage_org(c, 3, tx, ty, tlg);
                unsigned smin;
                sad_search(c, qe, cm, smin);
                cm = uni(cm);
                PROF_MARK(ls1_);
                PROF_ADD2(PH_LEAF + 14, ls0_, ls1_);
            }
            // step_search(mode, 1, _, aux = false) on {cm, cm - 1, cm + 1} (:974)
            const int mode = k == 0 ? PLANAR : (k == 1 ? DC : (k == 2 ? cm : (k == 3 ? cm - 1 : cm + 1)));
            qe.ml = mode;
            mc = mode;
            qe.refs0 = qe.refs1 = k == 0;
            if (k == 5) {
                // the winner is decided (:975-978); :989-1037 re-runs its luma to have it in the tile: here it comes back
                // from the slot; :1040 repeats its chroma evaluation: the parts are re-used
                if (!tile_best) copy_block(c, COPY_RESTORE, 1, q.copy_slot, tx, ty, tlg);
                dm_cost = uni_f(assemble_chroma_cost(c, best.mode, best.e));
                if (c.trace && LANE == 0)
                    TRACE_REC(c.ctu_x + tx, c.ctu_y + ty, tlg, TREE_SINGLE, 3, 0, best.mode, __float_as_int(dm_cost));
                qe.comps = 2;
                qe.ml = 0;
                probe = true;
            }
        }
        PROF_MARK(lkc_);
        if (probe) {
            // the three CCLM probes and the pick (cclm_probe); the evaluation follows below
            if (tlg > 4) stage_org(c, 2, tx, ty, tlg);
            CclmParams call_;
            mc = cclm_probe(c, tx, ty, tlg, q.tree, &call_);
            r.imin = mc;
            cpick_ = cclm_pick(call_, 2 * cclm_mode_index(mc)); // the evaluation below predicts with these
        }
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {
            const int cset = qe.comps & (1 << round);
            if (!cset) continue;
            if (qe.active) {
#pragma unroll 1
                for (int comp = 0; comp < 2; ++comp)
                    if ((cset >> comp) & 1) {
                        PROF_MARK(tf0_);
                        full_front(c, qe, comp, comp ? mc : qe.ml, 0, cpick_);
                        PROF_MARK(tf1_);
                        PROF_ADD2(PH_PSZ + ((tlg - 2) * 2 + comp), tf0_, tf1_);
                        PROF_ADD2(PH_PCNT + ((tlg - 2) * 2 + comp), 0, 1);
                    }
            }
            PROF_MARK(ts0_);
            bool any_y = false, any_c = false;
            {
                bool any = false;
                long long lvl = 0;
                if (qe.active)
                    lvl = quantize_solo(c, tlg - round, round ? 2 : 1, overflow, &any);
                if (round) {
                    r.lvl_c = lvl;
                    any_c = any;
                } else {
                    r.lvl_y = lvl;
                    any_y = any;
                }
            }
            PROF_MARK(ts1_);
            PROF_ADD2(PH_QZ + ((tlg - 2) & 3), ts0_, ts1_);
            if (!qe.active) {
                PROF_ADD2(PH_SKIP, ts0_, ts1_);
                continue;
            }
#pragma unroll 1
            for (int comp = 0; comp < 2; ++comp) {
                if (!((cset >> comp) & 1)) continue;
                PROF_MARK(tb0_);
                const uint32_t ssd = full_back(c, pb, qe, comp, 0, comp ? any_c : any_y);
                PROF_MARK(tb1_);
                PROF_ADD2(PH_PSZ + ((tlg - 2) * 2 + comp), tb0_, tb1_);
                if (comp)
                    r.ssd_c = ssd;
                else
                    r.ssd_y = ssd;
            }
        }
        if (!l32) continue;
        EvalParts e;
        e.ssd_y = r.ssd_y;
        e.ssd_c = r.ssd_c;
        e.lvl_y = r.lvl_y;
        e.lvl_c = r.lvl_c;
        if (k < 5) {
            // a full candidate: its cost, its trace record, the running first minimum; a new best is saved at once, any
            // other candidate has overwritten the tile
            tile_best = leaf_candidate(c, tx, ty, tlg, TREE_SINGLE, mpl_, best, k, qe.ml, e);
            if (tile_best) copy_block(c, COPY_SAVE, 3, q.copy_slot, tx, ty, tlg);
            PROF_MARK(lk1_);
            PROF_ADD2(PH_LEAF + 13, lkc_, lk1_);
            continue;
        }
        // the CCLM candidate = the winner's luma parts + the chroma parts just evaluated; :1062-1072 the final
        // get_intra_pred_cost with the winner's class from its candidate evaluation.  DM wins: its chroma pair comes back
        const int cclm = mc;
        e.ssd_y = best.e.ssd_y;
        e.lvl_y = best.e.lvl_y;
        const float cclm_cost = uni_f(assemble_chroma_cost(c, cclm, e));
        if (c.trace && LANE == 0)
            TRACE_REC(c.ctu_x + tx, c.ctu_y + ty, tlg, TREE_SINGLE, 3, 0, cclm, __float_as_int(cclm_cost));
        r.imin = best.mode;
        if (dm_keeps(dm_cost, cclm_cost)) {
            r.vmin = uni_f(assemble_cost(c, TREE_SINGLE, best.cls, best.mode, best.e));
            r.imin2 = best.mode;
            copy_block(c, COPY_RESTORE, 2, q.copy_slot, tx, ty, tlg);
        } else {
            r.vmin = uni_f(assemble_cost(c, TREE_SINGLE, best.cls, cclm, e));
            r.imin2 = cclm;
        }
        PROF_MARK(lk2_);
        PROF_ADD2(PH_LEAF + 15, lk0_, lk2_);
    }
    return r;
}

// the decision maps of a block: at most 8 x 8 units of 4x4 (one lane each), sizes are powers of two
__device__ __forceinline__ void fill_maps(int bx, int by, int lg, int luma_mode, int chroma_mode, bool luma,
                                          bool chroma) {
    const int l4 = lg - 2; // log2 of the block's side in 4x4 units
    if (luma && LANE < (1 << (2 * l4))) {
        const int idx = ((by >> 2) + (LANE >> l4)) * 8 + (bx >> 2) + (LANE & ((1 << l4) - 1));
        SH.cu_log2[idx] = (uint8_t)lg;
        SH.luma_mode[idx] = (uint8_t)luma_mode;
    }
    if (chroma) {
        const int l8 = max(l4 - 1, 0);
        if (LANE < (1 << (2 * l8)))
            SH.chroma_mode[((by >> 3) + (LANE >> l8)) * 4 + (bx >> 3) + (LANE & ((1 << l8) - 1))] = (uint8_t)chroma_mode;
    }
    WSYNC();
}


// Split cut, the check before a child is searched: the partial cost of the children searched so far, then the floor
// of every child still to come (DevConst::split_floor: `n` children of floor index `fi`, then the chroma leaf's if
// `chroma`) added one by one in z-order, exactly where the full sum adds that child's cost.  Each floor is <= the cost
// it stands for and f32 addition is monotone in either operand, so the full sum is >= this bound whatever the
// children hold: a bound strictly greater than the unsplit cost means the split has lost (a tie is a split).  Never a
// sum of floors formed on its own and never a budget taken off the unsplit cost: f32 addition is not associative, and
// only this order is the order of the sum the bound stands for.  With no child left it is the plain comparison.
// *bound = the bound where it cut: it loses the comparison the caller makes next and is never used as a cost.
// The floors are read from the constant block here, at the check, not carried through the searches as scalars; the
// adds run on the vector unit (no scalar f32 add on gfx950) and the branch is scalar (uni_f).
__device__ __forceinline__ bool split_floor_cut(const Ctx& c, float partial, int n, int fi, bool chroma, float unsplit,
                                                float* bound) {
    if (!kSplitCut) return false;
    float b = partial;
    const float f = c.k->split_floor[fi];
    for (int i = 0; i < n; ++i) b = b + f;
    if (chroma) b = b + c.k->split_floor[1];
    b = uni_f(b);
    if (!(b > unsplit)) return false;
    *bound = b;
    return true;
}

// K_SPLIT8: the split candidate of an 8x8 CU (ctu.rs:1990-2063: four DUAL_TREE_LUMA 4x4 CUs, then the DUAL_TREE_CHROMA
// CU) in ONE request: leaf4_search four times, leafc4_search once, with what the tree walk did between them -- the
// leaf's originals staged, the decision maps filled (the chroma leaf's DM mode is the luma mode of the 4x4 covering
// the parent's centre, block_splitter.rs:795-805), the costs summed in z-order in f32 from 0.0 (:1116-1123).  Five control
// steps of 3-6 k cycles each fewer per 8x8 node, 80 per CTU at max-split-depth 3.
// The leaves from the one on before which the split has lost against q.fcur, the node's unsplit cost, are not searched (kSplitCut).
// The check runs before every leaf, the first one included, with the leaves still to come at their floors (split_floor_cut).
// (Only the kernels built for max-split-depth 3 contain it, D3 below: inlined into the one evaluator of a kernel that also
// serves depth 2, which never splits an 8x8, it cost that depth 2.5 %; as an out-of-line function it cost both depths more.)
// *leaves (where asked for): 0 when the split was cut before its first leaf, so that nothing has touched the tile or the maps
__device__ __forceinline__ Res split8_search(const Ctx& c, const Req& q, int* overflow, int* leaves) {
    Res r = res_none();
    float split8 = 0.0f;
#pragma unroll 1
    for (int i8 = 0; i8 < 4; ++i8) {
        Req ql = {}; // (only what leaf4_search reads: a copy of q would keep thirty scalars alive across the four searches)
        ql.comps = 1;
        ql.tx = q.tx + (i8 & 1) * 4;
        ql.ty = q.ty + (i8 >> 1) * 4;
        ql.tlg = 2;
        ql.refs0 = true;
        ql.refs1 = false;
        ql.tree = TREE_DUAL_LUMA;
        if (split_floor_cut(c, split8, 4 - i8, 0, true, q.fcur, &r.vmin)) { // (before the first leaf: the split is skipped whole)
            PROF_ADD2(PH_CUT + 0, 0, 4 - i8);
            PROF_ADD2(PH_CUT + 1, 0, 1);
            PROF_ADD2(PH_CUT + 4, 0, split8 > q.fcur ? 0 : 1);
            return r;
        }
        if (leaves) *leaves = 1;
        PROF_MARK(l4g0_);
        stage_org_leaf(c, 1, ql.tx, ql.ty, 2);
        PROF_MARK(l4g1_);
        PROF_ADD2(PH_L4 + 0, l4g0_, l4g1_);
        const Res rl = leaf4_search(c, ql, overflow);
        fill_maps(ql.tx, ql.ty, 2, rl.imin, 0, true, false);
        split8 = uni_f(split8 + rl.vmin);
    }
    if (split_floor_cut(c, split8, 0, 0, true, q.fcur, &r.vmin)) {
        PROF_ADD2(PH_CUT + 1, 0, 1);
        PROF_ADD2(PH_CUT + 4, 0, split8 > q.fcur ? 0 : 1);
        return r;
    }
    Req qc = {};
    qc.tx = q.tx;
    qc.ty = q.ty;
    qc.comps = 2;
    qc.tlg = 3;
    qc.ml = 0;
    qc.mc = uni((int)SH.luma_mode[((q.ty + 4) >> 2) * 8 + ((q.tx + 4) >> 2)]); // DM = the luma mode at the parent's centre
    qc.refs0 = false;
    qc.refs1 = true;
    qc.tree = TREE_DUAL_CHROMA;
    PROF_MARK(l4c0_);
    stage_org_leaf(c, 2, q.tx, q.ty, 3);
    const Res rc = leafc4_search(c, qc, overflow);
    fill_maps(q.tx, q.ty, 3, 0, rc.imin, false, true);
    PROF_MARK(l4c1_);
    PROF_ADD2(PH_L4 + 4, l4c0_, l4c1_);
    r.vmin = uni_f(split8 + rc.vmin);
    return r;
}

// ---------------------------------------------------------------------------
// Search control as state machines: a step function runs until it needs a block evaluated, stores
// the request and where to continue, and returns true; the driver evaluates the block and calls
// it again with the result.  All state lives in LDS (CtuSt / LeafSt, wave-uniform); the control
// flow is a plain loop around a switch (reducible, all scalar branches).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void req_full(Req& q, int comps, int tx, int ty, int tlg, int ml, int mc, bool active,
                                         bool refs0, bool refs1, bool final) {
    q.kind = K_FULL;
    q.comps = comps;
    q.tx = tx;
    q.ty = ty;
    q.tlg = tlg;
    q.ml = ml;
    q.mc = mc;
    q.active = active;
    q.refs0 = refs0;
    q.refs1 = refs1;
    q.final = final;
    q.stage = (final && tlg <= 4) ? comps : 0; // a final-pass block is evaluated once: stage its originals now
    q.pre_copy = COPY_NONE;
    q.xchg = false;
}

__device__ __forceinline__ void req_copy(Req& q, int mode, int comps, int slot, int tx, int ty, int tlg) {
    q.pre_copy = mode;
    q.copy_comps = comps;
    q.copy_slot = slot;
    q.copy_tx = tx;
    q.copy_ty = ty;
    q.copy_tlg = tlg;
    q.copy_from = -1;
}

// (the numbers index the profile build's counters, tools/phase_profile.py: the gaps are states that are gone)
enum {
    C_START = 0, C_CCLM = 11, C_DM = 12,
    C_L8 = 20, C_L16 = 21, C_WINNER = 22
};

// slot: where the search keeps its best candidate's reconstruction (0 = the leaf's own slot; 1 + level when the wave
// schedule goes on to test the block's split: the slot then already holds the unsplit candidate, see ctu_step)
// Every leaf that is searched step by step is a SINGLE_TREE block; the leaves of an 8x8 split are searched inside K_SPLIT8.
__device__ __forceinline__ void leaf_init(LeafSt& s, int bx, int by, int lg, int slot = 0) {
    s.cont = C_START;
    s.bx = (uint8_t)bx;
    s.by = (uint8_t)by;
    s.lg = (uint8_t)lg;
    s.need_refs0 = 1;
    s.need_refs1 = 1;
    s.need_org = lg <= 4 ? 1 : 0;
    s.need_save = 0;
    s.tile_best = 0;
    s.slot = (uint8_t)slot;
}

// a new best candidate's reconstruction is saved to slot 0 by the request that follows it (before
// anything overwrites the tile)
__device__ __forceinline__ void leaf_attach_save(LeafSF& s, Req& q) {
    q.pre_copy = COPY_NONE;
    if (s.need_save) {
        req_copy(q, COPY_SAVE, 3, s.slot, s.bx, s.by, s.lg);
        s.need_save = 0;
    }
}
// the first evaluation of a leaf stages the originals of all the leaf's components (blocks <= 16x16)
__device__ __forceinline__ void leaf_attach_org(LeafSF& s, Req& q) {
    q.stage = 0;
    if (s.need_org) {
        q.stage = 3;
        s.need_org = 0;
    }
}
// a request that only saves / restores a reconstruction
__device__ __forceinline__ void leaf_copy_only(LeafSF& s, Req& q, int mode, int comps, int cont) {
    q.kind = K_NOP;
    q.xchg = false;
    req_copy(q, mode, comps, s.slot, s.bx, s.by, s.lg);
    s.cont = (uint8_t)cont;
}

// full evaluation (get_intra_pred_cost, block_splitter.rs:110-474) of comps with modes [ml, mc, mc];
// the first request of a leaf for a component also (re)builds its reference samples
__device__ __forceinline__ void leaf_full(LeafSF& s, Req& q, int comps, int ml, int mc, bool act, int cont) {
    const bool r0 = (comps & 1) && s.need_refs0 != 0;
    const bool r1 = (comps & 2) && mc < LT_CCLM && s.need_refs1 != 0;
    req_full(q, comps, s.bx, s.by, s.lg, ml, mc, act, r0, r1, false);
    q.tree = TREE_SINGLE;
    leaf_attach_org(s, q);
    leaf_attach_save(s, q);
    if (act) {
        if (r0) s.need_refs0 = 0;
        if (r1) s.need_refs1 = 0;
    }
    s.op_ml = (uint8_t)ml;
    s.op_mc = (uint8_t)mc;
    s.op_act = act ? 1 : 0;
    s.cont = (uint8_t)cont;
}

// the SAD (get_chroma_intra_pred_aux_cost) of the chroma pair under one CCLM mode (K_SADLIST)
__device__ __forceinline__ void leaf_sadlist(LeafSF& s, Req& q, int mc, int cont) {
    q.kind = K_SADLIST;
    q.xchg = false;
    q.tree = TREE_SINGLE;
    q.comps = 2;
    q.tx = s.bx;
    q.ty = s.by;
    q.tlg = s.lg;
    q.mc = mc;
    q.refs0 = false;
    q.refs1 = false; // (a CCLM mode reads no reference samples)
    leaf_attach_org(s, q);
    leaf_attach_save(s, q);
    s.cont = (uint8_t)cont;
}

// the whole CCLM part of a leaf search as one request (K_CCLMSEARCH): chroma pair only
__device__ __forceinline__ void leaf_cclmsearch(LeafSF& s, Req& q, int cont) {
    leaf_full(s, q, 2, 0, LT_CCLM, true, cont); // (the mode is a placeholder >= LT_CCLM: no reference samples needed)
    q.kind = K_CCLMSEARCH;
}

// the whole SAD part of a leaf search as one request (K_SADSEARCH)
__device__ __forceinline__ void leaf_sadsearch(LeafSF& s, Req& q, int cont) {
    q.kind = K_SADSEARCH;
    q.xchg = false;
    q.tree = TREE_SINGLE;
    q.comps = 3;
    q.tx = s.bx;
    q.ty = s.by;
    q.tlg = s.lg;
    q.refs0 = s.need_refs0 != 0;
    q.refs1 = s.need_refs1 != 0;
    if (q.refs0) s.need_refs0 = 0;
    if (q.refs1) s.need_refs1 = 0;
    leaf_attach_org(s, q);
    leaf_attach_save(s, q);
    s.cont = (uint8_t)cont;
}

// the whole search of an 8x8 SINGLE_TREE leaf as one request (K_LEAF8, leaf8_search)
__device__ __forceinline__ void leaf_leaf8(LeafSF& s, Req& q, int cont) {
    req_full(q, 3, s.bx, s.by, s.lg, 0, 0, true, s.need_refs0 != 0, s.need_refs1 != 0, false);
    q.kind = K_LEAF8;
    q.tree = TREE_SINGLE;
    leaf_attach_org(s, q);
    leaf_attach_save(s, q);
    s.need_refs0 = 0;
    s.need_refs1 = 0;
    s.cont = (uint8_t)cont;
}

// the full candidates of a 16x16 SINGLE_TREE leaf as one request (K_LEAF16, leaf16_search)
__device__ __forceinline__ void leaf_leaf16(LeafSF& s, Req& q, int cont) {
    leaf_leaf8(s, q, cont);
    q.kind = K_LEAF16;
}

__device__ __forceinline__ EvalParts res_parts(const Res& r) {
    EvalParts e;
    e.ssd_y = r.ssd_y;
    e.ssd_c = r.ssd_c;
    e.lvl_y = r.lvl_y;
    e.lvl_c = r.lvl_c;
    return e;
}
__device__ __forceinline__ void put_parts(EvalPartsSF& d, const EvalParts& e) {
    d.ssd_y = e.ssd_y;
    d.ssd_c = e.ssd_c;
    d.lvl_y = e.lvl_y;
    d.lvl_c = e.lvl_c;
}

// the step machines' running best takes a candidate: cost, parts, luma mode and its MPM class.  Where the winner's
// reconstruction then is stays with the caller: the wave schedule sets need_save / tile_best, the team schedule holder.
__device__ __forceinline__ void leaf_take(LeafSF& s, float val, const EvalParts& parts, int mode, int cls) {
    s.best_cost = val;
    put_parts(s.e_best, parts);
    s.mode = (uint8_t)mode;
    s.best_cls = (uint8_t)cls;
}
// One step of the search of a SINGLE_TREE leaf (block_splitter.rs:886-1078).  An 8x8 leaf is one request (C_L8), a 16x16
// leaf one request and its CCLM part (C_L16, C_WINNER ..); of a 32x32 leaf only the CCLM part of the team schedule's
// member 0 runs here (from C_WINNER), the wave kernels search theirs in one request (K_LEAF32, ctu_step).  r is the
// result of the request the previous step made (unused at the first step).  Returns false when the leaf is decided
// (s.cost, s.luma_mode, s.chroma_mode).
__device__ __forceinline__ bool leaf_step(const Ctx& c, LeafSF& s, const Res& r, Req& q) {
    constexpr int tree = TREE_SINGLE;
    int cont = s.cont;
    const EvalParts rp = res_parts(r);
    for (;;) {
        switch (cont) {
        case C_START: // candidates {0,1,2,7,13,18,23,29,34,39,45,50,55,60,66} (:887)
            if (s.lg == 3) { // an 8x8 leaf: the whole search in one request, candidates in packs
                leaf_leaf8(s, q, C_L8);
                return true;
            }
            // a 16x16 leaf: its five full candidates and the SAD search in one request.  (A 32x32 leaf never starts here: the
            // wave kernels search it inside K_LEAF32, the team's member 0 joins at C_WINNER, leaf_step_team TC_D)
            leaf_leaf16(s, q, C_L16);
            return true;
        case C_L16: // the winner of [planar, DC, cm, cm - 1, cm + 1] is in the tile; it is saved by the next request
            leaf_take(s, r.vmin, rp, r.imin, mpm_class(c, s.bx, s.by, s.lg, r.imin));
            s.need_save = 1;
            s.tile_best = 1;
            cont = C_WINNER;
            break;
        case C_L8:
            s.cost = r.vmin;
            s.luma_mode = (uint8_t)r.imin;
            s.chroma_mode = (uint8_t)r.imin2;
            return false;
        case C_WINNER: {
            s.cost = s.best_cost;
            const int m = s.mode;
            s.luma_mode = (uint8_t)m;
            s.chroma_mode = (uint8_t)m;
            // :989-1037 re-runs the winner's luma to have its reconstruction in the tile; here the
            // winner's reconstruction comes back from slot 0 unless it is still in the tile
            const bool in_tile = s.tile_best != 0;
            // :1040 get_chroma_intra_pred_cost(mode) repeats the winner's chroma evaluation: re-use it
            s.cur_cost = uni_f(assemble_chroma_cost(c, m, s.e_best.get()));
            if (c.trace && LANE == 0)
                TRACE_REC(c.ctu_x + s.bx, c.ctu_y + s.by, s.lg, tree, 3, 0, m, __float_as_int((float)s.cur_cost));
            // the three CCLM probes, the pick and the evaluation of the picked mode in one request (K_CCLMSEARCH)
            leaf_cclmsearch(s, q, C_CCLM);
            if (!in_tile) req_copy(q, COPY_RESTORE, 1, s.slot, s.bx, s.by, s.lg); // (its save went out earlier)
            return true;
        }
        case C_CCLM: {
            // the CCLM candidate = the winner's luma parts + the chroma parts just evaluated
            s.cclm_mode = (uint8_t)r.imin;
            EvalParts e = s.e_best.get();
            e.ssd_c = rp.ssd_c;
            e.lvl_c = rp.lvl_c;
            const float cclm_cost = uni_f(assemble_chroma_cost(c, s.cclm_mode, e));
            if (c.trace && LANE == 0)
                TRACE_REC(c.ctu_x + s.bx, c.ctu_y + s.by, s.lg, tree, 3, 0, s.cclm_mode, __float_as_int(cclm_cost));
            // :1062-1072 final get_intra_pred_cost: luma = the winner (its mpm_class from its candidate evaluation); the
            // chroma pair is the DM evaluation (its reconstruction comes back from slot 0) or the CCLM evaluation just made.
            // (chroma_final's decision spelt out: called here, in any of five shapes, it cost the wave kernels 2 VGPRs)
            const int m = s.mode;
            const int bcls = s.best_cls; // mpm_class of the winner, from its candidate evaluation
            if (dm_keeps(s.cur_cost, cclm_cost)) {
                s.cost = uni_f(assemble_cost(c, tree, bcls, m, s.e_best.get()));
                leaf_copy_only(s, q, COPY_RESTORE, 2, C_DM);
                return true;
            }
            s.chroma_mode = s.cclm_mode;
            s.cost = uni_f(assemble_cost(c, tree, bcls, s.cclm_mode, e));
            return false;
        }
        default: // C_DM: the DM chroma is back in the tile
            return false;
        }
    }
}


// ---------------------------------------------------------------------------
// Team schedule: kTeam = 4 waves search ONE CTU.  Every member runs the same control flow on its own copy
// of the state and of the reconstruction tile; where the reference's leaf search evaluates candidates that
// do not depend on each other (block_splitter.rs:887-898: the 15 first-round candidates read only
// neighbours outside the block; :905-973 the two probes of a step-search round; :974 the three full
// evaluations of the last round; the three CCLM probes), each member evaluates ONE of them, the members
// publish their results in LDS (XRes) and meet at a workgroup barrier, and every member then makes the
// reference's decisions from all results in the reference's order.  A full candidate's reconstruction is
// saved to its evaluator's slot 0 in global scratch; once the leaf is decided every member restores the
// winner from the slot of the member that holds it, so all tiles agree again before the next block.
// Quantisation is solo (every member walks its own trellis): between exchanges the members run freely.
// ---------------------------------------------------------------------------

// published result of member m in the exchange that just completed (parity par)
__device__ __forceinline__ EvalParts xparts(const Ctx& c, int par, int m) {
    const XRes& x = team_lds(c, m).xr[par];
    EvalParts e;
    e.ssd_y = (uint32_t)uni((int)x.ssd_y);
    e.ssd_c = (uint32_t)uni((int)x.ssd_c);
    e.lvl_y = uni_i64(x.lvl_y);
    e.lvl_c = uni_i64(x.lvl_c);
    return e;
}
// K_SADSEARCH: the SAD of the mode found (f32 bits in ssd_y), the mode (ssd_c); K_SADLIST: the SAD (lvl_y)
__device__ __forceinline__ float xvmin(const Ctx& c, int par, int m) { return __int_as_float(uni((int)team_lds(c, m).xr[par].ssd_y)); }
__device__ __forceinline__ int ximin(const Ctx& c, int par, int m) { return uni((int)team_lds(c, m).xr[par].ssd_c); }
__device__ __forceinline__ float xv0(const Ctx& c, int par, int m) { return __int_as_float(uni((int)team_lds(c, m).xr[par].lvl_y)); }

__device__ __forceinline__ void team_publish(const Req& q, const Res& r, int par) {
    XRes x;
    if (q.kind == K_FULL) {
        x.ssd_y = r.ssd_y;
        x.ssd_c = r.ssd_c;
        x.lvl_y = r.lvl_y;
        x.lvl_c = r.lvl_c;
    } else {
        x.ssd_y = (uint32_t)__float_as_int(r.vmin);
        x.ssd_c = (uint32_t)r.imin;
        x.lvl_y = (long long)(unsigned)__float_as_int(r.v0);
        x.lvl_c = 0;
    }
    if (LANE == 0) SH.xr[par] = x;
}

enum { TC_START = 0, TC_A = 1, TC_D = 2, TC_E = 3, TC_F = 4 };

// a member with nothing to evaluate in a stage
__device__ __forceinline__ void team_idle(Req& q) {
    q.kind = K_NOP;
    q.pre_copy = COPY_NONE;
}
// every member copies comps of the leaf's block from the tile of member `holder` (who holds the winner's
// reconstruction) into its own tile: attached to q as a COPY_PULL, which every member must issue
__device__ __forceinline__ void team_restore(const Ctx& c, const LeafSF& s, Req& q, int comps, int holder) {
    req_copy(q, COPY_PULL, comps, 0, s.bx, s.by, s.lg);
    q.copy_from = holder;
}

// the leaf is decided: the winner's comps come from member `holder`'s tile -- deferred to the driver loop, which
// pulls before the next evaluation (one control step and one empty request less per leaf)
__device__ __forceinline__ void team_defer_pull(CtuSt& t, const LeafSF& s, int comps, int holder) {
    t.dp1 = (uint8_t)((s.bx >> 2) | ((s.by >> 2) << 3));
    t.dp0 = (uint8_t)(1 | (comps << 1) | (holder << 3) | ((s.lg - 2) << 5));
}

// One step of the search of the CTU's 32x32 candidate in the team schedule (the level schedule takes over once it is
// decided, see TC_D; the CCLM stages TC_E and TC_F run at max-split-depth 0 only); par = parity of the exchange that delivered the results
// of the previous step's requests.  Same decisions, in the same order, as leaf_step.
__device__ __forceinline__ bool leaf_step_team(const Ctx& c, CtuSt& t, LeafSF& s, Req& q, int par, const Res& r) {
    constexpr int tree = TREE_SINGLE;
    const int me = c.member;
    int cont = s.cont;
    for (;;) {
        switch (cont) {
        case TC_START: // stage A: planar | DC | the directional SAD search (:887-973)
            if (me == 0) {
                leaf_full(s, q, 3, PLANAR, PLANAR, true, TC_A);
            } else if (me == 1) {
                leaf_full(s, q, 3, DC, DC, true, TC_A);
            } else if (me == 2) {
                leaf_sadsearch(s, q, TC_A); // the 13 directional SADs + both step-search rounds (K_SADSEARCH)
            } else {
                team_idle(q);
            }
            s.cont = TC_A;
            q.xchg = true;
            return true;
        case TC_A: {
            const EvalParts e0 = xparts(c, par, 0), e1 = xparts(c, par, 1);
            const float v0 = uni_f(assemble_cost(c, tree, 0, PLANAR, e0));
            const int cls1 = mpm_class(c, s.bx, s.by, s.lg, DC);
            const float v1 = uni_f(assemble_cost(c, tree, cls1, DC, e1));
            if (c.write && LANE == 0) {
                TRACE_REC(c.ctu_x + s.bx, c.ctu_y + s.by, s.lg, tree, 1, PLANAR, PLANAR, __float_as_int(v0));
                TRACE_REC(c.ctu_x + s.bx, c.ctu_y + s.by, s.lg, tree, 1, DC, DC, __float_as_int(v1));
            }
            if (v1 < v0) { // first minimum of [planar, DC, ...] as a running strict-less update
                leaf_take(s, v1, e1, DC, cls1);
                s.holder = 1;
            } else {
                leaf_take(s, v0, e0, PLANAR, 0);
                s.holder = 0;
            }
            // member 2 searched the directional modes (K_SADSEARCH): its winner and its SAD
            s.cur_mode = (uint8_t)ximin(c, par, 2);
            s.cur_cost = xvmin(c, par, 2);
            // stage D: cm, cm - 1, cm + 1 side by side (:974) on the three members that do not hold the
            // best of {planar, DC}; candidate k goes to the k-th of them in ascending order
            const int cm = s.cur_mode, holder = s.holder;
            const int k = me - (me > holder ? 1 : 0); // my candidate, if I am not the holder
            const int mode = k == 0 ? cm : (k == 1 ? cm - 1 : cm + 1);
            const bool act = k == 0 || (k == 1 ? !(cm < 3) : !(cm + 1 > 66));
            if (me != holder && act) {
                leaf_full(s, q, 3, mode, mode, true, TC_D);
            } else {
                team_idle(q);
            }
            s.cont = TC_D;
            q.xchg = true;
            return true;
        }
        case TC_D: {
            const int cm = s.cur_mode, holder0 = s.holder;
#pragma unroll 1
            for (int k = 0; k < 3; ++k) {
                const int mode = k == 0 ? cm : (k == 1 ? cm - 1 : cm + 1);
                const bool act = k == 0 || (k == 1 ? !(cm < 3) : !(cm + 1 > 66));
                if (!act) continue; // a skipped evaluation costs f32::MAX in the reference: never a new minimum
                const int mem = k + (k >= holder0 ? 1 : 0);
                const EvalParts e = xparts(c, par, mem);
                const int cls = mpm_class(c, s.bx, s.by, s.lg, mode);
                const float val = uni_f(assemble_cost(c, tree, cls, mode, e));
                if (c.write && LANE == 0)
                    TRACE_REC(c.ctu_x + s.bx, c.ctu_y + s.by, s.lg, tree, 1, mode, mode, __float_as_int(val));
                if (val < s.best_cost) {
                    leaf_take(s, val, e, mode, cls);
                    s.holder = (uint8_t)mem;
                }
            }
            s.cost = s.best_cost;
            const int m = s.mode, holder = s.holder;
            s.luma_mode = (uint8_t)m;
            s.chroma_mode = (uint8_t)m;
            if (s.lg == 5 && c.k->max_depth >= 1) {
                // The CTU's 32x32 candidate, and the level schedule follows: its LUMA mode is all the other levels need
                // (their MPM classes), and it is decided now.  Everybody pulls the winner (member 0 keeps
                // the candidate for the CTU's decision); then members 1 .. 3 are done with this leaf and start their
                // levels, while member 0 finishes the candidate alone -- its CCLM part as the one-wave search does it
                // (leaf_step from C_WINNER: the winner saved to slot 0 by the CCLM request, restored from there if DM wins).
                team_defer_pull(t, s, 3, holder);
                if (me != 0) return false;
                s.need_save = 1;
                s.tile_best = 1;
                s.cont = C_WINNER;
                t.lvmode = 1; // from here on ctu_step runs this member's leaf through leaf_step; an empty request first
                team_idle(q); // (the driver loop pulls the winner in front of it, as the others do at the switch)
                q.xchg = false;
                return true;
            }
            // :1040 the winner's chroma cost, then the three CCLM probes side by side on the winner's luma
            s.cur_cost = uni_f(assemble_chroma_cost(c, m, s.e_best.get()));
            if (c.write && LANE == 0)
                TRACE_REC(c.ctu_x + s.bx, c.ctu_y + s.by, s.lg, tree, 3, 0, m, __float_as_int((float)s.cur_cost));
            // the three CCLM probes side by side on the winner's luma, which everybody pulls first (one member doing
            // the three-mode pass and the evaluation in one request, as the wave schedule does, measured 3 % slower here)
            if (me < 3)
                leaf_sadlist(s, q, me == 0 ? LT_CCLM : (me == 1 ? T_CCLM : L_CCLM), TC_E);
            else
                team_idle(q);
            team_restore(c, s, q, 3, holder);
            s.cont = TC_E;
            q.xchg = true;
            return true;
        }
        case TC_E: {
            const int cm = pick_cclm(xv0(c, par, 0), xv0(c, par, 1), xv0(c, par, 2));
            s.cclm_mode = (uint8_t)cm;
            const int ev = (s.holder + 1) & (kTeam - 1); // never the holder: its tile keeps the DM chroma
            s.evalr = (uint8_t)ev;
            if (me == ev) {
                leaf_full(s, q, 2, 0, cm, true, TC_F);
            } else {
                team_idle(q);
            }
            s.cont = TC_F;
            q.xchg = true;
            return true;
        }
        case TC_F: {
            const int ev = s.evalr, holder = s.holder;
            const EvalParts rp = xparts(c, par, ev);
            EvalParts e = s.e_best.get();
            e.ssd_c = rp.ssd_c;
            e.lvl_c = rp.lvl_c;
            const float cclm_cost = uni_f(assemble_chroma_cost(c, s.cclm_mode, e));
            if (c.write && LANE == 0)
                TRACE_REC(c.ctu_x + s.bx, c.ctu_y + s.by, s.lg, tree, 3, 0, s.cclm_mode, __float_as_int(cclm_cost));
            const ChromaFinal f = chroma_final(c, s.cur_cost, cclm_cost, s.e_best.get(), e, s.best_cls, s.mode, s.cclm_mode);
            s.cost = f.cost;
            if (!f.dm_wins) s.chroma_mode = s.cclm_mode;
            // DM wins: only the evaluator's tile holds the CCLM chroma, it takes the DM chroma back
            team_defer_pull(t, s, 2, f.dm_wins ? holder : ev);
            return false;
        }
        default:
            return false;
        }
    }
}

// ---------------------------------------------------------------------------
// Level schedule (team kernel at max-split-depth 3): after the team has searched the CTU's 32x32 candidate together
// (every in-CTU cost needs that candidate's luma mode: SURVEY.md Q7), the members take one TREE LEVEL each and run
// ahead side by side: member 1 the four 16x16 leaf searches, member 2 the sixteen 8x8 ones, member 3 the sixteen
// 8x8 SPLITS (four 4x4 luma leaves + the chroma leaf each); member 0 keeps the 32x32 candidate in its tile.  A
// node's unsplit search and the search of everything below it read only neighbours outside the node
// (block_splitter.rs:1081-1123), so the levels depend on each other only through DECISIONS: node (L, i) is decided --
// unsplit against the sum of its decided children, :1116-1145 -- by the members L .. 3 together once member L has
// searched it and its children are decided; whoever lost copies the winner's reconstruction and decision maps from
// the tile of the member that holds them (LDS to LDS), so every member's tile shows later blocks exactly the
// neighbourhood the reference's depth-first search shows them.  Each member runs the ordinary one-wave leaf search
// (leaf_step with the packed requests K_LEAF16 / K_LEAF8; member 3 issues K_SPLIT8), solo trellis walks throughout.
// A decision has two meeting points (everybody arrived: the costs are posted; everybody has copied: tiles may be
// written again); they are counters in LDS that the members of the decision poll -- a workgroup barrier would also
// stop the members of other levels, who are in the middle of their own searches.  Same decisions, same f32 sums in
// the same order as ctu_step's depth-first walk; the final pass is shared by quadrant (every member ends with the
// final tile and maps).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void lv_meet(int L, int which, int target) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (LANE == 0) {
        __hip_atomic_fetch_add(&SHT.lvb.cnt[L][which], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        // (bounded: a member that never arrives must not hang the device; the cap is seconds, a CTU takes milliseconds,
        // and the host reports it: SHT.lvb.pad_ -> WRENC_GPU_EHIP through the overflow word, bit 1)
        int polls = 0;
        while (__hip_atomic_load(&SHT.lvb.cnt[L][which], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (unsigned)target) {
            __builtin_amdgcn_s_sleep(2);
            if (++polls > (1 << 23)) {
                SHT.lvb.pad_ = 1;
                break;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    WSYNC();
}
// position of node i of tree level L in z-order (L = 0: the CTU, 1: 16x16, 2: 8x8)
__device__ __forceinline__ void lv_node(int L, int i, int& bx, int& by) {
    if (L == 0) {
        bx = by = 0;
    } else if (L == 1) {
        bx = (i & 1) * 16;
        by = (i >> 1) * 16;
    } else {
        const int qd = i >> 2, sb = i & 3;
        bx = (qd & 1) * 16 + (sb & 1) * 8;
        by = (qd >> 1) * 16 + (sb >> 1) * 8;
    }
}
// the decision maps of a block from member `from`'s LDS (the split candidate's: they differ per 4x4 unit)
__device__ __forceinline__ void lv_pull_maps(const Ctx& c, int from, int bx, int by, int lg) {
    const Lds& src = team_lds(c, from);
    const int l4 = lg - 2;
    if (LANE < (1 << (2 * l4))) {
        const int idx = ((by >> 2) + (LANE >> l4)) * 8 + (bx >> 2) + (LANE & ((1 << l4) - 1));
        SH.cu_log2[idx] = src.cu_log2[idx];
        SH.luma_mode[idx] = src.luma_mode[idx];
    }
    const int l8 = lg - 3;
    if (LANE < (1 << (2 * l8))) {
        const int idx = ((by >> 3) + (LANE >> l8)) * 4 + (bx >> 3) + (LANE & ((1 << l8) - 1));
        SH.chroma_mode[idx] = src.chroma_mode[idx];
    }
    WSYNC();
}
// block from member `from`'s tile into this member's (copy_block's COPY_PULL without its workgroup barrier)
__device__ __forceinline__ void lv_pull(const Ctx& c, int from, int tx, int ty, int tlg) {
    const Lds& src = team_lds(c, from);
    const int words = 1 << (2 * tlg - 2);
    for (int w = LANE; w < words; w += 64) {
        const int row = (4 * w) >> tlg, col = (4 * w) & ((1 << tlg) - 1);
        const int at = (ty + row) * 36 + tx + col + 4;
        *(uint32_t*)&SH.recY[at] = *(const uint32_t*)&src.recY[at];
    }
    const int lg = tlg - 1;
    const int cwords = 1 << (2 * lg - 2); // per plane
    for (int w = LANE; w < 2 * cwords; w += 64) {
        const int pl = w >= cwords ? 1 : 0;
        const int ww = w - pl * cwords;
        const int row = (4 * ww) >> lg, col = (4 * ww) & ((1 << lg) - 1);
        const int at = ((ty >> 1) + row) * 20 + (tx >> 1) + col + 4;
        *(uint32_t*)&SH.recC[pl][at] = *(const uint32_t*)&src.recC[pl][at];
    }
    WSYNC();
}
// Decision of node (L, idx), by members L .. 3: returns the decided cost (block_splitter.rs:1125-1151)
__device__ __forceinline__ float lv_decide(const Ctx& c, int L, int idx) {
    const int me = c.member;
    const int dl = c.k->max_depth;                      // levels 1 .. dl are searched by members 1 .. dl
    const int nmem = L == 0 ? kTeam : dl - L + 1;       // (the CTU's decision: everybody, idle members included)
    PROF_MARK(tx0_);
    lv_meet(L, 0, (idx + 1) * nmem);
    PROF_MARK(tx1_);
    PROF_ADD2(PH_XCHG, tx0_, tx1_);
    PROF_ADDM(2, tx0_, tx1_);
    const float ns = uni_f(SHT.lvb.ns_cost[L]), sp = uni_f(SHT.lvb.split[L]);
    const int ml = uni((int)SHT.lvb.ml[L]), mc = uni((int)SHT.lvb.mc[L]);
    int bx, by;
    lv_node(L, idx, bx, by);
    const int lg = 5 - L;
    const bool unsplit = sp > ns; // :1125-1145 (ties => split)
    if (unsplit) {
        if (me > L) lv_pull(c, L, bx, by, lg);
        fill_maps(bx, by, lg, ml, mc, true, true);
    } else if (me == L || me > dl) { // (members without a level hold nothing of the split candidate either)
        lv_pull(c, L + 1, bx, by, lg);
        lv_pull_maps(c, L + 1, bx, by, lg);
    }
    PROF_MARK(tx2_);
    lv_meet(L, 1, (idx + 1) * nmem);
    PROF_MARK(tx3_);
    PROF_ADD2(PH_COPY, tx1_, tx2_);
    PROF_ADD2(PH_XCHG, tx2_, tx3_);
    PROF_ADDM(2, tx2_, tx3_);
    return unsplit ? ns : sp;
}
__device__ __forceinline__ void lv_post_unsplit(int L, float ns, int ml, int mc) {
    if (LANE == 0) {
        SHT.lvb.ns_cost[L] = ns;
        SHT.lvb.ml[L] = (uint8_t)ml;
        SHT.lvb.mc[L] = (uint8_t)mc;
    }
}
__device__ __forceinline__ void lv_post_split(int L, float sp) {
    if (LANE == 0) SHT.lvb.split[L] = sp;
}


// split_ct (block_splitter.rs:782-1154) for one CTU + the final pass (ctu_encoder.rs:1421-1461):
// exhaustive quad-tree search as an explicit depth-first walk (level 0 = 32x32 ... level 2 = 8x8;
// an 8x8 node's split is four DUAL_TREE_LUMA 4x4 leaves + one DUAL_TREE_CHROMA 4x4 leaf,
// ctu.rs:1990-2063), per-level state in LDS.
//
// Decided blocks whose reconstruction was overwritten by later candidates come back from the
// slots in global scratch they were saved to (copy_block): the reference's cache_reconsts /
// restore_reconsts (block_splitter.rs:807-840, 1085-1145), with the saved planes kept in L2/HBM
// instead of LDS.
// (the numbers index the profile build's counters, tools/phase_profile.py: 5 was a state of the 4x4 leaf walk K_SPLIT8 replaced)
enum { T_START = 0, T_ENTER = 1, T_NODE_LEAF = 2, T_NODE8 = 3, T_LEAF32 = 4, T_REGEN_DONE = 6, T_RETURN = 7, T_FINAL_Z = 8, T_FZ_TAIL = 9, T_FZ_NEXT = 10,
       T_LV_UNIT = 11, T_LV_LEAFDONE = 12, T_LV_UP = 13, T_SPLIT8 = 14, T_LV_SERVE = 15 };

template <bool TEAM, bool D3>
__device__ __forceinline__ bool ctu_step(Ctx& c, const Res& r, Req& q) {
    CtuSt& t = SH.st;
    bool in_leaf = t.in_leaf != 0;
    int cont = t.cont;
    for (;;) {
        if (in_leaf) {
            // team schedule: the results of the previous requests are in the members' XRes of parity xpar ^ 1
            LeafSF ls = snap_leaf(t.leaf);
            if ((TEAM && !t.lvmode) ? leaf_step_team(c, t, ls, q, t.xpar ^ 1, r) : leaf_step(c, ls, r, q)) {
                if (t.pend) { // the first request of a node's first child saves the unsplit candidate
                    req_copy(q, COPY_SAVE, t.pend, t.pslot, t.pbx, t.pby, t.plg);
                    t.pend = 0;
                }
                t.cont = (uint8_t)cont;
                t.in_leaf = 1;
                return true;
            }
            t.in_leaf = 0;
            in_leaf = false;
        }
        switch (cont) {
        case T_START:
            t.level = 0;
            t.bx = 0;
            t.by = 0;
            cont = T_ENTER;
            break;
        case T_ENTER: { // enter node (bx, by) at `level`: the unsplit candidate
            const int lg = 5 - t.level;
            t.lg = (uint8_t)lg;
            if (!TEAM && D3 && lg == 3) {
                // max-split-depth 3: an 8x8 node is decided against its split inside ONE request (K_NODE8, node8_search);
                // the pending save of the parent's unsplit candidate rides on it as on any first request of a first child
                req_full(q, 3, t.bx, t.by, 3, 0, 0, true, false, false, false);
                q.kind = K_NODE8;
                q.tree = TREE_SINGLE;
                if (t.pend) {
                    req_copy(q, COPY_SAVE, t.pend, t.pslot, t.pbx, t.pby, t.plg);
                    t.pend = 0;
                }
                t.cont = T_NODE8;
                return true;
            }
            if (!TEAM && lg == 5) {
                // wave schedule, the CTU's 32x32 leaf: the whole search in ONE request (K_LEAF32, full_search), its best
                // candidate kept in slot copy_slot -- the unsplit slot when the split is tested next, see below
                req_full(q, 3, t.bx, t.by, 5, 0, 0, true, true, true, false);
                q.kind = K_LEAF32;
                q.tree = TREE_SINGLE;
                q.copy_slot = t.level < t.max_depth ? 1 + t.level : 0;
                t.cont = T_LEAF32;
                return true;
            }
            // wave schedule, a node whose split is tested next: the search saves its best candidate straight to the
            // node's slot 1 + level, which then holds the unsplit candidate without a save of its own (T_NODE_LEAF)
            leaf_init(t.leaf, t.bx, t.by, lg, (!TEAM && t.level < t.max_depth) ? 1 + t.level : 0);
            if (TEAM && !t.lvmode) t.leaf.cont = TC_START;
            in_leaf = true;
            cont = T_NODE_LEAF;
            break;
        }
        case T_NODE_LEAF: {
            const float ns = t.leaf.cost;
            const int ml = t.leaf.luma_mode, mc = t.leaf.chroma_mode;
            const int level = t.level, lg = t.lg;
            fill_maps(t.bx, t.by, lg, ml, mc, true, true);
            if (level == 0) c.cu32_mode = ml;
            if (t.max_depth - level == 0) {
                t.ret = ns;
                cont = T_RETURN;
                break;
            }
            if (TEAM) { // (max-split-depth >= 1 here)
                // ---- level schedule from here on (see lv_decide): every member has searched the 32x32 candidate ----
                if (t.dp0) { // its winner into every member's tile first (team_defer_pull)
                    const int dp = t.dp0, dq = t.dp1;
                    t.dp0 = 0;
                    copy_block(c, COPY_PULL, (dp >> 1) & 3, 0, (dq & 7) << 2, (dq >> 3) << 2, (dp >> 5) + 2, (dp >> 3) & 3);
                }
                t.lvmode = 1;
                t.lv_i = 0;
                t.lv_acc0 = 0.0f;
                t.lv_acc1 = 0.0f;
                if (c.member == 0) lv_post_unsplit(0, ns, ml, mc);
                // (members 1 .. max-split-depth take a level; member 0 and the others wait for the CTU's decision)
                cont = (c.member == 0 || c.member > t.max_depth) ? T_LV_UP : T_LV_UNIT;
                break;
            }
            // ---- wave schedule from here on ----
            // the unsplit candidate's reconstruction goes to slot 1 + level (cache_reconsts, :1085-1100):
            // the search saved its winner there already (luma and DM chroma, leaf_init above), so all that is left to
            // save is the chroma pair when the CCLM candidate won.  (An 8x8 node is never here: below max-split-depth 3 it
            // is a leaf, at depth 3 it is decided inside K_NODE8.)
            t.pend = (uint8_t)(mc >= LT_CCLM ? 2 : 0);
            t.pbx = t.bx;
            t.pby = t.by;
            t.plg = (uint8_t)lg;
            t.pslot = (uint8_t)(1 + level);
            if (LANE == 0) {
                SH.ns_cost[level] = ns;
                SH.ns_luma[level] = (uint8_t)ml;
                SH.ns_chroma[level] = (uint8_t)mc;
                SH.split_cost[level] = 0.0f;
                SH.child[level] = 0;
            }
            WSYNC();
            // four children at their floors already cost more than the unsplit candidate (split_floor_cut): the split has
            // lost before its first child.  No child has touched the tile or the maps, which hold the unsplit candidate
            // as they do for a node at max-split-depth, so there is nothing to save or to restore
            float bound;
            if (split_floor_cut(c, 0.0f, 4, 2 + level + 1, false, ns, &bound)) {
                PROF_ADD2(PH_CUT + 2 + level, 0, 4);
                PROF_ADD2(PH_CUT + 5, 0, 1);
                t.pend = 0;
                t.ret = ns;
                cont = T_RETURN;
                break;
            }
            t.level = (uint8_t)(level + 1); // descend into child 0 (same top-left corner)
            cont = T_ENTER;
            break;
        }
        case T_LEAF32: {
            if constexpr (!TEAM) { // the 32x32 leaf is decided: on as after any leaf search
                t.leaf.cost = r.vmin;
                t.leaf.luma_mode = (uint8_t)r.imin;
                t.leaf.chroma_mode = (uint8_t)r.imin2;
                cont = T_NODE_LEAF;
                break;
            }
            }
            break;
        case T_NODE8: {
            if constexpr (!TEAM && D3) { // the 8x8 node's cost came back
                t.ret = r.vmin;
                cont = T_RETURN;
                break;
            }
            }
            break;
        case T_SPLIT8: {
            if constexpr (TEAM && D3) { // level schedule: member 3's unit is done
                lv_post_split(2, r.vmin);
                cont = T_LV_UP;
                break;
            }
            }
            break;
        case T_REGEN_DONE:
            fill_maps(t.rbx, t.rby, t.rlg, t.rl, t.rc, true, true);
            t.ret = uni_f(SH.ns_cost[t.level]);
            cont = T_RETURN;
            break;
        case T_RETURN: { // return `ret` from the finished node at `level` to its parent
            const int level = t.level;
            if (level == 0) {
                t.ctu_cost = t.ret;
                t.z = 0;
                if (TEAM && t.dp0) { // the last leaf's winner is still to be pulled: one empty request for every member
                    q.kind = K_NOP;
                    q.pre_copy = COPY_NONE;
                    q.xchg = false;
                    t.cont = T_RETURN;
                    return true;
                }
                // final pass: every block reads only final neighbours, and every member's tile and maps are final, so the
                // team shares it by 16x16 quadrant (a CU is emitted by the member that owns its top-left unit)
                t.z = (uint8_t)(TEAM ? 16 * c.member : 0);
                t.zend = (uint8_t)(TEAM ? 16 * c.member + 16 : 64);
                cont = T_FINAL_Z;
                break;
            }
            const int pl = level - 1;
            const int psz = 1 << (5 - pl);
            const int pbx = t.bx & ~(psz - 1), pby = t.by & ~(psz - 1);
            // children in z-order, f32 (:1116-1123)
            const float acc = uni_f(uni_f(SH.split_cost[pl]) + t.ret);
            const int ch = uni((int)SH.child[pl]) + 1;
            WSYNC();
            if (LANE == 0) {
                SH.split_cost[pl] = acc;
                SH.child[pl] = (uint8_t)ch;
            }
            WSYNC();
            // the parent's split has lost once its partial cost, with the children still to come at their floors, is
            // strictly greater than its unsplit cost (split_floor_cut): no sibling is entered.  After the last child
            // this is the comparison itself (:1125-1145)
            const float ns_p = uni_f(SH.ns_cost[pl]);
            float bound;
            const bool lost = ch < 4 ? split_floor_cut(c, acc, 4 - ch, 2 + level, false, ns_p, &bound) : acc > ns_p;
            if (ch < 4 && !lost) { // next sibling
                t.bx = (uint8_t)(pbx + (ch & 1) * (psz >> 1));
                t.by = (uint8_t)(pby + (ch >> 1) * (psz >> 1));
                cont = T_ENTER;
                break;
            }
            PROF_ADD2(PH_CUT + 1 + level, 0, 4 - ch); // (level 2: 8x8 nodes not searched, level 1: 16x16 nodes)
            PROF_ADD2(PH_CUT + 5, 0, (ch < 4 && !(acc > ns_p)) ? 1 : 0);
            // parent complete: split vs unsplit (:1125-1145)
            t.bx = (uint8_t)pbx;
            t.by = (uint8_t)pby;
            t.level = (uint8_t)pl;
            if (lost) {
                t.rbx = (uint8_t)pbx;
                t.rby = (uint8_t)pby;
                t.rlg = (uint8_t)(5 - pl);
                t.rl = (uint8_t)uni((int)SH.ns_luma[pl]);
                t.rc = (uint8_t)uni((int)SH.ns_chroma[pl]);
                q.kind = K_NOP;
                q.xchg = false;
                req_copy(q, COPY_RESTORE, 3, 1 + pl, t.rbx, t.rby, t.rlg);
                t.cont = T_REGEN_DONE;
                return true;
            }
            t.ret = acc;
            break; // cont stays T_RETURN
        }
        // ---- level schedule: this member's next unit (members 1, 2: a leaf search; member 3: an 8x8 split) ----
        case T_LV_UNIT: {
            if constexpr (TEAM) {
                const int me = c.member, i = t.lv_i;
                int bx, by;
                lv_node(me == 1 ? 1 : 2, i, bx, by);
                t.bx = (uint8_t)bx;
                t.by = (uint8_t)by;
                if constexpr (D3) {
                    if (me == 3) { // four DUAL_TREE_LUMA 4x4 leaves, then the DUAL_TREE_CHROMA leaf, as one request (K_SPLIT8)
                        t.lg = 3;
                        req_full(q, 3, bx, by, 3, 0, 0, true, false, false, false);
                        q.kind = K_SPLIT8;
                        q.stage = 0;
                        q.tree = TREE_DUAL_LUMA;
                        q.fcur = __builtin_inff(); // every leaf: member 2 is still searching the unsplit candidate
                        t.cont = T_SPLIT8;
                        return true;
                    }
                }
                const int lg = me == 1 ? 4 : 3;
                t.lg = (uint8_t)lg;
                leaf_init(t.leaf, bx, by, lg);
                in_leaf = true;
                cont = T_LV_LEAFDONE;
                break;
            }
            }
            break;
        case T_LV_LEAFDONE: {
            if constexpr (TEAM) {
                const int me = c.member;
                if (me < t.max_depth) { // the unsplit candidate of node (member, lv_i), to be decided against its children
                    lv_post_unsplit(me, t.leaf.cost, t.leaf.luma_mode, t.leaf.chroma_mode);
                } else {                // the deepest level: the leaf is the node's decision
                    fill_maps(t.bx, t.by, t.lg, t.leaf.luma_mode, t.leaf.chroma_mode, true, true);
                }
                cont = T_LV_UP;
                break;
            }
            }
            break;
        case T_LV_UP: {
            if constexpr (TEAM) { // the decisions this member takes part in now, deepest first
                const int me = c.member, i = t.lv_i, dl = t.max_depth;
                if (me == 0 && dl >= 2 && !t.lv_i) { // (lv_i of member 0: 1 = the server is through)
                    cont = T_LV_SERVE;
                    break;
                }
                if (me == 2 && me <= dl && i == 15) lv_word_add(&SHT.lvb.job_fin); // no more 8x8 leaves
                if (D3 && me == 3 && i == 15) lv_word_add(&SHT.lvb.job4_fin);              // ... 4x4 leaves
                if (me >= 2 && me <= dl) {
                    // an 8x8 node: decided against its split at max-split-depth 3, final at depth 2
                    const float d2 = dl == 3 ? lv_decide(c, 2, i) : (float)t.leaf.cost;
                    const float a1 = uni_f(t.lv_acc1 + d2); // children in z-order, f32, from 0.0 (:1116-1123)
                    t.lv_acc1 = a1;
                    if ((i & 3) != 3) {
                        t.lv_i = (uint8_t)(i + 1);
                        cont = T_LV_UNIT;
                        break;
                    }
                    if (me == 2) lv_post_split(1, a1);
                    t.lv_acc1 = 0.0f;
                }
                if (me >= 1 && me <= dl) {
                    const int i1 = me == 1 ? i : (i >> 2);
                    const float d1 = dl >= 2 ? lv_decide(c, 1, i1) : (float)t.leaf.cost; // (depth 1: the 16x16 leaf is final)
                    const float a0 = uni_f(t.lv_acc0 + d1);
                    t.lv_acc0 = a0;
                    if (i1 != 3) {
                        t.lv_i = (uint8_t)(i + 1);
                        cont = T_LV_UNIT;
                        break;
                    }
                    if (me == 1) lv_post_split(0, a0);
                }
                t.ret = lv_decide(c, 0, 0);
                t.level = 0;
                cont = T_RETURN;
                break;
            }
            }
            break;
        case T_LV_SERVE: {
            if constexpr (TEAM) {
                // Member 0 between its 32x32 candidate and the CTU's decision: pack {planar, DC} of member 2's 8x8 leaves
                // (K_SERVE8) and of member 3's 4x4 luma leaves (K_SERVE4), one job at a time: wait for a job or for "no more jobs", wait until the
                // previous job's results have been taken, run it.
                if (LANE == 0) SHT.lvb.srv_ready = 1;
                const bool two = D3 && t.max_depth == 3; // member 3 posts jobs too
                const unsigned served8 = uni((int)lv_word(&SHT.lvb.job_done)), served4 = uni((int)lv_word(&SHT.lvb.job4_done));
                int what = 0; // 1: a job of member 2, 3: of member 3, 2: both are through
                if (LANE == 0) {
                    int polls = 0;
                    for (;;) {
                        const unsigned p8 = lv_word(&SHT.lvb.job_posted), p4 = lv_word(&SHT.lvb.job4_posted);
                        if (two && p4 > served4) { // (the shorter job first: member 3's level is the longer one)
                            what = 3;
                            break;
                        }
                        if (p8 > served8) {
                            what = 1;
                            break;
                        }
                        if (lv_word(&SHT.lvb.job_fin) != 0 && (!two || lv_word(&SHT.lvb.job4_fin) != 0) &&
                            lv_word(&SHT.lvb.job_posted) == served8 && lv_word(&SHT.lvb.job4_posted) == served4) {
                            what = 2;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                        if (++polls > (1 << 23)) {
                            SHT.lvb.pad_ = 1;
                            what = 2;
                            break;
                        }
                    }
                }
                what = uni(what);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (what == 2) {
                    t.lv_i = 1;
                    cont = T_LV_UP;
                    break;
                }
                if (what == 3) {
                    lv_word_wait(&SHT.lvb.job4_ack, served4); // the previous results have been taken
                    req_full(q, 1, uni((int)SHT.lvb.job4_bx), uni((int)SHT.lvb.job4_by), 2, 0, 0, true, false, false, false);
                    q.kind = K_SERVE4;
                    q.stage = 0;
                    q.tree = TREE_DUAL_LUMA;
                    t.cont = T_LV_SERVE;
                    return true;
                }
                lv_word_wait(&SHT.lvb.job_ack, served8); // the previous job's reconstructions are still in this wave's park
                req_full(q, 3, uni((int)SHT.lvb.job_bx), uni((int)SHT.lvb.job_by), 3, 0, 0, true, false, false, false);
                q.kind = K_SERVE8;
                q.stage = 0;
                q.tree = TREE_SINGLE;
                t.cont = T_LV_SERVE;
                return true;
            }
            }
            break;
        // ---- final pass (ctu_encoder.rs:1421-1461): coding order = z-order over the 4x4 units; a
        // CU is emitted at its top-left unit (luma TB, then the chroma TBs) ----
        case T_FINAL_Z: {
            const int z = t.z;
            if (z >= t.zend) {
                t.cont = T_START;
                return false;
            }
            const int bx = 4 * ((z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4));
            const int by = 4 * (((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4));
            const int lg = uni((int)SH.cu_log2[(by >> 2) * 8 + (bx >> 2)]);
            t.bx = (uint8_t)bx;
            t.by = (uint8_t)by;
            t.lg = (uint8_t)lg;
            if ((bx & ((1 << lg) - 1)) == 0 && (by & ((1 << lg) - 1)) == 0) {
                const int ml = uni((int)SH.luma_mode[(by >> 2) * 8 + (bx >> 2)]);
                const int mc = uni((int)SH.chroma_mode[(by >> 3) * 4 + (bx >> 3)]);
                req_full(q, lg >= 3 ? 3 : 1, bx, by, lg, ml, mc, true, true, true, true);
                t.cont = T_FZ_TAIL;
                return true;
            }
            cont = T_FZ_NEXT;
            break;
        }
        case T_FZ_TAIL: {
            const int bx = t.bx, by = t.by;
            if (t.lg == 2 && (t.z & 3) == 3) { // after the fourth 4x4 luma CU: the 8x8's chroma CU
                req_full(q, 2, bx & ~7, by & ~7, 3, 0, uni((int)SH.chroma_mode[(by >> 3) * 4 + (bx >> 3)]), true,
                         true, true, true);
                t.cont = T_FZ_NEXT;
                return true;
            }
            cont = T_FZ_NEXT;
            break;
        }
        default: { // T_FZ_NEXT: on to the next CU (a CU of 2^lg samples a side covers 4^(lg - 2) units of the z-order)
            const int lgz = t.lg;
            t.z = (uint8_t)(t.z + (lgz <= 2 ? 1 : (1 << (2 * (lgz - 2)))));
            cont = T_FINAL_Z;
            break;
        }
        }
    }
}

// ---------------------------------------------------------------------------
// CTU entry: load, search, final pass, store
// ---------------------------------------------------------------------------
__device__ __forceinline__ void load_tables(Ctx c) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        SHT.ldq[i] = (int32_t)c.k->ldq[i];
        SHT.lv[i] = (int32_t)c.k->lv[i];
    }
    for (int i = threadIdx.x; i < 128; i += blockDim.x) ((int8_t*)SHT.fc)[i] = ((const CONST_AS int8_t*)c.k->fc)[i];
    if (threadIdx.x < 6) (&SHT.lvb.cnt[0][0])[threadIdx.x] = 0; // level schedule: the meeting points of this CTU's decisions
    if (threadIdx.x == 0) SHT.lvb.pad_ = 0;
    if (threadIdx.x < 9) (&SHT.lvb.srv_ready)[threadIdx.x] = 0;
    __syncthreads();
}


template <bool TEAM, bool D3>
__device__ __forceinline__ void encode_ctu(Ctx& c, const PicBufs& pb, int ctu_col, int ctu_row, int* overflow) {
    const CONST_AS DevConst* k = c.k;
    const int W = k->W;
    const int Wc = W >> 1;
    c.ctu_x = ctu_col * 32;
    c.ctu_y = ctu_row * 32;
    c.cu32_mode = PLANAR;
#ifdef WRENC_PROFILE
    for (int i = threadIdx.x; i < PH_COUNT; i += blockDim.x) s_prof[i] = 0;
    __syncthreads();
#endif
    PROF_MARK(tt0_);
    load_tables(c);
    GLOBAL_AS uint8_t* const rec = AS_GLOBAL(uint8_t, pb.rec[0]);
    // neighbour border of the reconstruction: row -1 (x = -4..67) and columns -4..-1
    for (int i = LANE; i < 72; i += 64) {
        const int gx = c.ctu_x - 4 + i, gy = c.ctu_y - 1;
        SH.recYtop[i] = (gx >= 0 && gx < W && gy >= 0) ? rec[(size_t)gy * W + gx] : 0;
    }
    // columns -4..-1 and the left CTU's modes: two cache lines of the left CTU's border record instead of 64
    // row pieces of the planes (lane = dword: 32 luma rows, 16 + 16 chroma rows, 2 dwords of modes)
    GLOBAL_AS uint8_t* const my_border =
        AS_GLOBAL(uint8_t, pb.border) + (size_t)(ctu_row * k->ctu_cols + ctu_col) * kBorderBytes;
    {
        const uint32_t v = (c.ctu_x > 0 && LANE < 66) ? ((const GLOBAL_AS uint32_t*)(my_border - kBorderBytes))[LANE] : 0u;
        const uint32_t v2 = (c.ctu_x > 0 && LANE < 2) ? ((const GLOBAL_AS uint32_t*)(my_border - kBorderBytes))[64 + LANE] : 0u;
        if (LANE < 32)
            *(uint32_t*)&SH.recY[LANE * 36] = v;
        else if (LANE < 48)
            *(uint32_t*)&SH.recC[0][(LANE - 32) * 20] = v;
        else
            *(uint32_t*)&SH.recC[1][(LANE - 48) * 20] = v;
        if (LANE < 2) *(uint32_t*)&SH.left_mode[4 * LANE] = v2;
    }
    for (int comp = 1; comp < 3; ++comp)
        for (int i = LANE; i < 40; i += 64) {
            const int gx = (c.ctu_x >> 1) - 4 + i, gy = (c.ctu_y >> 1) - 1;
            SH.recCtop[comp - 1][i] = (gx >= 0 && gx < Wc && gy >= 0) ? rec[plane_off(c, comp) + (size_t)gy * Wc + gx] : 0;
        }
    // tile.rs:49-58: planes start at zero
    for (int i = LANE; i < 32 * 32; i += 64) SH.recY[(i >> 5) * 36 + (i & 31) + 4] = 0;
    for (int comp = 1; comp < 3; ++comp)
        for (int i = LANE; i < 256; i += 64) SH.recC[comp - 1][(i >> 4) * 20 + (i & 15) + 4] = 0;
    WSYNC();
    // ---- the search + final pass: one evaluator, driven by the state machine ----
    #ifndef WRENC_EXP_LDS_PAD
    // LDS is handed out in granules of 1280 bytes (measured: a workgroup of 32,480 bytes -- 672 more than today, for scan
    // tables -- fits the CU four times, not five: 520 -> 460 frames/s, gpurun_out/r3w/ab.log)
    static_assert((sizeof(Lds) * WPB + sizeof(LdsTab) + 1279) / 1280 * 1280 * kWorkgroupsPerCU <= 160 * 1024,
                  "kWorkgroupsPerCU workgroups must fit the CU's 160 KB of LDS");
#endif
    SH.st.cont = T_START;
    SH.st.in_leaf = 0;
    SH.st.pend = 0;
    SH.st.dp0 = 0;
    SH.st.xpar = 0;
    SH.st.lvmode = 0;
    SH.st.fz_on = 0;
    SH.st.max_depth = (uint8_t)k->max_depth;
    Res r = {};
    Req q = {};
    for (;;) {
#ifdef WRENC_PROFILE
        // control time by where the step starts: leaf continuation (0..19) or 20 + tree continuation
        const int cb_ = SH.st.in_leaf ? (int)SH.st.leaf.cont : 20 + (int)SH.st.cont;
#endif
        PROF_MARK(tc0_);
        const bool more = ctu_step<TEAM, D3>(c, r, q);
        PROF_MARK(tc1_);
        PROF_ADD2(PH_CTRL, tc0_, tc1_);
        PROF_ADDM(0, tc0_, tc1_);
        PROF_ADD2(PH_CB + (cb_ & 31), tc0_, tc1_);
        PROF_ADD2(PH_CBN + (cb_ & 31), 0, 1);
        PROF_ADD2(PH_NSTEP, 0, 1);
        PROF_ADD2(PH_NFULL, 0, (q.kind == K_FULL ? 1 : 0));
        if (!more) break;
        if (TEAM) { // a decided leaf's winner into every member's tile (team_defer_pull), before anything else
            const int dp = SH.st.dp0;
            if (dp) {
                const int dq = SH.st.dp1;
                SH.st.dp0 = 0;
                copy_block(c, COPY_PULL, (dp >> 1) & 3, 0, (dq & 7) << 2, (dq >> 3) << 2, (dp >> 5) + 2, (dp >> 3) & 3);
            }
        }
        if (q.final && !SH.st.fz_on) { // the first block of the final pass (the search no longer needs ns_cost / split_cost)
            SH.st.fz_on = 1;
            if (LANE < 4) {
                SH.lev_was[LANE] = AS_GLOBAL(uint32_t, pb.lev_dirty)[(size_t)(ctu_row * k->ctu_cols + ctu_col) * 4 + LANE];
                SH.lev_now[LANE] = 0;
            }
            WSYNC();
        }
#ifdef WRENC_EXP_CTRL_ONLY // timing / counting experiment only (wrong results): the control flow without evaluations
        r = Res{};
#else
        PROF_MARK(te0_);
        r = evaluate<TEAM, D3>(c, pb, q, overflow);
        PROF_MARK(te1_);
        PROF_ADDM(q.kind == K_NOP ? 3 : 1, te0_, te1_);
        PROF_ADD2(PH_EV + (((q.kind & 15) * 4 + ((q.kind == K_NOP ? q.copy_tlg : q.tlg) - 2)) & 63), te0_, te1_); // by request kind and block size
        PROF_ADD2(PH_EVN + (((q.kind & 15) * 4 + ((q.kind == K_NOP ? q.copy_tlg : q.tlg) - 2)) & 63), 0, 1);
#ifdef WRENC_PROFILE
        if (LANE == 0 && WAVE < 4 && cb_ < 12) s_prof[PH_ST + 4 * cb_ + WAVE] += te1_ - te0_; // eval time by step origin, member
        if (threadIdx.x == 0 && cb_ < 12) s_prof[PH_STN + cb_] += 1;
#endif
#endif
        if (TEAM && q.xchg) {
            // publish, meet the team (the workgroup's teams walk the same schedule: the same barriers), flip the
            // parity: a fast member's next result goes to the other buffer while slow members still read this one
            PROF_MARK(tx0_);
            const int par = SH.st.xpar;
            team_publish(q, r, par);
            SH.st.xpar = (uint8_t)(par ^ 1);
            __syncthreads();
            PROF_MARK(tx1_);
            PROF_ADD2(PH_XCHG, tx0_, tx1_);
            PROF_ADDM(2, tx0_, tx1_);
        }
    }
    const float cost = SH.st.ctu_cost;
    // which blocks of levels this encode left non-zero: the words of the quadrants whose CUs this wave emitted (wave
    // schedule: all four; a team member: its own, member 0 all four when the CTU is one 32x32 CU)
    // a team whose meeting point timed out (lv_meet) has made its decisions from half-posted costs: it stores nothing more
    // (the host reports WRENC_GPU_EHIP at the next sync / download and the context is to be destroyed, wrenc_gpu.h)
    const bool dead = TEAM && uni((int)SHT.lvb.pad_) != 0;
    if (c.store && SH.st.fz_on && !dead) {
        WSYNC();
        const bool all4 = !TEAM || uni((int)SH.cu_log2[0]) == 5;
        if (LANE < 4 && (all4 || LANE == c.member))
            AS_GLOBAL(uint32_t, pb.lev_dirty)[(size_t)(ctu_row * k->ctu_cols + ctu_col) * 4 + LANE] = SH.lev_now[LANE];
    }
    // store recon + decisions
    if (c.write && !dead) {
        for (int i = LANE; i < 1024 / 4; i += 64) {
            const int y = i >> 3, x4 = (i & 7) * 4;
            *(GLOBAL_AS uint32_t*)&rec[(size_t)(c.ctu_y + y) * W + c.ctu_x + x4] = *(const uint32_t*)&SH.recY[y * 36 + x4 + 4];
        }
        for (int comp = 1; comp < 3; ++comp)
            for (int i = LANE; i < 256 / 4; i += 64) {
                const int y = i >> 2, x4 = (i & 3) * 4;
                *(GLOBAL_AS uint32_t*)&rec[plane_off(c, comp) + (size_t)((c.ctu_y >> 1) + y) * Wc + (c.ctu_x >> 1) + x4] =
                    *(const uint32_t*)&SH.recC[comp - 1][y * 20 + x4 + 4];
            }
        const int i = LANE; // 64 4x4 units
        const size_t o = (size_t)((c.ctu_y >> 2) + (i >> 3)) * (W >> 2) + (c.ctu_x >> 2) + (i & 7);
        AS_GLOBAL(uint8_t, pb.cu_log2)[o] = SH.cu_log2[i];
        AS_GLOBAL(uint8_t, pb.luma_mode)[o] = SH.luma_mode[i];
        if (i < 16) {
            const size_t oc = (size_t)((c.ctu_y >> 3) + (i >> 2)) * (W >> 3) + (c.ctu_x >> 3) + (i & 3);
            AS_GLOBAL(uint8_t, pb.chroma_mode)[oc] = SH.chroma_mode[i];
        }
        if (i == 0) AS_GLOBAL(float, pb.ctu_cost)[ctu_row * k->ctu_cols + ctu_col] = cost;
        // the border record for the CTU to the right (see kBorderBytes)
        {
            uint32_t v;
            if (LANE < 32)
                v = *(const uint32_t*)&SH.recY[LANE * 36 + 32];
            else if (LANE < 48)
                v = *(const uint32_t*)&SH.recC[0][(LANE - 32) * 20 + 16];
            else
                v = *(const uint32_t*)&SH.recC[1][(LANE - 48) * 20 + 16];
            ((GLOBAL_AS uint32_t*)my_border)[LANE] = v;
            if (LANE < 2) {
                const int r0 = 4 * LANE; // modes of the 4x4 units (7, r0 .. r0 + 3)
                ((GLOBAL_AS uint32_t*)my_border)[64 + LANE] =
                    (uint32_t)SH.luma_mode[r0 * 8 + 7] | ((uint32_t)SH.luma_mode[(r0 + 1) * 8 + 7] << 8) |
                    ((uint32_t)SH.luma_mode[(r0 + 2) * 8 + 7] << 16) | ((uint32_t)SH.luma_mode[(r0 + 3) * 8 + 7] << 24);
            }
        }
    }
#ifdef WRENC_PROFILE
    PROF_MARK(tt1_);
    PROF_ADD2(PH_TOTAL, tt0_, tt1_);
    if (threadIdx.x == 0) s_prof[PH_HIST + (int)min((unsigned long long)63, (tt1_ - tt0_) >> 17)] += 1; // how long this CTU took (the launch waits for the slowest)
    __syncthreads();
    for (int i = threadIdx.x; i < PH_COUNT; i += blockDim.x) atomicAdd(&g_prof[i], s_prof[i]);
#endif
}

} // namespace wrenc
