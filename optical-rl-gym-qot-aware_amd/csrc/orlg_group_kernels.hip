// orlg_group_kernels.hip -- RMSA step kernel, FOUR ENVIRONMENTS PER WAVEFRONT (one 16-lane DPP row each).
//
// The wave-per-environment kernel (orlg_kernels.hip) is bound by instruction issue, and most of its instructions are
// wave-uniform control work done for one environment.  Here a wave steps four environments in lockstep: every scalar of an
// environment (clock, pending request, counters, running sums) lives in VGPRs replicated over its row, so one instruction does
// that piece of bookkeeping for four environments, and the bitmap work maps onto the 16 lanes of a row:
//     (path, word) lanes   16 / W candidate paths per pass: AND of the link bitmaps; the first fit is found with a shift-and-AND
//                          doubling over the path's W words (the next word arrives by DPP row_shl:1), then one row minimum
//     (hop, word) lanes    provision / release of a slot window, 16 / W hops per pass
//     queue lanes          slot j * 16 + lane: lane-local minimum, then a row minimum of (time, slot)
//     (link, word) lanes   link statistics: 16 / W links per row and pass, reductions over a link's W lanes with DPP row_shl
// The rows diverge (accepted / blocked, number of releases, hops): every loop runs to the longest row and predicates the others.
// Reductions stay inside a row (full-mask DPP: quad_perm, row_half_mirror, row_mirror, row_shl), row-level votes come from
// one ballot shifted to the row's 16 bits.  The state format in HBM is the wave-per-environment kernel's: either kernel
// can continue a batch the other one stepped, and the reset kernel is shared (the host looks it up; this file does not include it).  The MT19937 state and the ring of pre-generated
// arrivals stay in HBM: a row reads its next arrival one step ahead, and a refill (every ~62 steps per environment) is done
// by the whole wave for one environment at a time through the workgroup's LDS staging buffer (refill_requests, orlg_requests.h).
// The wave's LDS region is array-major (four occupancy bitmaps, then four link-statistics blocks, ...: OrlgParams::g_occ ...),
// as four consecutive environments lie in the HBM arrays: a quad's state moves as linear copies by all 64 lanes.
//
// Policies: the first-fit family (shortest path / shortest available path, path-only agent actions), the DeepRMSA block family
// (its two heuristics and the agent's (path, block) action), load balancing (llp_ff) and external (path, slot) actions.  Reference: the same lines of rmsa_env.py as orlg_kernels.hip cites.
#pragma once
#include "orlg_link_stats.h"   // and through it orlg_wave.h, orlg_rmsa_layout.h, orlg_spectrum.h
#include "orlg_requests.h"
#include "orlg_sections.h"
#include "orlg_block_cause.h"  // window_level: the classifier of the CAUSE instantiations (group_fit_level below)
#include "orlg_assign.h"       // assign_word_key: the assignment rules of the ASSIGN instantiations
#include "orlg_cut.h"          // cut_word_key: the fewest-cuts window of the CUT instantiations
#include "orlg_usage.h"        // usage_prefix, window_word_key: the rule MOST_USED and the route BEST_WINDOW of the USAGE instantiations
#include "orlg_graph_log.h"    // OrlgGraphEntry, orlg_glog_*: the lean body's logged graph statistics (group_graph_replay below)
#include "orlg_link_summary.h" // lsum_pack, lsum_unpack, orlg_lsum_provision: a link's summary of the DEFER instantiations

#define ORLG_GL 16  // lanes per environment (one DPP row)
#define ORLG_GE 4   // environments per wave
#define ORLG_LEAN_FLUSH_STEPS 0x8000   // the lean body's packed bit-rate counts (orlg_group_body.h, LANE_HIST) go to memory at least this often

DEV int row_add_i32(int v) { v += dpp_xor1(v); v += dpp_xor2(v); v += dpp_half_mirror(v); v += dpp_row_mirror(v); return v; }
// ... of 64-bit terms (the lean body's flushes: cold)
#define ORLG_DPP_I64(fn, x) (long long)(((u64)(uint32_t)fn((int)((u64)(x) >> 32)) << 32) | (uint32_t)fn((int)(uint32_t)(x)))
DEV long long row_add_i64(long long v) {
    v += ORLG_DPP_I64(dpp_xor1, v); v += ORLG_DPP_I64(dpp_xor2, v); v += ORLG_DPP_I64(dpp_half_mirror, v); v += ORLG_DPP_I64(dpp_row_mirror, v);
    return v;
}
// the value of the lane eight places away in the row (row_ror:8): a row's two halves trade places
DEV int row_swap8_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false); }
// OR over the eight lanes of a half row, on every lane of it
DEV u64 half_row_or_u64(u64 v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo |= (uint32_t)dpp_xor1((int)lo); hi |= (uint32_t)dpp_xor1((int)hi);
    lo |= (uint32_t)dpp_xor2((int)lo); hi |= (uint32_t)dpp_xor2((int)hi);
    lo |= (uint32_t)dpp_half_mirror((int)lo); hi |= (uint32_t)dpp_half_mirror((int)hi);
    return ((u64)hi << 32) | lo;
}
DEV int row_min_i32(int v) {
    int o = dpp_xor1(v); v = o < v ? o : v;
    o = dpp_xor2(v); v = o < v ? o : v;
    o = dpp_half_mirror(v); v = o < v ? o : v;
    o = dpp_row_mirror(v); return o < v ? o : v;
}
// votes of the lane's own row (16 bits)
DEV uint32_t row_ballot(bool p, int lane) { return (uint32_t)(ballot(p) >> (lane & 48)) & 0xffffu; }

// Reductions over the W consecutive lanes that hold one link's words (W is not a power of two in general: 16 / W links share a
// row): the link's FIRST lane ends with the link's result (the other lanes hold partial results nobody reads).  Sums and
// unsigned maxima only: a source past the row's end reads as 0 (bound_ctrl), their identity, so that every step is ONE
// instruction (v_add_u32_dpp / v_max_u32_dpp); a doubling tree: lanes i, i+1 -> i .. i+3 -> the rest.
#define ORLG_SEG_REDUCE(name, OP)                                                                   \
    template <int W>                                                                                \
    DEV uint32_t name(uint32_t v) {                                                                 \
        static_assert(W >= 1 && W <= 8 && W != 7, "words per link");                                \
        if (W == 1) return v;                                                                       \
        uint32_t o = (uint32_t)lane_ahead_i32<1>((int)v);                                           \
        const uint32_t s = OP(v, o);                                   /* lanes i, i+1 */           \
        if (W == 2) return s;                                                                       \
        o = (uint32_t)lane_ahead_i32<2>((int)(W == 3 ? v : s));                                     \
        const uint32_t t = OP(s, o);                                   /* lanes i .. i+2 / i+3 */   \
        if (W <= 4) return t;                                                                       \
        o = (uint32_t)lane_ahead_i32<4>((int)(W == 5 ? v : (W == 6 ? s : t)));                      \
        return OP(t, o);                                               /* lanes i .. i+W-1 */       \
    }
#define ORLG_OP_ADD(a, b) ((a) + (b))
#define ORLG_OP_MAX(a, b) ((a) > (b) ? (a) : (b))
ORLG_SEG_REDUCE(seg_add, ORLG_OP_ADD)
ORLG_SEG_REDUCE(seg_max, ORLG_OP_MAX)
#undef ORLG_SEG_REDUCE

// path_word_rec (orlg_spectrum.h) with the hop words FOUR TO A WAIT: the record's link bytes are all in registers, so the reads of
// a group of four hops are issued back to back and ANDed in after one round trip, where the other form waits for every hop's
// word before it votes on the next (three waves per SIMD do not hide that chain here; the wave kernel, at four, keeps its own
// form).  No hop is tested against the path's end: every link byte of the record is read as it stands and its word ANDed in.
// The host pads the bytes past the end with the path's first link (OrlgPathRec, orlg_device.h) and AND is idempotent, so a
// hop past the end repeats a word the result already holds; its address is a link of the path, valid on every lane.  An
// inactive lane keeps a zero record: it reads link 0, starts from acc = 0 and returns 0 with se = hops = 0, as there.
// group_path_word_of: the same from a record the caller holds in registers (the later first-fit passes of the lean body
// load it for group_path_candidate below and hand it on); an inactive lane passes a record whose first word is zero.
template <int W>
DEV u64 group_path_word_of(const u64 *occ, const uint4 r, int w, bool active, int &se, int &hops_out) {
    const uint32_t q[4] = {r.x, r.y, r.z, r.w};
    const int hops = (int)(r.x & 0xffu);
    se = (int)((r.x >> 8) & 0xffu);
    hops_out = hops;
    u64 acc = active ? ~0ull : 0ull;
#pragma unroll
    for (int h0 = 0; h0 < ORLG_MAX_HOPS; h0 += 4) {
        if (ballot(h0 < hops) == 0ull) break;
        u64 v[4] = {~0ull, ~0ull, ~0ull, ~0ull};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int h = h0 + k;
            if (h < ORLG_MAX_HOPS) {
                const int link = (int)((q[(h + 2) >> 2] >> (8 * ((h + 2) & 3))) & 0xffu);
                v[k] = occ[__mul24(link, W) + w];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc &= v[k];
    }
    return acc;
}
template <int W>
DEV u64 group_path_word_rec(const u64 *occ, const OrlgPathRec *recs, int gid, int w, bool active, int &se, int &hops_out) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (active) r = *reinterpret_cast<const uint4 *>(recs + gid);
    return group_path_word_of<W>(occ, r, w, active, se, hops_out);
}

// Byte i (0 .. 15, lane-variable) of a path record held in registers: hops, se, link[0 .. 13] (OrlgPathRec).  Two selects pick the
// record's half, one 64-bit shift the byte.
DEV int group_rec_byte(const uint4 r, int i) {
    const u64 half = ((u64)((i & 8) ? r.w : r.y) << 32) | ((i & 8) ? r.z : r.x);
    return (int)((half >> (8 * (i & 7))) & 0xffull);
}

// The longest-run test of a first-fit pass after the first (the lean body of the DEFER instantiations).  A
// path can hold a window of n slots only if every one of its links has a free run of n, and a link's summary holds its longest
// free run ml -- exact after every provision (the statistics pass recomputes it), every release (max(ml, L + n + R)) and every
// state load.  The pass's own layout: lane (ps, w) of path record gid tests hops w, w + W, w + 2 W, ... -- a byte of the record
// and the high half of that link's summary per hop -- and the path's W lanes learn the outcome from one row vote.
// Straight-line code, two LDS round trips: the record and the lane's link bytes, then the slot count and the summaries.  So
// nothing is tested against the path's end or against `on`, knowingly: a byte past the path's end repeats the path's first link
// (OrlgPathRec, orlg_device.h), whose outcome the vote holds already; a hop index past the record's last byte is clamped to that
// byte (a link of the path, or the padding); and a lane that is not on reads record gid0, which every lane may read (the
// first candidate of the row's request), and does not vote.
// Returns the lane's `on` for the pass: on, and no link of its path rules the window out.  rec: the path's record for
// group_path_word_of (its first word zero where the result is false); n: the path's slot count, 1 where the result is false
// (run_starts' doubling loop runs to the largest n of the wave: a lane that does not look must not lengthen it).  The vote stands outside every
// condition (row_ballot).
template <int W>
DEV bool group_path_candidate(const int lane, const u64 *lsum, const Tab &tb, int gid, int gid0, int w, bool on, int br, uint4 &rec, int &n) {
    constexpr int NH = (ORLG_MAX_HOPS + W - 1) / W;   // hops per lane at most
    const uint32_t *sum_hi = reinterpret_cast<const uint32_t *>(lsum) + 1;
    const OrlgPathRec *pr = tb.recs + (on ? gid : gid0);
    uint4 r = *reinterpret_cast<const uint4 *>(pr);
    int lk[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        int h = w + j * W;
        if ((j + 1) * W > ORLG_MAX_HOPS) h = h < ORLG_MAX_HOPS - 1 ? h : ORLG_MAX_HOPS - 1;   // (the last group only)
        lk[j] = (int)pr->link[h];
    }
    n = tb.nslots[br * ORLG_NSLOT_STRIDE + (int)((r.x >> 8) & 0xffu)];
    uint32_t ml = 0x3ffu;   // the shortest of the longest runs of the lane's hops
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        const uint32_t m = (sum_hi[2 * lk[j]] >> 20) & 0x3ffu;
        ml = m < ml ? m : ml;
    }
    const uint32_t bad = row_ballot(on && (int)ml < n, lane);
    const uint32_t mine = ((1u << W) - 1u) << ((lane & 15) - w);   // the lanes of this lane's path
    const bool ok = on && (bad & mine) == 0u;
    r.x = ok ? r.x : 0u;
    n = ok ? n : 1;   // (a lane that is not on must not lengthen run_starts for the others)
    rec = r;
    return ok;
}

// link statistics of up to ORLG_MAX_HOPS links per row: link_stats_update (orlg_link_stats.h) with 16 / W links per row and
// pass, one word per lane; nlinks = 0 for a row that does not take part.  links: the row's link indices (bytes, LDS).
// DEFER: the float64 part of _update_link_stats is not done here.  It is a recurrence PER LINK -- the time-weighted means of
// utilization, external fragmentation and compactness since the link's last update -- of ~100 instructions that every lane of
// the row executes for the one to three links a pass holds: 29 % of this kernel's instructions.  The deferred form logs what
// the recurrence consumes (the integers behind cur0..2 and the time: 16 bytes) per (environment, link) in HBM, counts the
// entries in the upper bits of the link's span cache, and group_link_replay works the logs off with ONE LINK PER LANE, sixteen
// links of an environment at a time, every lane through its own link's events in their order -- the same operations on the
// same values, so the same bits.
// SUM (DEFER): 1 = also write each link's summary (lsum_pack) to lsum[link]; 2 = ONLY that, for links 0 .. nlinks - 1 (links is
// not read): the summaries of a quad whose state was just loaded, without a log entry, span cache or running sum touched.
// APPLY: the pass of a provision clears the window [win_s, win_s + win_n) on its links itself (the lane layout is
// group_apply_window's: a link's word w on one lane, and a path never repeats a link, so no word is touched twice in a launch of
// the pass): the word is cleared in the register it was read into, stored back where the window reaches it, and everything
// after -- the neighbours' DPP reads included -- sees the cleared words.  No write pass of its own, no second read.
// PART: sum_span and sum_gaps are LANE PARTIALS of the row's two sums (the lean body, orlg_group_body.h): a link lane adds its own
// link's differences to its own registers and the pass joins nothing over the row -- integer sums, formed where they are read.
// FROMSUM (the lean body's pass at a provision): the window was WHOLLY FREE on every link of the pass (a first fit's window on an
// accepted row) and the link's summary is exact, so the rescan produces the longest free run alone -- the one integer that does
// not follow from the summary (65 % of the updates cut a longest run: DESIGN 2.5, rounds 4 and 15).  A word lane reads its word,
// clears the window, hands `prev` on and runs the lead / e chain, fstarts and the run loop for seg_max(ml); the used runs, the
// popcounts, the first / last used slot, slot S - 1 and their three segment reductions are not computed.  The link lane reads
// the old summary and the two words that hold slot win_s - 1 and slot win_s + win_n -- with the pass's first reads, on every
// lane and outside every condition: the indices are words of the lane's link whatever the lane's window says, and a lane that
// is not on reads link 0 -- and orlg_lsum_provision (orlg_link_summary.h) gives the other seven.  The same values as the rescan,
// so the same bits in the summary, the log entry, the span cache and the two sums.
template <int W, bool LINKF, bool GRAPH, bool DEFER = false, int SUM = 0, bool APPLY = false, bool PART = false, bool FROMSUM = false>
DEV void group_link_stats(const int lane, u64 *occ, double *lst, int32_t *lint, const Tab &tb, int S, int E, const uint8_t *links,
                          int nlinks, double now, int &sum_span, int &sum_gaps, double &comp_cur, int sum_sh, double cur_thr,
                          double &g_thr, double &g_comp, double &g_lu, uint4 *llog = nullptr, bool *need_replay = nullptr,
                          u64 *lsum = nullptr, int win_s = 0, int win_n = 0) {
    static_assert(W <= 8, "at least two links per row");
    static_assert(!APPLY || SUM != 2, "the summary rebuild changes no occupancy");
    static_assert(SUM == 0 || (LINKF && DEFER && (SUM == 1 || !GRAPH)), "summaries belong to the deferred instantiation");
    static_assert(!FROMSUM || (SUM == 1 && APPLY), "the statistics follow from the summary where the pass clears a free window");
    constexpr int NS = ORLG_GL / W;  // links per row and pass
    const int gl = lane & 15;
    const int sl = gl / W, w = gl - sl * W;
    double ynow = 0.0;
    if ((LINKF || GRAPH) && nlinks > 0 && now > 0) ynow = recip_refine(now);
    for (int h0 = 0;; h0 += NS) {
        if (ballot(h0 < nlinks) == 0ull) break;
        const int h = h0 + sl;
        const bool on = sl < NS && h < nlinks;
        int link = 0;
        uint32_t packed = 0u, ilo = 0u, hi = 0u, ml = 0u;   // ilo = 0x7fff - first used slot (0: none): the minimum taken as a maximum
        if (on) link = SUM == 2 ? h : (int)links[h];
        // the link's words sit on consecutive lanes: the neighbours' words arrive by DPP instead of further LDS reads
        u64 x = 0ull;
        if (on) x = occ[__mul24(link, W) + w];
        [[maybe_unused]] u64 old_sum = 0ull, x_below = 0ull, x_above = 0ull;
        if constexpr (FROMSUM) {
            old_sum = lsum[link];
            x_below = occ[__mul24(link, W) + orlg_lsum_word_below(S, win_s)];
            x_above = occ[__mul24(link, W) + orlg_lsum_word_above(S, win_s + win_n)];
        }
        if (APPLY && on) {
            const u64 m = window_mask(win_s, win_n, w);
            x &= ~m;
            if (m) occ[__mul24(link, W) + w] = x;
        }
        const u64 prev = lane_prev_u64(x);
        int e = 0;  // free slots that continue a run reaching this word's end into the next words
        if (LINKF) {
            const int lead = x == ~0ull ? 64 : ctz64(~x);  // free slots at the word's start
            // (the DPP reads stand outside any condition: a lane switched off by a branch is not a readable source)
            const int nlead_raw = lane_next_i32(lead);
            const int nlead = w < W - 1 ? nlead_raw : 0;
            e = nlead;
#pragma unroll
            for (int i = 0; i < W - 2; ++i) {
                const int ne_raw = lane_next_i32(e);
                const int ne = w < W - 1 ? ne_raw : 0;
                e = nlead == 64 ? 64 + ne : nlead;
            }
        }
        bool first_free = false, last_free = false;
        if constexpr (!FROMSUM) {
            first_free = x & 1ull;                                                            // meaningful on w == 0
            // slot S - 1 sits in word (S - 1) >> 6 -- not always the last of the W words (S = 400 runs on the 8-word layout)
            const uint32_t last_free_bit = w == ((S - 1) >> 6) ? (uint32_t)((x >> ((S - 1) & 63)) & 1ull) : 0u;
            // ... on the link's first lane: slot S - 1 sits in the link's last word or in the one before it (W = ceil(S / 64), 8 for 7)
            uint32_t lf = last_free_bit;
            if (W > 1) lf |= (uint32_t)lane_ahead_i32<(W > 1 ? W - 1 : 1)>((int)last_free_bit);
            if (W > 2) lf |= (uint32_t)lane_ahead_i32<(W > 2 ? W - 2 : 1)>((int)last_free_bit);
            last_free = lf != 0u;
        }
        if (on) {
            u64 carry_f = w > 0 ? (prev >> 63) : 0ull;
            u64 fstarts = x & ~((x << 1) | carry_f);
            if constexpr (!FROMSUM) {
                u64 u = ~x & valid_mask(S, w);
                u64 carry_u = w > 0 ? ((~prev) >> 63) : 0ull;
                u64 ustarts = u & ~((u << 1) | carry_u);
                packed = (uint32_t)(popc64(x) | (popc64(fstarts) << 10) | (popc64(ustarts) << 20));  // free slots, free runs, used runs
                ilo = u ? (uint32_t)(0x7fff - (64 * w + ctz64(u))) : 0u;
                hi = u ? (uint32_t)(64 * w + 64 - clz64(u)) : 0u;
            }
            if (LINKF) {
                u64 st = fstarts;
                while (st) {
                    int b = ctz64(st);
                    st &= st - 1;
                    const uint32_t len = (uint32_t)free_run_length((~x) >> b, 64 - b + e);
                    ml = len > ml ? len : ml;
                }
            }
        }
        int freec, F, U, lmin, lmax;
        if constexpr (FROMSUM) {
            ml = seg_max<W>(ml);
            const int win_e = win_s + win_n;
            const OrlgLinkSummary r = orlg_lsum_provision(lsum_unpack(old_sum), S, win_s, win_n, orlg_lsum_free_below(x_below, S, win_s),
                                                          orlg_lsum_free_above(x_above, S, win_e), (int)ml);
            freec = r.freec, F = r.F, U = r.U, lmin = r.lmin, lmax = r.lmax, first_free = r.ff, last_free = r.lf;
        } else {
            packed = seg_add<W>(packed);
            lmin = 0x7fff - (int)seg_max<W>(ilo), lmax = (int)seg_max<W>(hi);
            if (LINKF) ml = seg_max<W>(ml);
            freec = (int)(packed & 0x3ff), F = (int)((packed >> 10) & 0x3ff), U = (int)(packed >> 20);
        }
        const bool link_lane = on && w == 0;  // one lane per link carries on
        if (SUM != 0 && link_lane) lsum[link] = lsum_pack(freec, F, U, lmin, lmax, (int)ml, first_free, last_free);
        if (SUM == 2) { wave_sync(); continue; }
        int dspan = 0, dgaps = 0;
        if (link_lane) {
            int nspan = U > 1 ? lmax - lmin : 0, ngaps = U > 1 ? U - 1 : 0;
            int old = lint[link];
            int cnt = 0;
            if (LINKF && DEFER) {
                // the update's inputs, for group_link_replay: free slots, max_empty, span, used runs | the time
                cnt = (int)((uint32_t)old >> 26);
                const int max_empty = (F > 1 && !(F == 2 && first_free && last_free)) ? (int)ml : 0;
                if (cnt < ORLG_LLOG_CAP - 1) {
                    llog[__mul24(link, ORLG_LLOG_CAP) + cnt] =
                        make_uint4((uint32_t)freec | ((uint32_t)max_empty << 10) | ((uint32_t)(lmax - lmin) << 20), (uint32_t)U,
                                   (uint32_t)__double2loint(now), (uint32_t)__double2hiint(now));
                    cnt += 1;
                }
                if (cnt >= ORLG_LLOG_FLUSH) *need_replay = true;
                old &= 0x03ffffff;
            }
            lint[link] = nspan | (ngaps << 16) | (cnt << 26);
            dspan = nspan - (old & 0xffff);
            dgaps = ngaps - (old >> 16);
        }
        if constexpr (PART) {
            sum_span += dspan;
            sum_gaps += dgaps;
        } else {
            sum_span += row_add_i32(dspan);
            sum_gaps += row_add_i32(dgaps);
        }
        if (LINKF && !DEFER && link_lane && now > 0) {
            double *l_util = lst, *l_ef = lst + E, *l_c = lst + 2 * E, *l_lu = lst + 3 * E;
            const double last_update = l_lu[link];
            const double last0 = l_util[link], last1 = l_ef[link], last2 = l_c[link];
            const double cur0 = tb.div_s[S - freec];  // (S - free) / S
            double cur1 = 0.0, cur2 = 0.0;
            if (freec > 0) {
                int max_empty = (F > 1 && !(F == 2 && first_free && last_free)) ? (int)ml : 0;
                cur1 = 1.0 - ORLG_FDIV((double)max_empty, (double)freec);
                cur2 = U > 1 ? ORLG_FDIV((double)(lmax - lmin), (double)(S - freec)) * tb.inv_k[U] : 1.0;
            }
            const double time_diff = now - last_update;
            l_util[link] = div_by((last0 * last_update) + (cur0 * time_diff), now, ynow);
            l_ef[link] = div_by((last1 * last_update) + (cur1 * time_diff), now, ynow);
            l_c[link] = div_by((last2 * last_update) + (cur2 * time_diff), now, ynow);
        }
        if (LINKF && !DEFER && link_lane) lst[3 * E + link] = now;
        wave_sync();
    }
    if (GRAPH && SUM != 2 && nlinks > 0) {
        // _update_network_stats (rmsa_env.py:537-560), on every lane of the row
        comp_cur = network_compactness(sum_span, sum_sh, sum_gaps, E);
        if (now > 0) {
            const double time_diff = now - g_lu;
            g_thr = div_by((g_thr * g_lu) + (cur_thr * time_diff), now, ynow);
            g_comp = div_by((g_comp * g_lu) + (comp_cur * time_diff), now, ynow);
        }
        g_lu = now;
    }
}

// Release of the window [s, s+n) on the row's path (DEFER instantiation): group_apply_window + group_link_stats in ONE pass, lane
// = hop.  The window was wholly in use, so every integer of the link's statistics follows from its summary and the free runs
// that border the window -- L slots ending at s - 1, R slots starting at s + n: free slots + n, free runs + 1 - [L > 0] - [R > 0],
// used runs + [slot s - 1 used] + [slot s + n used] - 1, longest free run max(ml, L + n + R) (a release never shortens it), the
// first / last used slot move only where the window was one, slot 0 / S - 1 are free once the window held them.  The lane reads
// the words next to and under the window at once (independent LDS reads), ORs the window into the one or two words it covers,
// looks further out only where a bordering free run reaches a word's end, then logs the update and refreshes the span cache
// exactly as group_link_stats would (the same values, so the same bits).
// The lane's hop is its own: hop `hop` of a path of `hops` (none: hops = 0) over link `link` (the caller holds the path's record in
// registers; read only where hop < hops), with that path's window.  A row that releases one
// service has hop = the lane's place in the row; a row that releases two link-disjoint services at once (orlg_group_body.h) gives
// its lower eight lanes the first one's hops and its upper eight the second one's, and the row sums below cover both.
// PART: sum_span and sum_gaps are lane partials, as in group_link_stats: every hop lane adds its own link's differences.
template <int W, bool PART = false>
DEV void group_release_links(const int lane, u64 *occ, u64 *lsum, int32_t *lint, int S, const int link, int hop, int hops, int s,
                             int n, double now, int &sum_span, int &sum_gaps, uint4 *llog, bool &need_replay) {
    static_assert(ORLG_MAX_HOPS <= ORLG_GL, "one lane per hop");
    int dspan = 0, dgaps = 0;
    if (hop < hops) {
        u64 *lw = occ + __mul24(link, W);
        const int e = s + n;
        // the words that hold slot s - 1, slot s + n, and the window's first / last slot: independent reads (coinciding ones too)
        const int ia = s > 0 ? (s - 1) >> 6 : 0, ib = e < S ? e >> 6 : 0, ws = s >> 6, we = (e - 1) >> 6;
        const u64 xa = lw[ia], xb = lw[ib], xs = lw[ws], xe = lw[we];
        const u64 sm = lsum[link];
        // the window's bits (a window wider than 64 slots fills the words between its first and last one)
        const u64 hm = ~0ull << (s & 63), lm = ~0ull >> (63 - ((e - 1) & 63));
        if (ws == we) {
            lw[ws] = xs | (hm & lm);
        } else {
            lw[ws] = xs | hm;
            for (int j = ws + 1; j < we; ++j) lw[j] = ~0ull;
            lw[we] = xe | lm;
        }
        // p = the last used slot below s (none: -1), q = the first slot from s + n on that is not free (none: 64 W; slots >= S
        // are stored as not free, so q <= S): in the word next to the window, else further out word by word (rarely more than one)
        int p = -1, q = 64 * W;
        if (s > 0) {
            const u64 y = ~xa & (~0ull >> (63 - ((s - 1) & 63)));
            if (y) p = 64 * ia + 63 - clz64(y);
            else
                for (int j = ia - 1; j >= 0; --j) {
                    const u64 v = ~lw[j];
                    if (v) { p = 64 * j + 63 - clz64(v); break; }
                }
        }
        if (e < S) {
            const u64 y = ~xb & (~0ull << (e & 63));
            if (y) q = 64 * ib + ctz64(y);
            else
                for (int j = ib + 1; j < W; ++j) {
                    const u64 v = ~lw[j];
                    if (v) { q = 64 * j + ctz64(v); break; }
                }
        } else {
            q = e;
        }
        const int L = s - 1 - p, R = q - e;
        const uint32_t lo32 = (uint32_t)sm, hi32 = (uint32_t)(sm >> 32);
        const int freec = (int)(lo32 & 0x3ff) + n;
        const int F = (int)((lo32 >> 10) & 0x3ff) + 1 - (L > 0) - (R > 0);
        const int U = (int)((lo32 >> 20) & 0x3ff) + (s > 0 && L == 0) + (e < S && R == 0) - 1;
        int lmin = (int)(hi32 & 0x3ff);   // (a window in use: U >= 1 before, lmin is a slot)
        int lmax = (int)((hi32 >> 10) & 0x3ff);
        int ml = (int)((hi32 >> 20) & 0x3ff);
        const bool ff = ((hi32 >> 30) & 1u) || s == 0, lf = (hi32 >> 31) || e == S;
        ml = L + n + R > ml ? L + n + R : ml;
        if (U == 0) { lmin = 0x7fff; lmax = 0; }
        else {
            if (lmin == s) lmin = e + R;
            if (lmax == e) lmax = s - L;
        }
        lsum[link] = lsum_pack(freec, F, U, lmin, lmax, ml, ff, lf);
        // group_link_stats' link lane from here on
        const int nspan = U > 1 ? lmax - lmin : 0, ngaps = U > 1 ? U - 1 : 0;
        int old = lint[link];
        int cnt = (int)((uint32_t)old >> 26);
        const int max_empty = (F > 1 && !(F == 2 && ff && lf)) ? ml : 0;
        if (cnt < ORLG_LLOG_CAP - 1) {
            llog[__mul24(link, ORLG_LLOG_CAP) + cnt] =
                make_uint4((uint32_t)freec | ((uint32_t)max_empty << 10) | ((uint32_t)(lmax - lmin) << 20), (uint32_t)U,
                           (uint32_t)__double2loint(now), (uint32_t)__double2hiint(now));
            cnt += 1;
        }
        if (cnt >= ORLG_LLOG_FLUSH) need_replay = true;
        old &= 0x03ffffff;
        lint[link] = nspan | (ngaps << 16) | (cnt << 26);
        dspan = nspan - (old & 0xffff);
        dgaps = ngaps - (old >> 16);
    }
    if constexpr (PART) {
        sum_span += dspan;
        sum_gaps += dgaps;
    } else {
        sum_span += row_add_i32(dspan);
        sum_gaps += row_add_i32(dgaps);
    }
    wave_sync();
}

DEV void group_link_replay(const int lane, double *lst, int32_t *lint, const Tab &tb, int S, int E, const uint4 *llog) {
    link_replay<ORLG_GL>(lane, lst, lint, tb, S, E, llog);
}

// The logged graph statistics of the lean body (orlg_graph_log.h), worked off: lane k of a row holds entry k of the row's
// environment, `cnt` of them (the same number on the row's lanes; the lanes from `cnt` on hold stale entries nobody reads).
// Every lane evaluates its own entry -- the compactness, the reciprocal of its time, the time difference to the entry before it
// (the previous lane's time; g_last_update for entry 0) and the two products: the part of _update_network_stats that does not depend on
// the running averages.  The chain then runs DOWN THE ROW, for all four rows at once: in iteration k lane k takes the two averages
// as lane k - 1 left them (row_shr:1; lane 0 starts from the stored ones), applies its own entry and hands the result on, so
// the terms stay where they were evaluated and only two doubles move per link of the chain.  A lane without an entry (a row with
// fewer entries than the longest, nmax) or whose time fails the guard hands on what it received; after nmax iterations lane
// nmax - 1 of every row holds the row's result.  The other lanes execute the same instructions on values nobody reads.  Between
// two replays the three doubles rest in the environment's scalars record (HBM; a few accesses per launch): no register of the
// step loop holds them.  Rows past the batch's end never log (their steps are not accepted).  The DPP reads stand outside any
// condition.
static_assert(255 * 64 * ORLG_MAX_W <= ORLG_GLOG_MAX_ES, "a link is a byte, a link's bitmap ORLG_MAX_W words: the log's E S fields");
DEV void group_graph_replay(const int lane, const OrlgGraphEntry &lg, int &cnt, OrlgEnvScalars *gs, int E) {
    const int gl = lane & 15;
    // what other lanes of this wave stored in an earlier replay: the stores only have to be complete (same CU)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const bool head = gl == 0 && cnt > 0;
    double x_thr = 0.0, x_comp = 0.0, g_lu = 0.0;
    if (head) { x_thr = gs->g_throughput; x_comp = gs->g_compactness; g_lu = gs->g_last_update; }
    const double before = ORLG_DPP_F64(lane_prev_i32, lg.now);
    const double lu = gl == 0 ? g_lu : before;   // g_last_update as the lane's entry meets it: every update ends with g_lu = now
    const OrlgGraphTerm t = orlg_glog_eval(lg, lu, E);
    const bool upd = gl < cnt && t.now > 0;
    const int c0 = __builtin_amdgcn_readlane(cnt, 0), c1 = __builtin_amdgcn_readlane(cnt, 16);
    const int c2 = __builtin_amdgcn_readlane(cnt, 32), c3 = __builtin_amdgcn_readlane(cnt, 48);
    const int m01 = c0 > c1 ? c0 : c1, m23 = c2 > c3 ? c2 : c3;
    const int nmax = m01 > m23 ? m01 : m23;
    double o_thr = 0.0, o_comp = 0.0;
    for (int k = 0; k < nmax; ++k) {
        const double n_thr = orlg_glog_chain(x_thr, lu, t.c_thr, t.now, t.ynow);
        const double n_comp = orlg_glog_chain(x_comp, lu, t.c_comp, t.now, t.ynow);
        o_thr = upd ? n_thr : x_thr;
        o_comp = upd ? n_comp : x_comp;
        x_thr = ORLG_DPP_F64(lane_prev_i32, o_thr);
        x_comp = ORLG_DPP_F64(lane_prev_i32, o_comp);
    }
    if (gl == nmax - 1 && cnt > 0) { gs->g_throughput = o_thr; gs->g_compactness = o_comp; }
    if (gl == cnt - 1) gs->g_last_update = lg.now;   // (g_last_update = now also where the guard fails)
    cnt = 0;
}

// set (release) or clear (provision) the window [s, s+n) on every link of a row's path; hops = 0: the row does not take part
template <int W>
DEV void group_apply_window(int lane, u64 *occ, const uint8_t *links, int hops, int s, int n, bool set_free) {
    constexpr int HPP = ORLG_GL / W;  // hops per pass
    const int gl = lane & 15;
    const int hs = gl / W, w = gl - hs * W;
    const u64 m = window_mask(s, n, w);
    for (int h0 = 0;; h0 += HPP) {
        if (ballot(h0 < hops) == 0ull) break;
        const int h = h0 + hs;
        if (hs < HPP && h < hops && m) {
            u64 *word = occ + __mul24((int)links[h], W) + w;
            *word = set_free ? (*word | m) : (*word & ~m);
        }
    }
    wave_sync();
}

// A quad's slices of one array between HBM and LDS: `bytes` (a multiple of 8) from a wave-uniform source by all 64 lanes, 16
// bytes per lane and pass (the quad's first environment is a multiple of four: 32-byte aligned for every array copied this way)
DEV void quad_copy(void *dst, const void *src, int bytes, int lane) {
    const int n16 = bytes >> 4;
    const uint4 *s16 = reinterpret_cast<const uint4 *>(src);
    uint4 *d16 = reinterpret_cast<uint4 *>(dst);
    // four requests per lane before the first write: a quad's occupancy (3.5 KB) is one round trip, not four
    for (int i0 = 0; i0 < n16; i0 += 4 * ORLG_WAVE) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * ORLG_WAVE + lane;
            v[k] = make_uint4(0u, 0u, 0u, 0u);
            if (i < n16) v[k] = s16[i];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * ORLG_WAVE + lane;
            if (i < n16) d16[i] = v[k];
        }
    }
    if ((bytes & 8) && lane == 0) reinterpret_cast<u64 *>(dst)[2 * n16] = reinterpret_cast<const u64 *>(src)[2 * n16];
}

// The highest fit level (include/orlg.h ORLG_FIT_*) over the K candidate paths of each row's pending request: wave_fit_levels
// (orlg_block_cause.h) in this kernel's layout -- 16 / W paths, then 16 / W links, per row and pass, a path's or a link's W words
// on consecutive lanes.  `need`: the row asks (its step is not accepted); the rows diverge, so every loop runs to the longest
// row and the others are predicated.  occ: the row's occupancy (LDS); base: the first path record of its request.
template <int W>
DEV int group_fit_level(int lane, const u64 *occ, const Tab &tb, int base, int K, int S, int br, bool need) {
    constexpr int PP = ORLG_GL / W;   // paths, or links, per row and pass
    const int gl = lane & 15;
    const int ps = gl / W, w = gl - ps * W;
    int top = 0;
    // windows: a first fit below S - n (4), only the window at S - n (3)
    for (int p0 = 0; p0 < K; p0 += PP) {
        const int pp = p0 + ps;
        const bool on = need && ps < PP && pp < K;
        int se_pp, hops_pp;
        const u64 x = group_path_word_rec<W>(occ, tb.recs, base + pp, w, on, se_pp, hops_pp);
        int n = 1;
        if (on) n = tb.nslots[br * ORLG_NSLOT_STRIDE + se_pp];
        const int lv = on ? window_level(run_starts<W>(x, n, w), n, S, w) : 0;
        const int row = row_ballot(lv == 4, lane) ? 4 : (row_ballot(lv == 3, lane) ? 3 : 0);
        top = row > top ? row : top;
    }
    // links, for the rows without a window: per path, some link short of n free slots (0), some link without a run of n (1), else 2
    const bool more = need && top < 3;
    if (ballot(more) == 0ull) return top;
    for (int idp = 0; idp < K; ++idp) {
        if (ballot(more && top < 2) == 0ull) break;   // every row that asks has its answer: no path scores above 2 here
        const OrlgPathRec *rec = tb.recs + (base + idp);
        const int hops = more && top < 2 ? (int)rec->hops : 0;
        const int n = tb.nslots[br * ORLG_NSLOT_STRIDE + rec->se];
        uint32_t nocap = 0u, norun = 0u;
        for (int h0 = 0;; h0 += PP) {
            if (ballot(h0 < hops) == 0ull) break;
            const int h = h0 + ps;
            const bool on = ps < PP && h < hops;
            u64 x = 0ull;
            if (on) x = occ[__mul24((int)rec->link[on ? h : 0], W) + w];
            const uint32_t freec = seg_add<W>((uint32_t)popc64(x));
            const uint32_t has = seg_max<W>(run_starts<W>(x, n, w) != 0ull ? 1u : 0u);
            const bool head = on && w == 0;   // the link's first lane holds the link's results
            nocap |= row_ballot(head && (int)freec < n, lane);
            norun |= row_ballot(head && has == 0u, lane);
        }
        const int lv = nocap ? 0 : (norun ? 1 : 2);
        if (more && lv > top) top = lv;
    }
    return top;
}

// HBMQ: launches of very few steps (the agent-driven loop) leave the release queue where it is, in HBM: staged in LDS it is
// half of an environment's footprint there (its capacity, not its live part, sizes the region), and a one-step launch is
// bound by how many waves a CU keeps resident, not by the queue's latency.  The ring logic is the same code on
// global pointers; OrlgParams::g_wave_bytes of such a launch ends where the ring's LDS slices would begin.
// TRAFFIC: the handle has per-environment traffic (OrlgParams::rates).  A template argument and not a test at run time: the
// instantiations that serve handles with the two scalars stay, instruction for instruction, what they were without the feature
// TRACE: the handle replays a request trace (OrlgParams::tr_*): a refill copies the next requests of the row's environment into
// its ring (refill_requests_trace_as) -- no staging buffer, no lock, no round trip of generator state -- and the ring's first
// array is the arrival time itself.  A template argument for the same reason as TRAFFIC
// LEAN: the body of a launch that steps a first-fit heuristic (shortest path / shortest available path) with no per-step output
// and discrete bit rates (OrlgParams::g_lean; the long launches of a heuristic's evaluation or a load sweep).  The kernel's one
// body serves every launch a handle can ask for, all decided at run time: seven policies, twelve outputs with two means over the
// links, two request generators -- and the step loop pays for the registers of what it never runs (94 spilled VGPRs at 168).  The
// lean body is the same text (orlg_group_body.h) with those parts compiled out: the same operations on the same values as the
// full body performs for such a launch.  Always inlined: a call would cost the ABI's register traffic
template <int W, int STATS, bool HBMQ, bool DEFER, bool TRAFFIC, bool TRACE, bool LEAN>
DEV void orlg_rmsa_group_body(const OrlgParams &p) {
    constexpr bool CAUSE = false;   // (the DEFER instantiations have no classifier: a cause launch runs the plain kind)
    constexpr bool ASSIGN = false;  // (... and no assignment rule but the reference's first fit)
    constexpr bool CUT = false;
    constexpr bool USAGE = false;
#include "orlg_group_body.h"
}

// The kernel.  A DEFER instantiation holds the lean body beside the full one and chooses at entry: one wave-uniform test of a
// kernel argument, a scalar branch.  Every other instantiation is the body's text alone, the code it was.
// CAUSE: the launch asks for the blocking cause of its steps (include/orlg.h orlg_step_diag): the rows whose step is not accepted
// are classified (group_fit_level) before the provision touches the occupancy.  A template argument for the same reason as
// TRAFFIC; the plain kind only (orlg_group_plan.h keeps such a launch on it)
// ASSIGN: the launch runs an assignment rule other than the reference's first fit (include/orlg.h orlg_step_assign,
// OrlgParams::assign; orlg_assign.h): the policy section is the rules' own.  A template argument and the plain kind only, as CAUSE
// CUT (with ASSIGN): the launch runs the fewest-cuts window (orlg_step_min_cut; orlg_cut.h): its hop loop stands in the rules' place.
// A flag of its own so that the ASSIGN instantiations stay the code they were
// USAGE (with ASSIGN, without CUT): the launch is orlg_step_window's under the rule MOST_USED or the route BEST_WINDOW (orlg_usage.h):
// a policy loop of its own, and the four environments' prefix sums of the slot usage in LDS behind the workgroup's wave regions
// (4 * ORLG_USAGE_BYTES(W) per wave, asked for by the launch alone)
template <int W, int STATS, bool HBMQ = false, bool DEFER = false, bool TRAFFIC = false, bool TRACE = false, bool CAUSE = false, bool ASSIGN = false,
          bool CUT = false, bool USAGE = false>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_GROUP_WAVES, (ORLG_GROUP_WAVES + 3) / 4) void orlg_rmsa_group_kernel(const OrlgParams p) {
    if constexpr (DEFER) {
        if (p.g_lean) orlg_rmsa_group_body<W, STATS, HBMQ, DEFER, TRAFFIC, TRACE, true>(p);
        else orlg_rmsa_group_body<W, STATS, HBMQ, DEFER, TRAFFIC, TRACE, false>(p);
    } else {
        constexpr bool LEAN = false;
#include "orlg_group_body.h"
    }
}
