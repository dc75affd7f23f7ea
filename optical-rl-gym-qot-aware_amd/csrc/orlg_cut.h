// orlg_cut.h -- fragmentation-aware spectrum assignment: the window with the fewest cuts (include/orlg.h
// orlg_step_min_cut, orlg_path_min_cuts).  For candidate path p of the pending request, n = get_number_slots(p), a window start s
// in 0 .. S - n (orlg_assign.h's windows):
//     cuts(p, s) = the number of links l of p with slot s - 1 AND slot s + n free on l (slots -1 and S are not free)
// -- the links on which the window splits one free block into two (Yin et al. 2013, the source the reference cites for its
// compactness; the reference has the count on its QoT-aware environment only, calculate_r_cut).  The rule MIN_CUT takes the
// window with the fewest cuts, ties to the lowest start; the route "fewest cuts" takes, of all k paths, the path whose MIN_CUT
// window has the fewest cuts, ties to the lowest path.  Not in the reference for these environments; integer-exact.
//
// The arithmetic, on the (path, word) lanes of orlg_assign.h (a path's W words on W consecutive lanes of a DPP row): the hop loop
// sees every hop's words, not only their AND.  Per hop: Lf = the link's word shifted up by one slot (the previous word's top bit
// arrives by DPP: the path's lanes walk the same link), Rf = the link's bitmap shifted down by n slots (two LDS words, funnel
// shifted), and Lf & Rf -- the starts this link would be cut at -- is added into a bit-sliced counter, four 64-bit planes per lane
// (hops <= 14 < 16).  Then the lane's minimum is read off the planes from the top plane down and ONE maximum of a key
// (cuts, start) over the path's lanes decides, as for every other rule.  The whole wave takes part: DPP moves stand outside
// conditions, hop words past a path's end are read (a valid address) and selected away.
#pragma once
#include "../../include/orlg.h"
#include "orlg_assign.h"   // ORLG_ASSIGN_KEY_TOP, the lane layouts
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// The MIN_CUT key of THIS lane's word of path record `gid`: ORLG_ASSIGN_KEY_TOP - (cuts << 10 | start) of the lane's best window,
// 0 = the word holds no window start -- a maximum over the path's lanes is the path's MIN_CUT window.  w: the lane's word, any
// value on an inactive lane; nsl: the request's row of the slots table (Tab::nslots + bit-rate index * ORLG_NSLOT_STRIDE).
// Hands back the record's hops, n (1 on an inactive lane) and x = the lane's word of the path-wide bitmap (0 on an inactive lane).
template <int W>
DEV uint32_t cut_word_key(const u64 *occ, const OrlgPathRec *recs, int gid, int w, bool active, const uint16_t *nsl, int S, int &hops_out,
                          int &n_out, u64 &x_out) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (active) r = *reinterpret_cast<const uint4 *>(recs + gid);
    const uint32_t q[4] = {r.x, r.y, r.z, r.w};
    const int hops = (int)(r.x & 0xffu);   // 0 on inactive lanes
    int n = 1;
    if (active) n = nsl[(r.x >> 8) & 0xffu];
    hops_out = hops;
    n_out = n;
    // the words of a link this lane reads: its own, and the two that hold slots 64 w + n .. 64 w + n + 63 (beyond the link: 0)
    const int wc = w < W ? w : W - 1;
    const int wa = w + (n >> 6), wb = wa + 1;
    const int wa_c = wa < W ? wa : W - 1, wb_c = wb < W ? wb : W - 1;
    const u64 a_keep = wa < W ? ~0ull : 0ull, b_keep = wb < W ? ~0ull : 0ull;
    const int sh = n & 63;
    const int first = __mul24((int)((r.x >> 16) & 0xffu), W);   // the path's first link: what a hop past the end reads
    u64 acc = ~0ull, p0 = 0ull, p1 = 0ull, p2 = 0ull, p3 = 0ull;
#pragma unroll
    for (int h = 0; h < ORLG_MAX_HOPS; ++h) {
        if (ballot(h < hops) == 0ull) break;
        const bool in = h < hops;
        const int link = (int)((q[(h + 2) >> 2] >> (8 * ((h + 2) & 3))) & 0xffu);
        const int lw = in ? __mul24(link, W) : first;
        const u64 cur = occ[lw + wc], ra = occ[lw + wa_c] & a_keep, rb = occ[lw + wb_c] & b_keep;
        const uint32_t prev_hi = (uint32_t)lane_prev_i32((int)(uint32_t)(cur >> 32));
        const u64 lf = (cur << 1) | (w > 0 ? (u64)(prev_hi >> 31) : 0ull);   // bit s: slot 64 w + s - 1 of the link
        const u64 rf = (ra >> sh) | ((rb << 1) << (63 - sh));                 // bit s: slot 64 w + s + n of the link
        u64 c = in ? lf & rf : 0ull, t;
        // ripple carry; after hop h a count is at most h + 1, so the upper planes join when they can first be reached
        t = p0 & c; p0 ^= c; c = t;
        if (h >= 1) { t = p1 & c; p1 ^= c; c = t; }
        if (h >= 3) { t = p2 & c; p2 ^= c; c = t; }
        if (h >= 7) p3 ^= c;
        acc &= in ? cur : ~0ull;
    }
    const u64 x = active ? acc & valid_mask(S, wc) : 0ull;
    x_out = x;
    const u64 fit = run_starts<W>(x, n, w);   // the window starts of this word
    // the starts with the fewest cuts: from the top plane down, keep those with a 0 where any has one
    u64 cand = fit, t;
    t = cand & ~p3; cand = t ? t : cand;
    t = cand & ~p2; cand = t ? t : cand;
    t = cand & ~p1; cand = t ? t : cand;
    t = cand & ~p0; cand = t ? t : cand;
    const int b = cand ? ctz64(cand) : 0;
    const uint32_t cuts = (uint32_t)((p0 >> b) & 1ull) | (uint32_t)((p1 >> b) & 1ull) << 1 | (uint32_t)((p2 >> b) & 1ull) << 2 |
                          (uint32_t)((p3 >> b) & 1ull) << 3;
    return cand ? ORLG_ASSIGN_KEY_TOP - (cuts << 10 | (uint32_t)(64 * wc + b)) : 0u;
}
// what a path's winning key (not 0) names
DEV int cut_key_slot(uint32_t key) { return (int)((ORLG_ASSIGN_KEY_TOP - key) & 1023u); }
DEV int cut_key_cuts(uint32_t key) { return (int)((ORLG_ASSIGN_KEY_TOP - key) >> 10); }

// wave_assign (orlg_assign.h) under the rule MIN_CUT: (path << 10) | slot of the request under route `route` (ORLG_POLICY_SP / SAP /
// LLP / PATH_EXT as there, or ORLG_POLICY_MIN_CUT: of all K paths the one whose MIN_CUT window has the fewest cuts, ties to the
// lowest path), or -1 = no path of the route has a window.  Eight candidate paths per pass; across passes the comparison is
// strict, so the earlier pass wins a tie.  Wave-uniform result.
template <int W>
DEV int wave_cut_assign(const u64 *occ, const Tab &tb, int base, int K, int S, int br, int lane, int route, int given) {
    const int g8 = lane >> 3, w = lane & 7;
    int path0 = 0, kmax = route == ORLG_POLICY_SP ? 1 : K;
    if (route == ORLG_POLICY_PATH_EXT) {
        if (given < 0 || given >= K) return -1;
        path0 = given;
        kmax = 1;
    }
    const bool ranked = route == ORLG_POLICY_LLP || route == ORLG_POLICY_MIN_CUT;
    int found = -1, top = 0;
    for (int p0 = 0; p0 < kmax; p0 += 8) {
        const int idp = p0 + g8;
        const bool on = idp < kmax && w < W;
        int hops_l, n;
        u64 x;
        const uint32_t wk = cut_word_key<W>(occ, tb.recs, base + path0 + idp, w, on, tb.nslots + br * ORLG_NSLOT_STRIDE, S, hops_l, n, x);
        const int key = group8_max((int)wk);   // the path's key on every lane of its group
        if (ranked) {
            // llp: most free slots; fewest cuts: the key without its start (larger = fewer cuts).  Strict >: ties go to the first
            const int fs = group8_add(popc64(x));
            const int rank = route == ORLG_POLICY_LLP ? fs : key >> 10;
            const int m = wave_max_i32(key ? (rank << 4) | (7 - g8) : 0);
            if (m && (m >> 4) > top) {
                const int g = 7 - (m & 15);
                top = m >> 4;
                found = ((p0 + g) << 10) | cut_key_slot((uint32_t)__builtin_amdgcn_readlane(key, g << 3));
            }
        } else {
            const u64 m = ballot(key != 0 && w == 0);
            if (m) {
                const int g = ctz64(m) >> 3;
                found = ((path0 + p0 + g) << 10) | cut_key_slot((uint32_t)__builtin_amdgcn_readlane(key, g << 3));
                break;
            }
        }
    }
    return found;
}

// orlg_path_min_cuts (include/orlg.h): the MIN_CUT window of every candidate path of every pending request -- cuts [B][K] (-1 = the
// path has no window), slots [B][K] (S there); either may be null.  The shape of orlg_fit_levels_kernel: tables staged once per
// workgroup, one wave per environment at a time, the grid striding over the batch, the occupancy row copied to LDS.  Reads state
// and writes only its outputs.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_min_cuts_kernel(const OrlgParams p, int16_t *cuts, int16_t *slots) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int occ_bytes = (p.NW * 8 + 15) & ~15;
    u64 *occ = reinterpret_cast<u64 *>(smem + p.l_shared_bytes + (size_t)wib * occ_bytes);
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const bool wide = (p.NW & 1) == 0;
    const int g8 = lane >> 3, w = lane & 7;
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = sc->req_src, dst = sc->req_dst, br = sc->req_br;
        if (wide) copy_words(occ, p.occ + (size_t)env * p.NW, p.NW * 8, lane);
        else {
            const u64 *g = p.occ + (size_t)env * p.NW;
            for (int i = lane; i < p.NW; i += 64) occ[i] = g[i];
        }
        wave_sync();
        const int base = tb.pair_base[src * p.N + dst];
        for (int p0 = 0; p0 < p.K; p0 += 8) {
            const int idp = p0 + g8;
            const bool on = idp < p.K && w < W;
            int hops_l, n;
            u64 x;
            const uint32_t key = (uint32_t)group8_max(
                (int)cut_word_key<W>(occ, tb.recs, base + idp, w, on, tb.nslots + br * ORLG_NSLOT_STRIDE, p.S, hops_l, n, x));
            if (on && w == 0) {
                const size_t o = (size_t)env * p.K + idp;
                if (cuts) cuts[o] = (int16_t)(key ? cut_key_cuts(key) : -1);
                if (slots) slots[o] = (int16_t)(key ? cut_key_slot(key) : p.S);
            }
        }
        wave_sync();
    }
}
