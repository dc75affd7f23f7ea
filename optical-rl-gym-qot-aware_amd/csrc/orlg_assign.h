// orlg_assign.h -- spectrum-assignment rules beyond the reference's first fit (include/orlg.h ORLG_ASSIGN_*): where on
// a candidate path the service starts -- the lowest window of the whole range 0 .. S - n (FIRST_FULL), the highest window (LAST),
// the shortest free block of >= n slots (BEST), the lowest block of exactly n slots (EXACT).  Not in the reference: its heuristics
// (rmsa_env.py:854-937) are first fit over range(0, S - n) only; the routes they walk are kept.
//
// The bitmap arithmetic, next to run_starts (orlg_spectrum.h) and for the same layout: the W words of a path-wide free bitmap sit
// on W consecutive lanes of a DPP row (w = the lane's word, 0 on a lane that holds nothing) -- 16 / W paths per row in the
// four-environments-per-wave kernel, one path per 8-lane group in the wave-per-environment kernel.  Every rule is ONE reduction of
// a key per path: assign_word_key is the best key of the lane's own word, a maximum over the path's lanes decides, and
// assign_key_slot reads the start slot out of it.  Integer-exact; the whole wave takes part (DPP moves: uniform control flow).
#pragma once
#include "../../include/orlg.h"   // ORLG_ASSIGN_*
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// key space: 21 bits, 0 = the word holds no candidate; larger wins
#define ORLG_ASSIGN_KEY_TOP 0x1fffffu

// The rule's best candidate among the windows (FIRST_FULL, LAST) or the block starts (BEST, EXACT) of THIS lane's word:
//   FIRST_FULL  lowest window start                      key = TOP - start
//   LAST        highest window start                     key = TOP - (1023 - start)
//   BEST        shortest block of >= n, lowest start     key = TOP - (length << 10 | start)
//   EXACT       a block of exactly n before the others,  key = TOP - ((length != n) << 10 | start)
//               lowest start (the lowest window is a block's start: no block of n -> FIRST_FULL)
// x: the lane's word of the path-wide bitmap, slots at and beyond S not free; n: slots of the request on this path; S <= 512.
// A block's length crosses words: the words' leading-free counts are chained along the row (W - 1 DPP steps), then the lane walks
// the block starts of its own word that hold a window.
template <int W>
DEV uint32_t assign_word_key(u64 x, int n, int w, int rule) {
    const u64 fit = run_starts<W>(x, n, w);   // starts of the free windows of n slots
    if (rule == ORLG_ASSIGN_FIRST_FULL) return fit ? ORLG_ASSIGN_KEY_TOP - (uint32_t)(64 * w + ctz64(fit)) : 0u;
    if (rule == ORLG_ASSIGN_LAST) return fit ? ORLG_ASSIGN_KEY_TOP - (uint32_t)(1023 - (64 * w + 63 - clz64(fit))) : 0u;
    // block starts that hold a window: free slots whose predecessor (the previous word's slot 63 for slot 0) is not free
    const uint32_t prev_hi = (uint32_t)lane_prev_i32((int)(uint32_t)(x >> 32));
    const u64 carry = w > 0 ? (u64)(prev_hi >> 31) : 0ull;
    u64 c = fit & x & ~((x << 1) | carry);
    // free slots that follow this word without a gap: ext(w) = lead(w + 1) + (word w + 1 all free ? ext(w + 1) : 0)
    const bool full = x == ~0ull;
    const int lead = full ? 64 : ctz64(~x);
    int ext = 0;
#pragma unroll
    for (int i = 0; i < W - 1; ++i) {
        ext = lane_next_i32(lead + (full ? ext : 0));
        ext = w == W - 1 ? 0 : ext;   // nothing beyond the last word
    }
    const u64 used = ~x;
    uint32_t best = 0u;
    while (ballot(c != 0ull) != 0ull) {
        if (c != 0ull) {
            const int b = ctz64(c);
            c &= c - 1ull;
            const u64 t = used >> b;
            const int len = t ? ctz64(t) : 64 - b + ext;
            const uint32_t rank = rule == ORLG_ASSIGN_BEST ? (uint32_t)len << 10 : (len != n ? 1024u : 0u);
            const uint32_t key = ORLG_ASSIGN_KEY_TOP - (rank | (uint32_t)(64 * w + b));
            best = key > best ? key : best;
        }
    }
    return best;
}

// the start slot a path's winning key (not 0) names
DEV int assign_key_slot(uint32_t key, int rule) {
    const int v = (int)(ORLG_ASSIGN_KEY_TOP - key);
    return rule == ORLG_ASSIGN_LAST ? 1023 - v : (v & 1023);
}

// The wave-per-environment layout: (path << 10) | slot of the request under route `route` (ORLG_POLICY_SP / SAP / LLP / PATH_EXT,
// rmsa_env.py:854-937, 982-1005; `given` = the agent's path for PATH_EXT) and rule `rule`, or -1 = no path of the route has a window.
// Eight candidate paths per pass, path p0 + g on the 8-lane group g with one word per lane, as orlg_action_masks_kernel lays them
// out; wave-uniform result.  occ: the environment's occupancy (LDS); base: the first path record of the request's node pair.
template <int W>
DEV int wave_assign(const u64 *occ, const Tab &tb, int base, int K, int S, int br, int lane, int route, int rule, int given) {
    const int g8 = lane >> 3, w = lane & 7;
    int path0 = 0, kmax = route == ORLG_POLICY_SP ? 1 : K;
    if (route == ORLG_POLICY_PATH_EXT) {
        if (given < 0 || given >= K) return -1;
        path0 = given;
        kmax = 1;
    }
    const bool llp = route == ORLG_POLICY_LLP;
    int found = -1, max_free = 0;
    for (int p0 = 0; p0 < kmax; p0 += 8) {
        const int idp = p0 + g8;
        const bool on = idp < kmax && w < W;
        int se_l, hops_l;
        const u64 x = path_word_rec<W>(occ, tb.recs, base + path0 + idp, w, on, se_l, hops_l) & valid_mask(S, w);
        int n = 1;
        if (on) n = tb.nslots[br * ORLG_NSLOT_STRIDE + se_l];
        const int key = group8_max((int)assign_word_key<W>(x, n, w, rule));   // the path's key on every lane of its group
        if (llp) {
            // of the paths that have a window, the one with the most free slots; strict >: ties go to the first
            const int fs = group8_add(popc64(x));
            const int m = wave_max_i32(key ? (fs << 4) | (7 - g8) : 0);
            if (m && (m >> 4) > max_free) {
                const int g = 7 - (m & 15);
                max_free = m >> 4;
                found = ((p0 + g) << 10) | assign_key_slot((uint32_t)__builtin_amdgcn_readlane(key, g << 3), rule);
            }
        } else {
            const u64 m = ballot(key != 0 && w == 0);
            if (m) {
                const int g = ctz64(m) >> 3;
                found = ((path0 + p0 + g) << 10) | assign_key_slot((uint32_t)__builtin_amdgcn_readlane(key, g << 3), rule);
                break;
            }
        }
    }
    return found;
}
