// orlg_spectrum.h -- questions about free slots, answered on bitmaps: one 64-bit word per 64 slots, a set bit = a free slot.
//
// On a wave-uniform path-wide bitmap x[W] (lane l of word w owns slot 64 w + l): ext_chain, ffbl_hw, free_run_length, first_fit,
// find_block, window_free.  On the link bitmaps of a path record, one (path, word) per lane: path_word, path_word_rec.  On a
// bitmap whose W words sit on W consecutive lanes of a DPP row: run_starts.  The functions take the bitmap and the records as
// plain pointers and know no kernel's layout: the wave-per-environment and four-environments-per-wave step kernels, the query
// and mask kernels and the QoT-aware step (path_word) all call them.
//
// Reference: optical_rl_gym/envs/rmsa_env.py is_path_free :721-734, get_available_slots :745-756, get_available_blocks :774-804,
// the first-fit loops of the heuristics :860-871, :908-913.
#pragma once
#include "orlg_run_schedule.h"
#include "orlg_wave.h"

// ---------------------------------------------------------------------------------------- first fit
// x[w]: wave-uniform free bitmap of one path (AND over its links).  Lane l of word w owns slot 64w+l
// and computes the length of the free run starting there.
template <int W>
DEV void ext_chain(const u64 (&x)[W], int (&ext)[W]) {
    ext[W - 1] = 0;
#pragma unroll
    for (int w = W - 2; w >= 0; --w) ext[w] = (x[w + 1] == ~0ull) ? 64 + ext[w + 1] : ctz64(~x[w + 1]);
}

// v_ffbl_b32 as the hardware defines it: index of the lowest set bit, 0xffffffff for 0 (__builtin_ctz is undefined there)
DEV uint32_t ffbl_hw(uint32_t v) {
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}
// length of the free run that starts at this lane's slot: t = (~word) >> lane has its lowest set bit at the first used slot at
// or after the lane; none left in the word (t == 0) -> the run reaches the word's end and goes on for `rest - (64 - lane)`
// slots in the next words.  ffbl(0) = 0xffffffff keeps the "none" case out of both minima without a select.
DEV int free_run_length(u64 t, int rest /* (64 - lane) + extension into the next words */) {
    const uint32_t a = ffbl_hw((uint32_t)t), b = ffbl_hw((uint32_t)(t >> 32)) | 32u;
    const uint32_t c = a < b ? a : b;
    return (int)(c < (uint32_t)rest ? c : (uint32_t)rest);
}

// smallest s in [0, limit) with slots [s, s+n) free, or -1 (rmsa_env.py:860-871, 908-913)
template <int W>
DEV int first_fit(const u64 (&x)[W], int n, int limit, int lane) {
    if (limit <= 0) return -1;
    int ext[W];
    ext_chain<W>(x, ext);
    const int to_end = 64 - lane;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        if (x[w] != 0ull && 64 * w < limit) {
            const int len = free_run_length((~x[w]) >> lane, to_end + ext[w]);
            // start slots below the limit: a wave-uniform lane mask, no per-lane compare
            const int below = limit - 64 * w;
            const u64 ok = below >= 64 ? ~0ull : ((1ull << below) - 1ull);
            const u64 m = ballot(len >= n) & ok;
            if (m) return 64 * w + ctz64(m);
        }
    }
    return -1;
}

// b-th (0-based) free run with length >= n (rmsa_env.py:774-804); returns start or -1, *len_out = its length
template <int W>
DEV int find_block(const u64 (&x)[W], int n, int b, int lane, int *len_out) {
    int ext[W];
    ext_chain<W>(x, ext);
#pragma unroll
    for (int w = 0; w < W; ++w) {
        if (x[w] != 0ull) {
            u64 carry = w > 0 ? (x[w > 0 ? w - 1 : 0] >> 63) : 0ull;
            u64 starts = x[w] & ~((x[w] << 1) | carry);
            int len = free_run_length((~x[w]) >> lane, (64 - lane) + ext[w]);
            u64 m = ballot(len >= n) & starts;   // run starts: a wave-uniform lane mask
            int cnt = popc64(m);
            if (b < cnt) {
                for (int q = 0; q < b; ++q) m &= m - 1;
                int l = ctz64(m);
                *len_out = __builtin_amdgcn_readlane(len, l);
                return 64 * w + l;
            }
            b -= cnt;
        }
    }
    return -1;
}

// is_path_free (rmsa_env.py:721-734) on a path-wide mask
template <int W>
DEV bool window_free(const u64 (&x)[W], int s, int n, int S) {
    if (s + n > S) return false;
    bool ok = true;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        u64 m = window_mask(s, n, w);
        ok = ok && ((x[w] & m) == m);
    }
    return ok;
}

// AND of the link bitmaps of path record `gid` for word w (get_available_slots, rmsa_env.py:745-756).
// `active` lanes hold a valid (gid, w); the hop loop is fully unrolled over the 16-byte record with
// compile-time byte positions (v_bfe_u32 + v_mad_u32_u24 per hop) and leaves as soon as no lane has hops left.
template <int W>
DEV u64 path_word(const u64 *occ, const OrlgPathRec *recs, int gid, int w, bool active) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (active) r = *reinterpret_cast<const uint4 *>(recs + gid);
    const uint32_t q[4] = {r.x, r.y, r.z, r.w};
    const int hops = (int)(r.x & 0xffu);  // 0 on inactive lanes
    u64 acc = active ? ~0ull : 0ull;
#pragma unroll
    for (int h = 0; h < ORLG_MAX_HOPS; ++h) {
        if (ballot(h < hops) == 0ull) break;
        const int link = (int)((q[(h + 2) >> 2] >> (8 * ((h + 2) & 3))) & 0xffu);
        if (h < hops) acc &= occ[__mul24(link, W) + w];
    }
    return acc;
}

// path_word that also hands back the record's spectral efficiency and hop count (0 on inactive lanes)
template <int W>
DEV u64 path_word_rec(const u64 *occ, const OrlgPathRec *recs, int gid, int w, bool active, int &se, int &hops_out) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (active) r = *reinterpret_cast<const uint4 *>(recs + gid);
    const uint32_t q[4] = {r.x, r.y, r.z, r.w};
    const int hops = (int)(r.x & 0xffu);
    se = (int)((r.x >> 8) & 0xffu);
    hops_out = hops;
    u64 acc = active ? ~0ull : 0ull;
#pragma unroll
    for (int h = 0; h < ORLG_MAX_HOPS; ++h) {
        if (ballot(h < hops) == 0ull) break;
        const int link = (int)((q[(h + 2) >> 2] >> (8 * ((h + 2) & 3))) & 0xffu);
        if (h < hops) acc &= occ[__mul24(link, W) + w];
    }
    return acc;
}

// Bits b of word w such that slots [64 w + b, 64 w + b + n) are all free, for a bitmap whose W words sit on W consecutive lanes
// of a row (w = the lane's word; `x` = 0 on lanes that hold nothing).  r_m = AND of x >> 0 .. x >> (m - 1) is doubled:
// r_{m+k} = r_m & (r_m >> k) for k <= m; k <= 31, so that a shift is two 32-bit funnel shifts (v_alignbit_b32) fed by the next
// word's low half (one DPP read).  n may differ between the rows (and between the paths inside a row): the loop runs to the
// longest, a finished lane shifts by k = 0, which leaves it as it is -- no predication.  The schedule is orlg_run_schedule.h's: the
// slots covered so far are one number for the wave (have_u and the round's step ku depend on no lane: scalar registers), a lane
// carries only what it has left (rem), n >= 1.  `keep` (nothing beyond the path's last word) is a mask in a register, not a
// condition -- the empty asm keeps the compiler from turning it back into a select -- so that the DPP read, which gives 0 past
// the row's end, folds into the AND (v_and_b32_dpp).  Eight vector instructions a round: v_min (k), v_and_dpp, 2 x v_alignbit,
// 2 x v_and, v_sub (rem), v_cmp (the ballot).  The ballot and the DPP read stand outside every condition.
//
// The loop's shape is part of its cost.  The exit test is a ballot of rem > 0 (which is k > 0: ku >= 1) at the END of a round,
// behind one test before the first: the compiler then closes the round with v_cmp + s_cbranch_vccnz, one taken branch, and
// keeps have_u scalar.  `for (;;) { ...; if (ballot(k > 0) == 0) break; ... }` became a round of three branches around a
// scalar select of the exit condition, and `while (ballot(rem > 0))` put have_u into a vector register (profiles/README.md,
// round 17: the shape is worth more than the three instructions).
template <int W>
DEV u64 run_starts(u64 x, int n, int w) {
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    uint32_t keep = w == W - 1 ? 0u : ~0u;  // nothing beyond the last word
    asm volatile("" : "+v"(keep));
    int rem = orlg_run_rem0(n);
    int have_u = 1;
    if (ballot(rem > 0) != 0ull) {   // (none: every lane wants one slot, r_1 = x)
        do {
            const int ku = orlg_run_ku(have_u);
            const int k = orlg_run_k(rem, ku);
            const uint32_t nlo = (uint32_t)lane_next_i32((int)lo) & keep;
            const uint32_t slo = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)k), shi = __builtin_amdgcn_alignbit(nlo, hi, (uint32_t)k);
            lo &= slo; hi &= shi;
            rem -= k;
            have_u += ku;
        } while (ballot(rem > 0) != 0ull);
    }
    return ((u64)hi << 32) | lo;
}
