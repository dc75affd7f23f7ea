// orlg_block_cause.h -- why a request is refused: the fit level of a candidate path and the blocking cause of a step
// (include/orlg.h ORLG_FIT_*, ORLG_CAUSE_*), for the wave layout -- 64 lanes per environment: the CAUSE
// instantiations of orlg_rmsa_kernel (orlg_kernels.hip) and the query kernel orlg_fit_levels_kernel below.  The group layout's
// classifier, 16 lanes per environment, is group_fit_level in orlg_group_kernels.hip; both are the same two questions asked with
// run_starts (orlg_spectrum.h):
//     windows  on the AND of a path's link bitmaps: a window of n free slots below S - n (level 4), or only the one at S - n
//              that the reference's first-fit loops never try (level 3) -- the bits of orlg_action_masks
//     links    on every link's own bitmap, only for a path without a window: fewer than n free slots on some link (level 0),
//              no run of n on some link (level 1), else the runs exist and do not line up (level 2)
// Not in the reference: it counts a refusal (rmsa_env.py:233-262) and does not say why.  State-based and integer-exact: the
// occupancy the step met, the pending request, nothing else.
#pragma once
#include "../../include/orlg.h"   // ORLG_FIT_*, ORLG_CAUSE_*
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// 4 where `fit` (the starts of the free windows of n slots of a path-wide word w, run_starts) holds a start below S - n, 3 where
// it holds only the start S - n, else 0 -- for this lane's word
DEV int window_level(u64 fit, int n, int S, int w) {
    const int last = S - n;
    const u64 lastbit = (last >= 0 && (last >> 6) == w) ? 1ull << (last & 63) : 0ull;
    return (fit & ~lastbit) ? 4 : ((fit & lastbit) ? 3 : 0);
}

// Levels 0..2 of ONE path (wave-uniform record `rec` in LDS, n slots) from its links' own bitmaps: eight links per pass, link
// h0 + g on the 8-lane group g with one word per lane -- the layout run_starts needs -- free slots by a group sum, "has a run of
// n" by a group maximum, then one ballot each over the pass's links.
template <int W>
DEV int links_level(const u64 *occ, const OrlgPathRec *rec, int n, int lane) {
    const int g8 = lane >> 3, w = lane & 7;
    const int hops = rec->hops;
    bool cap = true, run = true;
    for (int h0 = 0; h0 < hops; h0 += 8) {
        const int h = h0 + g8;
        const bool link_on = h < hops;
        u64 x = 0ull;
        if (link_on && w < W) x = occ[__mul24((int)rec->link[link_on ? h : 0], W) + w];
        const int freec = group8_add(popc64(x));
        const int has = group8_max(run_starts<W>(x, n, w) != 0ull ? 1 : 0);
        cap = cap && ballot(link_on && freec < n) == 0ull;
        run = run && ballot(link_on && !has) == 0ull;
    }
    return !cap ? 0 : (!run ? 1 : 2);
}

// The fit level of every candidate path of the request (src, dst: `base` = its first path record; bit-rate index br) on the
// occupancy `occ` (LDS, E x W words): out[p] = level of path p where `out` is not null (global memory), and the highest level
// of the K paths is returned.  Eight candidate paths per pass as orlg_action_masks_kernel lays them out; every lane of the wave
// takes part.  Without `out` the link questions are only asked when no path has a window (the answer is then below 3).
template <int W>
DEV int wave_fit_levels(const u64 *occ, const Tab &tb, int base, int K, int S, int br, int lane, uint8_t *out) {
    const int g8 = lane >> 3, w = lane & 7;
    int top = 0;
    for (int p0 = 0; p0 < K; p0 += 8) {
        const int idp = p0 + g8;
        const bool on = idp < K && w < W;
        int se_l, hops_l;
        const u64 x = path_word_rec<W>(occ, tb.recs, base + idp, w, on, se_l, hops_l);
        int n = 1;
        if (on) n = tb.nslots[br * ORLG_NSLOT_STRIDE + se_l];
        // (slots at and beyond S are stored as used: a window never leaves the spectrum, and n > S has none)
        int lv = group8_max(on ? window_level(run_starts<W>(x, n, w), n, S, w) : 0);
        if (out) {
            // the paths of this pass that have no window: their links, one path at a time
            for (u64 m = ballot(on && w == 0 && lv < 3); m; m &= m - 1) {
                const int g = ctz64(m) >> 3;
                const int l = links_level<W>(occ, tb.recs + (base + p0 + g), __builtin_amdgcn_readlane(n, g << 3), lane);
                if (g8 == g) lv = l;
            }
            if (on && w == 0) out[idp] = (uint8_t)lv;
        }
        top = lv > top ? lv : top;
    }
    top = wave_max_i32(top);
    if (!out && top < 3) {
        top = 0;
        for (int idp = 0; idp < K && top < 2; ++idp) {
            const OrlgPathRec *rec = tb.recs + (base + idp);
            const int l = links_level<W>(occ, rec, (int)tb.nslots[br * ORLG_NSLOT_STRIDE + rec->se], lane);
            top = l > top ? l : top;
        }
    }
    return top;
}

// orlg_path_fit_levels (include/orlg.h): levels [B][K] of every environment's pending request.  The shape of
// orlg_action_masks_kernel: tables staged once per workgroup, one wave per environment at a time, the grid striding over the
// batch, the occupancy row copied to LDS.  Reads state and writes only `levels`.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_fit_levels_kernel(const OrlgParams p, uint8_t *levels) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int occ_bytes = (p.NW * 8 + 15) & ~15;
    u64 *occ = reinterpret_cast<u64 *>(smem + p.l_shared_bytes + (size_t)wib * occ_bytes);
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const bool wide = (p.NW & 1) == 0;
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = sc->req_src, dst = sc->req_dst, br = sc->req_br;
        if (wide) copy_words(occ, p.occ + (size_t)env * p.NW, p.NW * 8, lane);
        else {
            const u64 *g = p.occ + (size_t)env * p.NW;
            for (int i = lane; i < p.NW; i += 64) occ[i] = g[i];
        }
        wave_sync();
        wave_fit_levels<W>(occ, tb, tb.pair_base[src * p.N + dst], p.K, p.S, br, lane, levels + (size_t)env * p.K);
        wave_sync();
    }
}
