// orlg_mask_kernels.hip -- valid-action masks of the RMSA environments for the whole batch (include/orlg.h orlg_action_masks).
//
// mask[a] = 1 iff the reference's step(a) on the pending request would provision the service:
//     slots    bit s of path p  <=>  RMSAEnv.step([p, s]) provisions: s + n <= S and is_path_free(path_p, s, n)
//                                    (rmsa_env.py:233-260, 721-734), n = get_number_slots(path_p) (:708-719)
//     path_ff  path p           <=>  PathOnlyFirstFitAction.action(p) finds a slot (rmsa_env.py:974-1008): some s in
//                                    range(0, S - n) is free -- the bound is exclusive, a path whose only fit starts at S - n
//                                    is NOT valid here although step([p, S - n]) provisions
// The kernel has the shape of orlg_deeprmsa_obs_kernel: tables staged once per workgroup, one wave per environment at a time,
// the grid sized to the device and striding over the batch, the occupancy row copied to LDS.  It reads state and writes only
// the caller's buffers.  (The DeepRMSA mask leaves orlg_deeprmsa_obs_kernel itself: the block scan is the observation's.)
#pragma once
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// Eight candidate paths per pass: path p0 + g on the 8-lane group g (two groups per DPP row), one word per lane -- the layout
// run_starts needs (a path's words on consecutive lanes of one row).  path_ff: [B][ff_dim] bytes, ff_dim = K (+ 1: the explicit
// rejection, always valid); slots: [B][K][W] words; either may be nullptr.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_action_masks_kernel(const OrlgParams p, uint8_t *path_ff,
                                                                                                int ff_dim, u64 *slots) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int occ_bytes = (p.NW * 8 + 15) & ~15;
    u64 *occ = reinterpret_cast<u64 *>(smem + p.l_shared_bytes + (size_t)wib * occ_bytes);
    const int N = p.N, K = p.K, S = p.S;
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
        const int base = tb.pair_base[src * N + dst];
        for (int p0 = 0; p0 < K; p0 += 8) {
            const int idp = p0 + g8;
            const bool on = idp < K && w < W;
            int se_l, hops_l;
            const u64 x = path_word_rec<W>(occ, tb.recs, base + idp, w, on, se_l, hops_l);
            int n = 1;
            if (on) n = tb.nslots[br * ORLG_NSLOT_STRIDE + se_l];
            // starts of the windows of n free slots; slots at and beyond S are stored as used, so a window never leaves the spectrum
            const u64 fit = run_starts<W>(x, n, w);
            if (slots && on) slots[((size_t)env * K + idp) * W + w] = fit;
            if (path_ff) {
                // the first-fit loops never try the start S - n (range(0, S - n))
                const int last = S - n;
                const u64 tried = (last >= 0 && (last >> 6) == w) ? fit & ~(1ull << (last & 63)) : fit;
                const int any = group8_max(on && tried != 0ull ? 1 : 0);
                if (on && w == 0) path_ff[(size_t)env * ff_dim + idp] = (uint8_t)any;
            }
        }
        if (path_ff && lane == 0 && ff_dim > K) path_ff[(size_t)env * ff_dim + K] = 1;
        wave_sync();
    }
}
