// orlg_gn_mask_kernels.hip -- valid-action masks that know the GN-model admission check, for the whole batch (include/orlg.h
// orlg_gn_action_masks).
//
// mask[a] = 1 iff step(a) on the gated handle would provision the pending request: the window the step would try is free AND its
// GSNR against the services running now meets the threshold of the path's spectral efficiency:
//     path_ff_gn   path p        <=>  step_path_first_fit(p): the first fit s in range(0, S - n) exists (rmsa_env.py:974-1008) and
//                                     the window [s, s + n) passes the gate
//     deeprmsa_gn  action a      <=>  step_deeprmsa(a): block a % j of route a // j exists (deeprmsa_env.py:48-58, rmsa_env.py:
//                                     774-804) and its first n slots pass the gate
// The windows are found by the functions the gated step itself calls for these two actions (first_fit, find_block on the path-wide
// bitmap), and every GSNR is rmsa_gn_gsnr (orlg_rmsa_gn.h) called with the arguments the step would give it: the value the mask
// compares has the bits of the value the step compares.
//
// The kernel has the shape of orlg_action_masks_kernel: tables staged once per workgroup, one wave per environment at a time, the
// grid sized to the device and striding over the batch.  Per environment the occupancy row goes to LDS, and so does the LIVE part
// of the release ring's descriptors -- n_running entries from q_head, copied in ring order to positions 0 .. q_n, so that
// rmsa_gn_gsnr walks them from head 0 in the chunks of 64 the step walks them in and never meets a wrap.  The release times are
// not needed: a state between launches holds no service that is due at the pending request's arrival (the step releases those
// when it draws the request, rmsa_env.py:689-695).  It reads state and writes only the caller's buffers.
#pragma once
#include "orlg_rmsa_gn.h"
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// path_ff: [B][K + reject] bytes, path_ff_gsnr: [B][K] doubles (NaN where path_ff of the plain mask is 0); deeprmsa: [B][K J +
// reject] bytes, deep_gsnr: [B][K J] doubles (NaN where the block does not exist); any of them may be nullptr.  The rejection's
// column is always 1.  LDS per wave: the occupancy row, then Q descriptors.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_gn_action_masks_kernel(const OrlgParams p, uint8_t *path_ff,
                                                                                                   double *path_ff_gsnr, uint8_t *deeprmsa,
                                                                                                   double *deep_gsnr, int reject) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int occ_bytes = (p.NW * 8 + 15) & ~15, q_bytes = (p.Q * 4 + 15) & ~15;
    unsigned char *wb = smem + p.l_shared_bytes + (size_t)wib * (occ_bytes + q_bytes);
    Wave wv = {};
    wv.lane = lane;
    wv.occ = reinterpret_cast<u64 *>(wb);
    wv.qdesc = reinterpret_cast<uint32_t *>(wb + occ_bytes);
    const int N = p.N, K = p.K, S = p.S, J = p.j, Q = p.Q, E = p.E;
    const int LS = K <= 8 ? 8 : W;   // lanes from one candidate path to the next, as the step kernel lays them out
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const bool wide = (p.NW & 1) == 0;
    const OrlgGnTable gn = ORLG_GPTR(const double, p.gn);
    const bool want_ff = path_ff || path_ff_gsnr, want_deep = deeprmsa || deep_gsnr;
    const int ff_dim = K + reject, deep_dim = K * J + reject;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = uni(sc->req_src), dst = uni(sc->req_dst), br = uni(sc->req_br);
        const int q_head = uni(sc->q_head), n_run = uni(sc->n_running);
        const int q_n = n_run < Q ? (n_run < 0 ? 0 : n_run) : Q;   // (n_running also counts services an overflow lost)
        if (wide) copy_words(wv.occ, p.occ + (size_t)env * p.NW, p.NW * 8, lane);
        else {
            const u64 *g = p.occ + (size_t)env * p.NW;
            for (int i = lane; i < p.NW; i += 64) wv.occ[i] = g[i];
        }
        {
            const uint32_t *g = p.qdesc + (size_t)env * Q;
            for (int i = lane; i < q_n; i += 64) {
                int pos = (q_head >= 0 && q_head < Q ? q_head : 0) + i;
                pos -= pos >= Q ? Q : 0;
                wv.qdesc[i] = g[pos];
            }
        }
        wave_sync();
        const int base = tb.pair_base[src * N + dst];
        const int pp = LS == 8 ? lane >> 3 : lane / W, pw = lane - pp * LS;
        int se_l, hops_l;
        const u64 acc = path_word_rec<W>(wv.occ, tb.recs, base + pp, pw, pp < K && pw < W, se_l, hops_l);
        int my_se = 0;
        if (lane < K) my_se = tb.recs[base + lane].se;
        const int my_n = tb.nslots[br * ORLG_NSLOT_STRIDE + my_se];   // get_number_slots per candidate
        for (int idp = 0; idp < K; ++idp) {
            u64 x[W];
#pragma unroll
            for (int w = 0; w < W; ++w) x[w] = readlane64(acc, idp * LS + w);
            const int n = __builtin_amdgcn_readlane(my_n, idp);
            const OrlgPathRec *cand = tb.recs + (base + idp);
            const double thr = gn[ORLG_GN_THR0 + (int)cand->se - 1];
            // candidate 0: the first fit below S - n (step_path_first_fit); candidate 1 + b: block b (step_deeprmsa).  Block 0
            // starts where the first fit starts unless the exclusive bound hides it: the same window, the same value
            int ff_s0 = -1;
            double ff_g = nan;
            for (int c = want_ff ? 0 : 1; c < (want_deep ? 1 + J : 1); ++c) {
                int len, s0;
                if (c == 0) s0 = first_fit<W>(x, n, S - n, lane);
                else s0 = find_block<W>(x, n, c - 1, lane, &len);
                s0 = uni(s0);
                double g = nan;
                if (s0 >= 0) {
                    if (c > 0 && s0 == ff_s0) g = ff_g;
                    else g = rmsa_gn_gsnr(wv, tb, gn, E, Q, 0, q_n, cand, s0, n);
                }
                const uint8_t ok = s0 >= 0 && g >= thr ? 1 : 0;
                if (c == 0) {
                    ff_s0 = s0; ff_g = g;
                    if (lane == 0) {
                        if (path_ff) path_ff[(size_t)env * ff_dim + idp] = ok;
                        if (path_ff_gsnr) path_ff_gsnr[(size_t)env * K + idp] = g;
                    }
                } else if (lane == 0) {
                    if (deeprmsa) deeprmsa[(size_t)env * deep_dim + idp * J + (c - 1)] = ok;
                    if (deep_gsnr) deep_gsnr[(size_t)env * K * J + idp * J + (c - 1)] = g;
                }
            }
        }
        if (lane == 0 && reject) {
            if (path_ff) path_ff[(size_t)env * ff_dim + K] = 1;
            if (deeprmsa) deeprmsa[(size_t)env * deep_dim + K * J] = 1;
        }
        wave_sync();
    }
}
