// orlg_gn_modulation_kernels.hip -- what every level of every candidate path gives the pending request on a handle whose gate chooses
// the modulation from the GSNR, for the whole batch (include/orlg.h orlg_gn_modulation_windows).
//
// For candidate path p and level m = 1..M, with no early exit: slot[p][m - 1] = the first fit of n_m on p (S = no window), gsnr = the
// GSNR of a service on that window against the services running now, each at its own stored level (NaN = no window), admitted = 1
// iff the window exists and its GSNR meets thresholds_db[m - 1] -- the outcome of orlg_step_modulation(ORLG_AM_EXTERNAL) with the
// action (p, slot, m); best_se[p] = the highest admitted level of p among the levels the step's walk visits (0 = none): what
// ORLG_AM_PATH_EXTERNAL provisions with action p.  The windows come from first_fit on the path-wide bitmap the step builds, every GSNR
// from rmsa_gn_gsnr_am with the arguments the step gives it (orlg_rmsa_gn_am.h): the value compared here has the bits of the value
// the step compares.  Two levels with the same n_m share window and GSNR, as in the step.
//
// The shape of orlg_gn_path_windows_kernel: tables staged once per workgroup, one wave per environment at a time, the grid striding
// over the batch, the occupancy row and the live descriptors of the release ring (linearised from head 0) in LDS.  Wave-uniform
// control flow.  It reads state and writes only the caller's buffers.
#pragma once
#include "orlg_rmsa_gn_am.h"
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// slot [B][K][M] int16, gsnr [B][K][M] doubles, admitted [B][K][M] bytes, best_se [B][K] bytes; any of them may be nullptr.
// LDS per wave: the occupancy row, then Q descriptors.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_gn_modulation_kernel(const OrlgParams p, int16_t *slot, double *gsnr,
                                                                                                 uint8_t *admitted, uint8_t *best_se) {
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
    const int N = p.N, K = p.K, S = p.S, Q = p.Q, E = p.E, M = p.gn_adaptive;
    const int LS = K <= 8 ? 8 : W;   // lanes from one candidate path to the next, as the step kernel lays them out
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const bool wide = (p.NW & 1) == 0;
    const OrlgGnTable gn = ORLG_GPTR(const double, p.gn);
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
        OrlgAmEntry first = {};
        if (q_n > 0) first = am_ring_entry(wv, tb, gn, E, Q, 0, q_n, 0);
        for (int idp = 0; idp < K; ++idp) {
            u64 x[W];
#pragma unroll
            for (int w = 0; w < W; ++w) x[w] = readlane64(acc, idp * LS + w);
            const OrlgPathRec *cand = tb.recs + (base + idp);
            int n_prev = -1, s_prev = -1, best = 0;
            double g_prev = nan;
            bool walk = true;   // the step's walk is still going: no level so far was admitted or without a window
            for (int m = M; m >= 1; --m) {
                const int n = uni((int)tb.nslots[br * ORLG_NSLOT_STRIDE + m]);
                if (n != n_prev) {
                    s_prev = uni(first_fit<W>(x, n, S - n, lane));
                    g_prev = s_prev >= 0 ? rmsa_gn_gsnr_am(wv, tb, gn, E, Q, 0, q_n, cand, s_prev, n, first) : nan;
                    n_prev = n;
                }
                const bool ok = s_prev >= 0 && uni((int)(g_prev >= gn[ORLG_GN_THR0 + m - 1])) != 0;
                if (walk && ok) best = m;
                walk = walk && s_prev >= 0 && !ok;
                if (lane == 0) {
                    const size_t o = ((size_t)env * K + idp) * M + (m - 1);
                    if (slot) slot[o] = (int16_t)(s_prev >= 0 ? s_prev : S);
                    if (gsnr) gsnr[o] = g_prev;
                    if (admitted) admitted[o] = ok ? 1 : 0;
                }
            }
            if (lane == 0 && best_se) best_se[(size_t)env * K + idp] = (uint8_t)best;
        }
        wave_sync();
    }
}
