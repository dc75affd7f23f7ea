// orlg_gn_rule_kernels.hip -- the window an assignment rule proposes on every candidate path, and what the GN-model admission
// check says to it, for the whole batch (include/orlg.h orlg_gn_path_windows).
//
// For candidate path p of the pending request: slots[p] = the start of the rule's window on p (S = the path has none), gsnr[p] =
// the GSNR of a service on that window against the services running now (NaN = no window), admitted[p] = 1 iff the window exists
// and its GSNR meets the threshold of p's spectral efficiency -- the outcome of orlg_step_rule_gn(PATH_FF_EXTERNAL, rule, check)
// with action p.  The rules: ORLG_ASSIGN_FIRST (the reference's first fit, what orlg_gn_action_masks' path_ff_gn looks at),
// FIRST_FULL, LAST, BEST, EXACT (orlg_assign.h) and the fewest-cuts window (orlg_cut.h; the device's ORLG_ASSIGN_MIN_CUT).
// The windows come from the device functions the step calls (first_fit; assign_word_key / assign_key_slot; cut_word_key /
// cut_key_slot) on the lane layouts it calls them on, and every GSNR from ONE call of rmsa_gn_gsnr with the arguments the step
// gives it: the value compared here has the bits of the value the step compares.
//
// The shape of orlg_gn_action_masks_kernel: tables staged once per workgroup, one wave per environment at a time, the grid striding
// over the batch, the occupancy row and the live descriptors of the release ring (linearised from head 0) in LDS.  Two phases per
// environment, both in wave-uniform control flow: the windows of all paths, eight paths per pass, collected on lane p = path p
// (k <= 64); then the paths in turn through the check.  It reads state and writes only the caller's buffers.
#pragma once
#include "orlg_assign.h"
#include "orlg_cut.h"
#include "orlg_rmsa_gn.h"
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// slots [B][K] int16, gsnr [B][K] doubles, admitted [B][K] bytes; any of them may be nullptr.  rule: wave-uniform (a kernel argument).
// LDS per wave: the occupancy row, then Q descriptors.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_gn_path_windows_kernel(const OrlgParams p, int rule, int16_t *slots,
                                                                                                   double *gsnr, uint8_t *admitted) {
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
    const int N = p.N, K = p.K, S = p.S, Q = p.Q, E = p.E;
    const int LS = K <= 8 ? 8 : W;   // lanes from one candidate path to the next, as the step kernel lays them out for its first fit
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const bool wide = (p.NW & 1) == 0;
    const OrlgGnTable gn = ORLG_GPTR(const double, p.gn);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int g8 = lane >> 3, w8 = lane & 7;
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
        int my_se = 0;
        if (lane < K) my_se = tb.recs[base + lane].se;
        const int my_n = tb.nslots[br * ORLG_NSLOT_STRIDE + my_se];   // get_number_slots per candidate
        // ---- phase 1: lane p = the start of the rule's window on path p, -1 = none
        int my_slot = -1;
        if (rule == ORLG_ASSIGN_FIRST) {
            // the first fit below S - n on the path-wide bitmap, as the step's path_ff_external finds it
            const int pp = LS == 8 ? lane >> 3 : lane / W, pw = lane - pp * LS;
            int se_l, hops_l;
            const u64 acc = path_word_rec<W>(wv.occ, tb.recs, base + pp, pw, pp < K && pw < W, se_l, hops_l);
            for (int idp = 0; idp < K; ++idp) {
                u64 x[W];
#pragma unroll
                for (int w = 0; w < W; ++w) x[w] = readlane64(acc, idp * LS + w);
                const int n = __builtin_amdgcn_readlane(my_n, idp);
                const int s0 = uni(first_fit<W>(x, n, S - n, lane));
                if (lane == idp) my_slot = s0;
            }
        } else {
            // eight paths per pass, path p0 + g on the 8-lane group g with one word per lane: wave_assign's and wave_cut_assign's layout
            for (int p0 = 0; p0 < K; p0 += 8) {
                const int idp = p0 + g8;
                const bool on = idp < K && w8 < W;
                int key, sl;
                if (rule == ORLG_ASSIGN_MIN_CUT) {
                    int hops_l, n;
                    u64 x;
                    key = group8_max((int)cut_word_key<W>(wv.occ, tb.recs, base + idp, w8, on, tb.nslots + br * ORLG_NSLOT_STRIDE, S, hops_l, n, x));
                    sl = cut_key_slot((uint32_t)key);
                } else {
                    int se_l, hops_l;
                    const u64 x = path_word_rec<W>(wv.occ, tb.recs, base + idp, w8, on, se_l, hops_l) & valid_mask(S, w8);
                    int n = 1;
                    if (on) n = tb.nslots[br * ORLG_NSLOT_STRIDE + se_l];
                    key = group8_max((int)assign_word_key<W>(x, n, w8, rule));
                    sl = assign_key_slot((uint32_t)key, rule);
                }
                sl = key ? sl : -1;
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const int s_g = __builtin_amdgcn_readlane(sl, g << 3);
                    if (lane == p0 + g && p0 + g < K) my_slot = s_g;
                }
            }
        }
        // ---- phase 2: every path's window through the check
        for (int idp = 0; idp < K; ++idp) {
            const int s0 = __builtin_amdgcn_readlane(my_slot, idp);
            const int n = __builtin_amdgcn_readlane(my_n, idp);
            const OrlgPathRec *cand = tb.recs + (base + idp);
            const double thr = gn[ORLG_GN_THR0 + (int)cand->se - 1];
            double g = nan;
            if (s0 >= 0) g = rmsa_gn_gsnr(wv, tb, gn, E, Q, 0, q_n, cand, s0, n);
            if (lane == 0) {
                const size_t o = (size_t)env * K + idp;
                if (slots) slots[o] = (int16_t)(s0 >= 0 ? s0 : S);
                if (gsnr) gsnr[o] = g;
                if (admitted) admitted[o] = s0 >= 0 && g >= thr ? 1 : 0;
            }
        }
        wave_sync();
    }
}
