// orlg_gn_admission_kernels.hip -- valid-action masks and rule windows that know BOTH halves of the GN-model admission check, for the
// whole batch (include/orlg.h orlg_gn_admission_masks / orlg_gn_admission_windows).
//
// They describe the step the handle runs.  On a handle whose gate protects the running lightpaths (orlg_set_gn_protect)
// a bit is 1 iff the window exists, its own GSNR meets the threshold of the path's modulation AND no running service that shares a
// link with it falls below its own threshold once the candidate is lit -- !(margin < 0), the step's predicate; the margin row holds
// that smallest neighbour margin.  On a gated handle that does not protect the second check does not run: masks, windows and GSNR
// are those of orlg_gn_action_masks_kernel / orlg_gn_path_windows_kernel, byte for byte, and every margin is NaN.
//     path_ff   path p     <=>  orlg_step_gn_protect(PATH_FF_EXTERNAL, p): the first fit s in range(0, S - n)
//     deeprmsa  action a   <=>  orlg_step_gn_protect(DEEPRMSA_EXTERNAL, a): the first n slots of block a % j of route a // j
//     windows   path p     <=>  orlg_step_gn_protect(EXTERNAL, [p, slots[p]]): the window the rule proposes on p
// The windows come from the device functions the step calls (first_fit, find_block; assign_word_key / assign_key_slot; cut_word_key /
// cut_key_slot) on the lane layouts it calls them on; the own check is ONE call of rmsa_gn_gsnr per distinct window with the step's
// arguments; the neighbour check is victim-major (rmsa_gn_neighbour_margins, orlg_rmsa_gn_admission.h): the candidates of the request
// sit on lanes, at most 64 per pass, and every running service that meets one of them has its interferer sums walked once for all of
// them.  Both values have the bits of the step's gn_gsnr_db and gn_neighbour_margin_db.
//
// The shape of orlg_gn_action_masks_kernel: tables staged once per workgroup, one wave per environment at a time, the grid sized to
// the device and striding over the batch.  Per environment the occupancy row goes to LDS, and so does the LIVE part of the release
// ring's descriptors -- n_running entries from q_head, copied in ring order to positions 0 .. q_n, so that both routines walk them
// from head 0 in the chunks of 64 the step walks them in and never meet a wrap: the wave sums come out with the step's bits.  It
// reads state and writes only the caller's buffers.
#pragma once
#include "orlg_assign.h"
#include "orlg_cut.h"
#include "orlg_rmsa_gn_admission.h"
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// the per-wave LDS of both kernels (the occupancy row, then Q descriptors) and the scalars of the environment loop
struct OrlgGnAdmitWave {
    Wave wv;
    int q_n;   // live entries of the ring, linearised from head 0
};
DEV void gn_admit_wave(OrlgGnAdmitWave &aw, unsigned char *smem, const OrlgParams &p, int wib, int lane) {
    const int occ_bytes = (p.NW * 8 + 15) & ~15, q_bytes = (p.Q * 4 + 15) & ~15;
    unsigned char *wb = smem + p.l_shared_bytes + (size_t)wib * (occ_bytes + q_bytes);
    aw.wv = {};
    aw.wv.lane = lane;
    aw.wv.occ = reinterpret_cast<u64 *>(wb);
    aw.wv.qdesc = reinterpret_cast<uint32_t *>(wb + occ_bytes);
    aw.q_n = 0;
}
// the occupancy row and the live descriptors of environment `env` into the wave's LDS
DEV void gn_admit_load_env(OrlgGnAdmitWave &aw, const OrlgParams &p, int env, int lane) {
    const OrlgEnvScalars *sc = p.scal + env;
    const int Q = p.Q;
    const int q_head = uni(sc->q_head), n_run = uni(sc->n_running);
    const int q_n = n_run < Q ? (n_run < 0 ? 0 : n_run) : Q;   // (n_running also counts services an overflow lost)
    if ((p.NW & 1) == 0) copy_words(aw.wv.occ, p.occ + (size_t)env * p.NW, p.NW * 8, lane);
    else {
        const u64 *g = p.occ + (size_t)env * p.NW;
        for (int i = lane; i < p.NW; i += 64) aw.wv.occ[i] = g[i];
    }
    const uint32_t *g = p.qdesc + (size_t)env * Q;
    for (int i = lane; i < q_n; i += 64) {
        int pos = (q_head >= 0 && q_head < Q ? q_head : 0) + i;
        pos -= pos >= Q ? Q : 0;
        aw.wv.qdesc[i] = g[pos];
    }
    aw.q_n = q_n;
    wave_sync();
}

// path_ff: [B][K + reject] bytes, path_ff_gsnr / path_ff_margin: [B][K] doubles; deeprmsa: [B][K J + reject] bytes, deep_gsnr /
// deep_margin: [B][K J] doubles; any of them may be nullptr.  The rejection's column is always 1.  protect: the handle protects its
// running lightpaths.  LDS per wave: the occupancy row, then Q descriptors.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_gn_admission_masks_kernel(const OrlgParams p, uint8_t *path_ff,
                                                                                                      double *path_ff_gsnr, double *path_ff_margin,
                                                                                                      uint8_t *deeprmsa, double *deep_gsnr,
                                                                                                      double *deep_margin, int reject, int protect) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    OrlgGnAdmitWave aw;
    gn_admit_wave(aw, smem, p, wib, lane);
    const Wave &wv = aw.wv;
    const int N = p.N, K = p.K, S = p.S, J = p.j, Q = p.Q, E = p.E;
    const int LS = K <= 8 ? 8 : W;   // lanes from one candidate path to the next, as the step kernel lays them out
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const OrlgGnTable gn = ORLG_GPTR(const double, p.gn);
    const bool want_ff = path_ff || path_ff_gsnr || path_ff_margin, want_deep = deeprmsa || deep_gsnr || deep_margin;
    const int ff_dim = K + reject, deep_dim = K * J + reject;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = uni(sc->req_src), dst = uni(sc->req_dst), br = uni(sc->req_br);
        gn_admit_load_env(aw, p, env, lane);
        const int q_n = aw.q_n;
        const int base = tb.pair_base[src * N + dst];
        const int pp = LS == 8 ? lane >> 3 : lane / W, pw = lane - pp * LS;
        int se_l, hops_l;
        const u64 acc = path_word_rec<W>(wv.occ, tb.recs, base + pp, pw, pp < K && pw < W, se_l, hops_l);
        int my_se = 0;
        if (lane < K) my_se = tb.recs[base + lane].se;
        const int my_n = tb.nslots[br * ORLG_NSLOT_STRIDE + my_se];   // get_number_slots per candidate
        // the candidates in column order, path by path: [the first fit below S - n (path_ff_external)] [block 0 .. J - 1
        // (deeprmsa_external)]; at most 64 per pass, candidate i of the pass on lane i
        const int c_first = want_ff ? 0 : 1, per_path = (want_ff ? 1 : 0) + (want_deep ? J : 0), n_cols = K * per_path;
        int ff_s0 = -1;   // (block 0 starts where the first fit starts unless the exclusive bound hides it: the same window, the
        double ff_g = nan;   //  same GSNR)
        for (int col0 = 0; col0 < n_cols; col0 += 64) {
            const int n_here = n_cols - col0 < 64 ? n_cols - col0 : 64;
            int c_gid = 0, c_s = -1, c_n = 1, c_idp = 0, c_c = 0;
            double c_g = nan;
            bool c_pass = false;
            for (int i = 0; i < n_here; ++i) {
                const int idp = (col0 + i) / per_path, c = c_first + (col0 + i) - idp * per_path;
                u64 x[W];
#pragma unroll
                for (int w = 0; w < W; ++w) x[w] = readlane64(acc, idp * LS + w);
                const int n = __builtin_amdgcn_readlane(my_n, idp);
                const OrlgPathRec *cand = tb.recs + (base + idp);
                int len, s0;
                if (c == 0) s0 = first_fit<W>(x, n, S - n, lane);
                else s0 = find_block<W>(x, n, c - 1, lane, &len);
                s0 = uni(s0);
                double g = nan;
                if (s0 >= 0) {
                    if (c > 0 && s0 == ff_s0) g = ff_g;
                    else g = rmsa_gn_gsnr(wv, tb, gn, E, Q, 0, q_n, cand, s0, n);
                }
                if (c == 0) { ff_s0 = s0; ff_g = g; }   // (every path's candidates begin with c == 0 where the first fits are wanted)
                if (lane == i) {
                    c_gid = base + idp; c_s = s0; c_n = n; c_idp = idp; c_c = c; c_g = g;
                    c_pass = s0 >= 0 && g >= gn[ORLG_GN_THR0 + (int)cand->se - 1];
                }
            }
            double c_margin = nan;
            if (protect) c_margin = rmsa_gn_neighbour_margins(wv, tb, gn, E, q_n, c_pass, c_gid, c_s, c_n);
            if (lane < n_here) {
                const uint8_t ok = c_pass && !(c_margin < 0.0) ? 1 : 0;   // the step's own predicate: NaN refuses nothing
                if (c_c == 0) {
                    if (path_ff) path_ff[(size_t)env * ff_dim + c_idp] = ok;
                    if (path_ff_gsnr) path_ff_gsnr[(size_t)env * K + c_idp] = c_g;
                    if (path_ff_margin) path_ff_margin[(size_t)env * K + c_idp] = c_margin;
                } else {
                    const size_t o = (size_t)env * K * J + c_idp * J + (c_c - 1);
                    if (deeprmsa) deeprmsa[(size_t)env * deep_dim + c_idp * J + (c_c - 1)] = ok;
                    if (deep_gsnr) deep_gsnr[o] = c_g;
                    if (deep_margin) deep_margin[o] = c_margin;
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

// slots [B][K] int16, gsnr / margin [B][K] doubles, admitted [B][K] bytes; any of them may be nullptr.  rule and protect: wave-uniform
// (kernel arguments).  Two phases per environment, both in wave-uniform control flow: the windows of all paths, collected on lane p =
// path p (k <= 64), on the lane layouts of orlg_gn_path_windows_kernel; then the paths in turn through the checks.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_gn_admission_windows_kernel(const OrlgParams p, int rule, int16_t *slots,
                                                                                                        double *gsnr, double *margin,
                                                                                                        uint8_t *admitted, int protect) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    OrlgGnAdmitWave aw;
    gn_admit_wave(aw, smem, p, wib, lane);
    const Wave &wv = aw.wv;
    const int N = p.N, K = p.K, S = p.S, Q = p.Q, E = p.E;
    const int LS = K <= 8 ? 8 : W;   // lanes from one candidate path to the next, as the step kernel lays them out for its first fit
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const OrlgGnTable gn = ORLG_GPTR(const double, p.gn);
    const int g8 = lane >> 3, w8 = lane & 7;
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = uni(sc->req_src), dst = uni(sc->req_dst), br = uni(sc->req_br);
        gn_admit_load_env(aw, p, env, lane);
        const int q_n = aw.q_n;
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
        // ---- phase 2: every path's window through its own check, the value kept on lane p; then the neighbour check of all paths
        double my_g = __longlong_as_double(0x7ff8000000000000ll);
        bool my_pass = false;
        for (int idp = 0; idp < K; ++idp) {
            const int s0 = __builtin_amdgcn_readlane(my_slot, idp);
            const int n = __builtin_amdgcn_readlane(my_n, idp);
            const OrlgPathRec *cand = tb.recs + (base + idp);
            if (s0 >= 0) {
                const double g = rmsa_gn_gsnr(wv, tb, gn, E, Q, 0, q_n, cand, s0, n);
                if (lane == idp) { my_g = g; my_pass = g >= gn[ORLG_GN_THR0 + (int)cand->se - 1]; }
            }
        }
        double my_margin = __longlong_as_double(0x7ff8000000000000ll);
        if (protect) my_margin = rmsa_gn_neighbour_margins(wv, tb, gn, E, q_n, my_pass, base + (lane < K ? lane : 0), my_slot, my_n);
        if (lane < K) {
            const size_t o = (size_t)env * K + lane;
            if (slots) slots[o] = (int16_t)(my_slot >= 0 ? my_slot : S);
            if (gsnr) gsnr[o] = my_g;
            if (margin) margin[o] = my_margin;
            if (admitted) admitted[o] = my_pass && !(my_margin < 0.0) ? 1 : 0;   // the step's own predicate: NaN refuses nothing
        }
        wave_sync();
    }
}
