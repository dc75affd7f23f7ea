// orlg_gn_slots_kernels.hip -- the GN-model admission check over the WHOLE spectrum, for the whole batch (include/orlg.h
// orlg_gn_admission_slots): for the pending request of every environment, every candidate path p and every start slot s
//     gsnr[p][s]    the GSNR the step would compare for the window [s, s + n) on p; NaN where there is no such free window
//     margin[p][s]  the neighbour margin of a protecting handle with that window lit; NaN where that check would not run
//     mask bit      window && gsnr >= thr && !(margin < 0): the step's predicate, the outcome of orlg_step_gn_protect(EXTERNAL, [p, s])
//     best_slot[p]  the lowest start among the admitted windows with the largest worst margin w = min(gsnr - thr, margin); S = none
// The outer shape is orlg_gn_admission_masks_kernel's: tables staged once per workgroup, one wave per environment striding over the
// batch, the occupancy row and the live descriptors of the release ring in LDS from head 0.  The evaluation of one path -- the lane
// layout of the two checks, the compaction, the band, the best window -- is orlg_gn_slots_path.h, which the max-margin policy section
// of the step kernel runs as well.
// It reads state and writes only the caller's buffers.  LDS per wave: the occupancy row, Q descriptors, Q compacted ranks.
#pragma once
#include "orlg_gn_admission_kernels.hip"
#include "orlg_gn_slots_path.h"

// mask: [B][K][W] words, bit s of word s / 64; gsnr / margin: [B][K][S] doubles; best_slot: [B][K] int16; best_margin: [B][K]
// doubles; any of them may be nullptr.  protect: the handle protects its running lightpaths (wave-uniform, a kernel argument).
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_gn_slots_kernel(const OrlgParams p, u64 *mask, double *gsnr, double *margin,
                                                                                            int16_t *best_slot, double *best_margin, int protect) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int occ_bytes = (p.NW * 8 + 15) & ~15, q_bytes = (p.Q * 4 + 15) & ~15;
    unsigned char *wb = smem + p.l_shared_bytes + (size_t)wib * (occ_bytes + 2 * q_bytes);
    OrlgGnAdmitWave aw;
    aw.wv = {};
    aw.wv.lane = lane;
    aw.wv.occ = reinterpret_cast<u64 *>(wb);
    aw.wv.qdesc = reinterpret_cast<uint32_t *>(wb + occ_bytes);
    aw.q_n = 0;
    uint32_t *cidx = reinterpret_cast<uint32_t *>(wb + occ_bytes + q_bytes);   // ranks of the services that meet the path
    const Wave &wv = aw.wv;
    const int N = p.N, K = p.K, S = p.S, Q = p.Q, E = p.E;
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const OrlgGnTable gn = ORLG_GPTR(const double, p.gn);
    const OrlgGnSlotsConst gk = gn_slots_const(gn);
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = uni(sc->req_src), dst = uni(sc->req_dst), br = uni(sc->req_br);
        gn_admit_load_env(aw, p, env, lane);
        const int q_n = aw.q_n;
        const int base = tb.pair_base[src * N + dst];
        u64 fit_l = 0ull;   // the free-start bitmaps of eight paths: path (idp & ~7) + g on the 8-lane group g, one word per lane
        for (int idp = 0; idp < K; ++idp) {
            if ((idp & 7) == 0) fit_l = gn_slots_fit8<W>(wv.occ, tb, base, idp, K, br, lane);
            const OrlgPathRec *rec = tb.recs + (base + idp);
            const int se = uni((int)rec->se);
            const int n = uni((int)tb.nslots[br * ORLG_NSLOT_STRIDE + se]);
            const size_t row = (size_t)env * K + idp;
            OrlgGnSlotsRows<W> r;
            gn_slots_path<W, false>(wv, tb, gn, gk, E, Q, 0, q_n, cidx, rec, n, fit_l, (idp & 7) << 3, protect, r);
            int first;
            double top;
            gn_slots_finish<W>(r, gn[ORLG_GN_THR0 + se - 1], S, lane, mask ? mask + row * W : nullptr, gsnr ? gsnr + row * S : nullptr,
                               margin ? margin + row * S : nullptr, best_slot || best_margin, first, top);
            if (lane == 0) {
                if (best_slot) best_slot[row] = (int16_t)first;
                if (best_margin) best_margin[row] = top;
            }
            wave_sync();   // (the next path compacts into the same offsets)
        }
        wave_sync();
    }
}
