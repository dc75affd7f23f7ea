// orlg_phy_kernels.hip -- gfx950 kernels of the QoT-aware (PhyRMSA) step() path, physical layer.
//
// Reference: optical_rl_gym/envs/phy_rmsa_env.py -- step :272-351, _provision_path :544-623, _provision_virtual_path
// :625-659, _service_acceptance :767-778, _release_path :781-861, _next_service :969-1017, is_channel_free :1029-1035,
// calculate_r_cut (modified) :1123-1193, calculate_r_spatial :1085-1108, _calculate_total_cuts :1195-1203,
// calculate_total_r_spatial :1110-1121, heuristics phy_aware_sapbm_rmsa :1254, phy_aware_bmff_rmsa :1317,
// phy_aware_bmfa_rmsa :1375, phy_aware_bmfa_rss_rmsa :1441, use_existing_channels :1650, sapff_rmsa :1676.
// Periodic defragmentation (step :355-417): phy_defragmentation, orlg_phy_defrag.h.  The data layout is orlg_phy_layout.h, the
// metrics orlg_phy_metrics.h, the virtual layer and the release queue orlg_phy_virtual.h, the GN gate orlg_phy_gn.h.
//
// Same execution model as orlg_kernels.hip: one wavefront per environment, the link x channel free bitmap
// (268 channels = 5 words per link) and the MT19937 state live in LDS for the whole launch.  The release queue
// (loads of 1400-4000 = that many running services) stays in HBM -- release times and 48-byte service records,
// touched on provision / release -- and only the releases of the near future are kept in a small LDS buffer
// (NearBuffer, orlg_phy_virtual.h): the per-wave LDS footprint decides how many environments a CU keeps resident.  The QoT gate is the reference's: modulation_level[pair row][channel][k-path] (0 = unusable,
// capacity = level x 100 Gb/s) read from HBM in [row][k-path][channel] order (coalesced over channels).
// Lanes are channels: lane l of word w owns channel 64w + l.
#pragma once
#include "../../include/orlg.h"   // ORLG_PHY_POLICY_*
#include "orlg_phy_defrag.h"
#include "orlg_phy_gn.h"
#include "orlg_requests.h"   // the ring's producers, orlg_env_rates
#include "orlg_sections.h"
#include "orlg_spectrum.h"   // path_word

// The step's sections (SEC(n) below) are written out in the kernel.  The forms tried as functions were compared with the parent's
// code (profiles/README.md, round 9): none gave the parent's instructions in every instantiation, and each piece says so where
// it stands, with its figures.
// DF: the instantiation that carries the periodic defragmentation (and the node-degree vectors of its cut metric); handles
// without it run the other one, whose registers are not shared with code they never execute
// GN: ... and the one that also carries the GN-model admission check (orlg_gn_gate)
// POL: the policy of the launch (ORLG_PHY_POLICY_*; launches that do not step run the EXTERNAL instantiation).  A compile-time
// policy turns the per-policy choices inside the channel loops (level as a sort key or not, which metric, first row or best
// row) into straight-line code: a wave of this kernel is bound by its own instruction latency, and every wave-uniform branch
// inside an unrolled word loop is a fetch bubble paid W times per candidate path.
// CONT: bit_rate_selection="continuous" -- arrivals from refill_requests_cont_t, the virtual layer's shares in float64
// (OrlgPhyParams::cs_f / svc_f) in the reference's order of operations; no defragmentation (refused at create time).
// TRACE: the handle replays a request trace (OrlgPhyParams::tr_*).  A template argument and not a test at run time, as in the
// group kernel: the instantiations that serve handles without a trace keep their register allocation to the number
template <int W, bool DF, bool GN, int POL, bool CONT = false, bool TRACE = false>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK, 4) void orlg_phy_kernel(const OrlgPhyParams p) {
    // the policy sorts channels by the RSS metric (floating point) instead of an integer key
    constexpr bool RSSP = POL == ORLG_PHY_POLICY_BMFA_RSS_METRIC || POL == ORLG_PHY_POLICY_FAFF_RSS;
    extern __shared__ __align__(16) unsigned char smem[];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(p.tables);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        const int n16 = p.tab_bytes >> 4;
        for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
#pragma unroll
        for (int i = 0; i < ORLG_PHY_NUM_OUTS; ++i)
            if ((int)threadIdx.x == i) reinterpret_cast<u64 *>(smem + p.l_outs)[i] = reinterpret_cast<u64>(p.outs[i]);
        if (threadIdx.x == 0) *reinterpret_cast<int *>(smem + p.l_mtstage + ORLG_MT_N * 4) = 0;   // the staging buffer's lock
        __syncthreads();
    }
    // one MT19937 staging buffer per workgroup, handed from wave to wave with a lock word (as orlg_rmsa_group_kernel): the
    // arrivals of an environment are generated 64 at a time (refill_requests) into a ring in HBM
    uint32_t *mt_lds = reinterpret_cast<uint32_t *>(smem + p.l_mtstage);
    int *mt_lock = reinterpret_cast<int *>(smem + p.l_mtstage + ORLG_MT_N * 4);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const PhyTab tb = make_phy_tab(smem, p);
    unsigned char *wb = smem + p.l_shared_bytes + (size_t)wib * p.l_wave_bytes;
    u64 *occ = reinterpret_cast<u64 *>(wb + p.l_occ);
    NearBuffer nb;
    nb.t = reinterpret_cast<double *>(wb + p.l_nbt);
    nb.qi = reinterpret_cast<uint16_t *>(wb + p.l_nbi);
    uint32_t *scratch = reinterpret_cast<uint32_t *>(wb + p.l_scratch);  // selection lists + per-channel doubles
    PhyWaveScalars *ws = reinterpret_cast<PhyWaveScalars *>(wb + p.l_wsc);

    const int E = p.E, C = p.C, K = p.K, N = p.N, NBR = p.NBR, Q = p.Q, NW = p.NW;
    SEC_DECL
    // work queue (as orlg_rmsa_kernel): long launches draw environments from the ticket counter (the next ticket is drawn
    // while the current environment runs), short ones stride statically
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const int n_static = n_waves < p.B ? n_waves : p.B;
    int env = (int)(blockIdx.x * (blockDim.x >> 6)) + wib;
    if (env >= p.B) return;
    uint32_t nxt_tk = 0;
    for (bool first = true;; first = false) {
    if (!first) {
        if (p.ticket_stride) {
            env += n_waves;
            if (env >= p.B) break;
        } else {
            const uint32_t tk = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt_tk) - p.ticket_base;
            if (tk >= (uint32_t)(p.B - n_static)) break;
            env = n_static + (int)tk;
        }
    }
    if (!p.ticket_stride && lane == 0) {
        const auto kq = kernarg_as<OrlgPhyParams>();
        nxt_tk = atomicAdd(kq->ticket, 1u);
    }
    OrlgPhySvc *grec = p.qrec + (size_t)env * Q;
    double *gq = p.qtime + (size_t)env * Q;   // release times, compact: entries 0..n_running-1 are live
    u64 *gsum = DF && p.qsum ? p.qsum + (size_t)env * Q : nullptr;        // side arrays of the records (defragmentation scans)
    uint32_t *gseq = DF && p.qseq ? p.qseq + (size_t)env * Q : nullptr;
    nb.n = 0;
    nb.horizon = -__longlong_as_double((long long)ORLG_INF_BITS);  // the first look at the queue rebuilds the buffer
    uint32_t *gcs = p.cs + (size_t)env * N * N * K * p.cs_len;
    uint8_t *gcs_n = p.cs_n + (size_t)env * N * N * K;
    u64 *gnv = p.use_nv ? reinterpret_cast<u64 *>(wb + p.l_nv) : nullptr;   // node-degree vectors of the cut metric
    static_assert(!(CONT && DF), "continuous bit rates without the periodic defragmentation");
    double *gcsf = CONT ? p.cs_f + (size_t)env * N * N * K * p.cs_len * 2 : nullptr;   // (used, free) of the channel_state entries
    double *gsvf = CONT ? p.svc_f + (size_t)env * Q * ORLG_PHY_MAX_CH : nullptr;      // service.channels[i][1] of the records

    SEC(1);  // state load
    // (written out: as a function that hands the running scalars back by reference, 568 differing lines of assembly over the four
    // instantiations of round 9, scratch unchanged; with them in a struct, scratch of <5,true,true,0> 448 -> 464 B)
    // ------------------------------------------------------------------ HBM -> LDS
    const OrlgPhyScalars *gs = p.scal + env;
    int n_running = gs->n_running;
    {
        const u64 *g = p.occ + (size_t)env * NW;
        for (int i = lane; i < NW; i += 64) occ[i] = g[i];
        if (lane < 8) ws->c[lane] = gs->c[lane];
        if (lane == 0) {
            ws->total_path_index = gs->total_path_index; ws->total_mod = gs->total_mod;
            ws->channels_accepted = gs->channels_accepted; ws->physical_accepted = gs->physical_accepted;
            ws->episodes_done = gs->episodes_done;
            ws->total_path_length = gs->total_path_length; ws->total_gsnr = gs->total_gsnr;
            ws->req_arrival = gs->req_arrival; ws->req_holding = gs->req_holding;
            ws->q_overflow = gs->q_overflow;
            ws->counted_moves = gs->counted_moves; ws->counted_moves_groom = gs->counted_moves_groom;
            ws->counted_defrag_cycles = gs->counted_defrag_cycles;
        }
    }
    int next_seq = gs->next_seq;
    OrlgPhyCand *gcand = p.cand ? p.cand + (size_t)env * p.cand_cap : nullptr;
    double current_time = gs->current_time;
    int req_src = gs->req_src, req_dst = gs->req_dst, req_br = gs->req_br, req_sid = gs->req_sid;
    int mt_idx = gs->mt_idx, new_service = gs->new_service;
    int ring_pos = gs->ring_pos, ring_cnt = gs->ring_cnt;
    int eproc = (int)gs->c[2];
    wave_sync();
    if (gnv && p.mode == ORLG_MODE_STEP) nv_build<W>(gnv, occ, tb.lnib, E, C, lane);

    int *sel_ch = reinterpret_cast<int *>(scratch);            // [16] selected channels
    int *sel_cap = reinterpret_cast<int *>(scratch) + 16;      // [16] their capacity (modulation level)
    int *sel_used = reinterpret_cast<int *>(scratch) + 32;     // [16] the share this service uses
    double *scratch_d = reinterpret_cast<double *>(scratch + 64);  // [W*64] per-channel doubles

    // per-step totals (number_cuts_total / rss_total_metric) kept incrementally over the launch when they are asked for
    MetricCache mc;
    mc.on = p.mode == ORLG_MODE_STEP && p.use_masks && p.cterm != nullptr &&
            (p.out_mask & ((1 << ORLG_PHY_OUT_CUTS) | (1 << ORLG_PHY_OUT_RSS))) != 0;
    mc.want_rss = (p.out_mask & (1 << ORLG_PHY_OUT_RSS)) != 0;
    mc.total_runs = 0;
    mc.cterm = p.cterm ? p.cterm + (size_t)env * p.cpad : nullptr;
    mc.lterm = (double __attribute__((address_space(3))) *)scratch_d;
    // the steps of this instantiation never touch scratch_d: the RSS terms stay there (a defragmentation cycle uses the scratch:
    // the terms go to the HBM array for its duration -- once in defrag_period steps instead of a round trip every step)
    constexpr bool LT = !RSSP;
    mc.sqrt_tab = tb.sqrt_tab; mc.E = E; mc.W = W;
    // (launches of few steps -- the gym views -- sum every step: a block of one step would cost more than its chain)
    mc.defer = LT && mc.on && mc.want_rss && p.rlog_t0 != nullptr && p.n_steps >= 16;
    mc.log_overflow = false; mc.nlog = 0; mc.stamp = 0; mc.t0 = 0; mc.env = env;
    if (mc.on) {
        double c0_unused, r0_unused;
        phy_column_metrics<W>(occ, tb.sqrt_tab, E, C, lane, scratch_d, true, mc.want_rss, true, c0_unused, r0_unused, mc.total_runs);
        if (mc.want_rss && !LT) {
            for (int ch = lane; ch < C; ch += 64) mc.cterm[ch] = scratch_d[ch];
            wave_sync();
        }
        if (mc.defer) {
            double *lt0 = p.rlog_t0 + (size_t)env * p.cpad;
#pragma unroll
            for (int w = 0; w < W; ++w) lt0[64 * w + lane] = scratch_d[64 * w + lane];
        }
    }

    // GN gate: threshold q of the modulation levels on lane q (+inf beyond the last), read once per environment
    double gn_thr_l = __longlong_as_double((long long)ORLG_INF_BITS);
    if (GN && p.gn_on && lane < p.gn_nthr) gn_thr_l = p.gn_thr[lane];
    ReleaseAhead ra;
    ra.q = -1; ra.rec = 0u;
    // the next ring entry, requested one step ahead: lanes 0, 1 inter-arrival time, lanes 2, 3 holding time, lane 4 the request
    // (lanes 8, 9: the inter-arrival time of the entry after it, for the look-ahead of the release loop)
    uint32_t pf_ring = 0u;
    bool pf_ring_ok = false, pf_next_ok = false;
    auto ring_fetch = [&]() {
        pf_ring_ok = ring_cnt > 0;
        pf_next_ok = ring_cnt > 1;
        if (pf_ring_ok) {
            const auto kq = kernarg_as<OrlgPhyParams>();
            const size_t ro = (size_t)env * ORLG_RING + ring_pos;
            const uint32_t *src = lane < 2 ? reinterpret_cast<const uint32_t *>(kq->ring_iat + ro) + lane
                                : lane < 4 ? reinterpret_cast<const uint32_t *>(kq->ring_ht + ro) + (lane - 2)
                                : lane < 8 ? kq->ring_req + ro : reinterpret_cast<const uint32_t *>(kq->ring_iat + ro + 1) + (lane - 8);
            if (lane < 5 || (pf_next_ok && (lane == 8 || lane == 9))) pf_ring = *src;
        }
    };
    if (p.mode == ORLG_MODE_STEP) ring_fetch();
    const int n_iter = p.mode == ORLG_MODE_STEP ? p.n_steps : 1;
    for (int t = 0; t < n_iter; ++t) {
        SEC(2);  // policy: virtual layer
        if (p.mode == ORLG_MODE_STEP) {
            // D of the lane's channels (cut metric): requested first, used after the virtual-layer check; it serves every candidate
            // path of the request.  (The fence: entries other lanes rewrote since the last look -- their stores are long done.)
            uint4 dv[W];
#pragma unroll
            for (int w = 0; w < W; ++w) dv[w] = make_uint4(0u, 0u, 0u, 0u);
            if (gnv && (POL == ORLG_PHY_POLICY_BMFA_CUT || POL == ORLG_PHY_POLICY_FAFF)) {
                nv_fence();
#pragma unroll
                for (int w = 0; w < W; ++w) dv[w] = nv_get(gnv, 64 * w + lane, C);
            }
            const int base = tb.pair_base[req_src * N + req_dst];
            const int row = tb.pair_row[req_src * N + req_dst];
            const int demand = CONT ? p.br_lower + req_br : tb.bit_rates[req_br];
            constexpr int policy = POL;
            int a_path = -2, nsel = 0;
            // continuous: the selection's float64 (used, free) shares, lane i = selected channel i (in registers: a per-wave LDS
            // array would cost the node-degree vectors their room on chip)
            double sh_u = 0.0, sh_f = 0.0;
            // requested now, used after the virtual-layer check as well: the modulation levels of the lane's channels on the K
            // candidate paths (one or two words per channel) and the paths' node records (lane 2 i, 2 i + 1: path i)
            uint32_t lvk[W];   // (a fifth path's levels are read where they are needed: K = 5 pays a wait, K <= 4 no registers)
            uint4 nvq = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int w = 0; w < W; ++w) lvk[w] = 0u;
            const uint32_t *mk_hi = p.mod_k + ((size_t)row * p.cpad + lane) * 2 + 1;
            if (!RSSP && policy != ORLG_PHY_POLICY_EXTERNAL) {
                const uint32_t *mk = p.mod_k + ((size_t)row * p.cpad + lane) * 2;
#pragma unroll
                for (int w = 0; w < W; ++w) lvk[w] = mk[128 * w];
                if (gnv && lane < 2 * K) nvq = p.nvrec[2 * base + lane];
            }

            if (policy == ORLG_PHY_POLICY_EXTERNAL) {
                const auto kp = kernarg_as<OrlgPhyParams>();
                a_path = uni(kp->act_path[env]);
                const int16_t *ac = kp->act_channels + (size_t)env * ORLG_PHY_MAX_CH;
                int raw = lane < ORLG_PHY_MAX_CH ? (int)ac[lane] : -1;
                nsel = popc64(ballot(raw >= 0));  // channels are the leading non-negative entries
                const int idp = a_path > 10 ? a_path - 20 : a_path;
                if (lane < nsel) {
                    const int c = raw & 0x1ff, u = (raw >> 9) & 0x1f;
                    int cap = (idp >= 0 && idp < K && c < C) ? (int)p.mod_t[(size_t)(row * K + idp) * p.cpad + c] : 0;
                    sel_ch[lane] = c; sel_cap[lane] = cap; sel_used[lane] = u ? u : cap;
                    if constexpr (CONT) {   // the tuple's (used, free) in float64 (act_share)
                        const double *as = kp->act_share + ((size_t)env * ORLG_PHY_MAX_CH + lane) * 2;
                        sh_u = as[0]; sh_f = as[1];
                    }
                }
                wave_sync();
            } else {
                // ---------------- the heuristics of phy_rmsa_env.py:1254-1737
                const bool faff = policy == ORLG_PHY_POLICY_FAFF || policy == ORLG_PHY_POLICY_FAFF_RSS;
                const bool bmfa = policy == ORLG_PHY_POLICY_BMFA_CUT || policy == ORLG_PHY_POLICY_BMFA_RSS_METRIC;
                const bool with_metric = bmfa || faff;
                const bool groom = bmfa ? (p.grooming != 0) : true;
                bool served = false;
                // (SEC(2) written out, both forms: as one function phy_use_existing<CONT> 11 603 differing lines, round 9; the two forms
                // over one loop, in place, 3 345 -- and every line of that loop chose between them)
                if (CONT && groom) {
                    // use_existing_channels (:1650-1673) on float64 shares: sum() is a sequential sum in list order from 0, the
                    // running unassigned_bitrate is a float once a share is taken off (it is not reset between k-paths)
                    double unassigned = (double)demand;
                    for (int idp = 0; idp < K && !served; ++idp) {
                        const int key = (req_src * N + req_dst) * K + idp;
                        const CsList l = cs_load(gcs, gcs_n, key, lane, p.cs_len);
                        const CsShares s = csf_load(gcsf, key, lane, l.n, p.cs_len);
                        double sum = 0.0;
                        for (int i = 0; i < l.n; ++i) sum += readlane_d(s.f, i);
                        if (sum >= unassigned / 100.0) {
                            for (int i = 0; i < l.n && nsel < ORLG_PHY_MAX_CH; ++i) {
                                const double f = readlane_d(s.f, i);
                                if (f > 0.0) {
                                    const uint32_t en = cs_get(l, i);
                                    unassigned -= f * 100.0;
                                    const bool last = unassigned <= 0.0;
                                    const double take = last ? f + unassigned / 100.0 : f, rest = last ? unassigned / -100.0 : 0.0;
                                    if (lane == 0) { sel_ch[nsel] = cs_ch(en); sel_cap[nsel] = cs_cap(en); sel_used[nsel] = 0; }
                                    if (lane == nsel) { sh_u = take; sh_f = rest; }
                                    nsel += 1;
                                    if (last) { a_path = idp + 20; served = true; break; }
                                }
                            }
                        }
                    }
                    if (!served) nsel = 0;
                } else if (groom) {
                    // use_existing_channels (:1650-1673): residual capacity on channels this (src, dst, k-path) already lights
                    int unassigned = demand;
                    for (int idp = 0; idp < K && !served; ++idp) {
                        const CsList l = cs_load(gcs, gcs_n, (req_src * N + req_dst) * K + idp, lane, p.cs_len);
                        int fr = lane < l.n ? cs_free(l.e) : 0;
                        const int sum = wave_add_i32(fr);
                        if (sum * 100 >= unassigned) {
                            for (int i = 0; i < l.n && nsel < ORLG_PHY_MAX_CH; ++i) {
                                const uint32_t en = cs_get(l, i);
                                const int f = cs_free(en);
                                if (f > 0) {
                                    unassigned -= f * 100;
                                    int take = f;
                                    if (unassigned <= 0) take = f + unassigned / 100;  // unassigned is a multiple of 100
                                    if (lane == 0) { sel_ch[nsel] = cs_ch(en); sel_cap[nsel] = cs_cap(en); sel_used[nsel] = take; }
                                    nsel += 1;
                                    if (unassigned <= 0) { a_path = idp + 20; served = true; break; }
                                }
                            }
                        }
                    }
                    if (!served) nsel = 0;
                }
                SEC(3);  // policy: row metrics  (SEC(3), (4) written out: as one function 37 338 differing lines, scratch of <3,false,false,6,true> 48 -> 64 B)
                if (!served) {
                    // per path ("row") the free channels ordered by (level desc, metric desc, channel asc)
                    //   bmfa / bmfa_rss: sorted(row, key=(-level, -metric)), row with the best head (level, metric)
                    //   bmff:            sorted(row, key=(-level, channel)),  row with the best head level (ties: lower index)
                    //   sapbm:           sorted(row, key=(-level, channel)),  first non-empty row
                    //   sapff:           sorted(row, key=channel),            first non-empty row
                    //   faff / faff_rss: sorted(row, key=-metric),            row with the best head metric (ties: lower index)
                    const int metric_mode = RSSP ? 1 : (policy == ORLG_PHY_POLICY_BMFA_CUT || policy == ORLG_PHY_POLICY_FAFF) ? 0 : 2;
                    const bool flat = policy == ORLG_PHY_POLICY_SAPFF || faff;  // the level is not a sort key
                    const bool first_row = policy == ORLG_PHY_POLICY_SAPFF || policy == ORLG_PHY_POLICY_SAPBM;
                    const int pp = lane / W, pw = lane - pp * W;
                    const u64 acc = path_word<W>(occ, tb.recs, base + pp, pw, pp < K);
                    if constexpr (!RSSP) {
                        // integer metric: one sortable key per channel (phy_row_keys)
                        int head_key[ORLG_PHY_MAX_K];
                        unsigned alive = 0;
                        // the row the first pick below will choose keeps its per-channel keys: no second pass
                        int keep_idp = -1, keep_key[W], keep_h = -1;
#pragma unroll
                        for (int w = 0; w < W; ++w) keep_key[w] = -1;
#pragma unroll
                        for (int idp = 0; idp < ORLG_PHY_MAX_K; ++idp) {
                            head_key[idp] = -1;
                            if (idp < K) {
                                int key[W];
                                phy_row_keys<W>(occ, tb, p, acc, idp, base + idp, p.mod_t + (size_t)(row * K + idp) * p.cpad, lane, metric_mode, flat, key, dv, lvk, mk_hi, nvq);
                                const int h = phy_keys_best<W>(key);
                                if (h >= 0) {
                                    head_key[idp] = h; alive |= 1u << idp;
                                    // the head's (level, metric): the key without its channel bits
                                    if (keep_idp < 0 || (!first_row && (h >> 9) > (keep_h >> 9))) {
                                        keep_idp = idp; keep_h = h;
#pragma unroll
                                        for (int w = 0; w < W; ++w) keep_key[w] = key[w];
                                    }
                                }
                            }
                        }
                        SEC(4);  // policy: channel selection
                        for (;;) {
                            int best = -1, bh = -1;
#pragma unroll
                            for (int idp = 0; idp < ORLG_PHY_MAX_K; ++idp)
                                if (idp < K && ((alive >> idp) & 1u)) {
                                    if (best < 0 || (!first_row && (head_key[idp] >> 9) > (bh >> 9))) { best = idp; bh = head_key[idp]; }
                                }
                            if (best < 0) break;
                            int key[W];
                            const uint8_t *mrow = p.mod_t + (size_t)(row * K + best) * p.cpad;
                            if (best == keep_idp) {
#pragma unroll
                                for (int w = 0; w < W; ++w) key[w] = keep_key[w];
                                keep_idp = -1;
                            } else {
                                phy_row_keys<W>(occ, tb, p, acc, best, base + best, mrow, lane, metric_mode, flat, key, dv, lvk, mk_hi, nvq);
                            }
                            int unassigned = demand;
                            nsel = 0;
                            bool covered = false;
                            int h = bh;   // the row's head is its first channel
                            while (nsel < ORLG_PHY_MAX_CH) {
                                if (h < 0) break;
                                const int c0 = 511 - (h & 511);
#pragma unroll
                                for (int w = 0; w < W; ++w) key[w] = key[w] == h ? -1 : key[w];
                                const int level = flat ? (int)mrow[c0] : (h >> 20);
                                unassigned -= level * 100;
                                const int used = unassigned <= 0 ? level + unassigned / 100 : level;
                                if (lane == 0) { sel_ch[nsel] = c0; sel_cap[nsel] = level; sel_used[nsel] = used; }
                                if (CONT && lane == nsel) {   // (channel, level + unassigned / 100, unassigned / -100, level): :1305-1308
                                    sh_u = unassigned <= 0 ? (double)level + (double)unassigned / 100.0 : (double)level;
                                    sh_f = unassigned <= 0 ? (double)unassigned / -100.0 : 0.0;
                                }
                                nsel += 1;
                                if (unassigned <= 0) { covered = true; break; }
                                h = phy_keys_best<W>(key);
                            }
                            if (covered) { a_path = best; break; }
                            alive &= ~(1u << best);  // sorted_free_channels.pop(row)
                            nsel = 0;
                        }
                    } else {
                        uint32_t cols[W];
                        double *r0w = scratch_d;   // free until the per-step outputs
                        phy_columns<W>(occ, tb, p, lane, metric_mode, cols, r0w);
                        int head_level[ORLG_PHY_MAX_K];
                        double head_metric[ORLG_PHY_MAX_K];
                        unsigned alive = 0;
                        // the row the first pick below will choose keeps its per-channel (level, metric) values: no second pass
                        int keep_idp = -1, keep_lv[W], keep_l = -1;
                        double keep_mt[W], keep_m = 0.0;
#pragma unroll
                        for (int w = 0; w < W; ++w) { keep_lv[w] = -1; keep_mt[w] = 0.0; }
#pragma unroll
                        for (int idp = 0; idp < ORLG_PHY_MAX_K; ++idp) {
                            head_level[idp] = -1; head_metric[idp] = 0.0;
                            if (idp < K) {
                                int lv[W];
                                double mtr[W];
                                phy_row_metrics<W>(occ, tb, p, acc, idp, base + idp, p.mod_t + (size_t)(row * K + idp) * p.cpad, lane, metric_mode, flat, lv, mtr, cols, r0w, dv);
                                int bl, bc;
                                double bm;
                                phy_row_best<W>(lv, mtr, lane, bl, bm, bc);
                                if (bl >= 0) {
                                    head_level[idp] = bl; head_metric[idp] = bm; alive |= 1u << idp;
                                    if (keep_idp < 0 || (!first_row && (bl > keep_l || (with_metric && bl == keep_l && bm > keep_m)))) {
                                        keep_idp = idp; keep_l = bl; keep_m = bm;
#pragma unroll
                                        for (int w = 0; w < W; ++w) { keep_lv[w] = lv[w]; keep_mt[w] = mtr[w]; }
                                    }
                                }
                            }
                        }
                        SEC(4);  // policy: channel selection
                        for (;;) {
                            int best = -1, bl = -1;
                            double bm = 0.0;
#pragma unroll
                            for (int idp = 0; idp < ORLG_PHY_MAX_K; ++idp)
                                if (idp < K && ((alive >> idp) & 1u)) {
                                    if (best < 0 || (!first_row && (head_level[idp] > bl ||
                                                                    (with_metric && head_level[idp] == bl && head_metric[idp] > bm)))) {
                                        best = idp; bl = head_level[idp]; bm = head_metric[idp];
                                    }
                                }
                            if (best < 0) break;
                            int lv[W];
                            double mtr[W];
                            const uint8_t *mrow = p.mod_t + (size_t)(row * K + best) * p.cpad;
                            if (best == keep_idp) {
#pragma unroll
                                for (int w = 0; w < W; ++w) { lv[w] = keep_lv[w]; mtr[w] = keep_mt[w]; }
                                keep_idp = -1;
                            } else {
                                phy_row_metrics<W>(occ, tb, p, acc, best, base + best, mrow, lane, metric_mode, flat, lv, mtr, cols, r0w, dv);
                            }
                            int unassigned = demand;
                            nsel = 0;
                            bool covered = false;
                            while (nsel < ORLG_PHY_MAX_CH) {
                                int l0, c0;
                                double m0;
                                phy_row_best<W>(lv, mtr, lane, l0, m0, c0);
                                if (l0 < 0) break;
#pragma unroll
                                for (int w = 0; w < W; ++w)
                                    if (64 * w + lane == c0) lv[w] = -1;
                                const int level = flat ? (int)mrow[c0] : l0;
                                unassigned -= level * 100;
                                const int used = unassigned <= 0 ? level + unassigned / 100 : level;
                                if (lane == 0) { sel_ch[nsel] = c0; sel_cap[nsel] = level; sel_used[nsel] = used; }
                                if (CONT && lane == nsel) {   // (channel, level + unassigned / 100, unassigned / -100, level): :1305-1308
                                    sh_u = unassigned <= 0 ? (double)level + (double)unassigned / 100.0 : (double)level;
                                    sh_f = unassigned <= 0 ? (double)unassigned / -100.0 : 0.0;
                                }
                                nsel += 1;
                                if (unassigned <= 0) { covered = true; break; }
                            }
                            if (covered) { a_path = best; break; }
                            alive &= ~(1u << best);  // sorted_free_channels.pop(row)
                            nsel = 0;
                        }
                
                    }
                }
                wave_sync();
            }

            SEC(5);  // provision  (both branches written out: as functions, the virtual one 11 315 differing lines, the physical one 13 065)
            bool accepted = false;
            double gn_last = __longlong_as_double(0x7ff8000000000000ll);   // NaN: no GN check in this step
            const bool dirbit = req_src > req_dst;
            if (a_path > 10 && a_path - 20 < K && nsel > 0) {
                // ---- virtual layer: _service_acceptance(True), _provision_virtual_path (:280-288, 625-659)
                const int idp = a_path - 20, gid = base + idp;
                const int key = (req_src * N + req_dst) * K + idp;
                CsList l = cs_load(gcs, gcs_n, key, lane, p.cs_len);
                bool ok = true;
                CsShares s{0.0, 0.0};
                if constexpr (CONT) s = csf_load(gcsf, key, lane, l.n, p.cs_len);
                for (int ci = 0; ci < nsel && ok; ++ci) {
                    const int q = cs_find(l, sel_ch[ci], lane);
                    if (q < 0) { ok = false; break; }
                    const uint32_t en = cs_get(l, q);
                    if constexpr (CONT) {   // (t[0], t[1] + channel[1], t[2] - channel[1], t[3]) when t[2] >= channel[1] (:640-644)
                        const double eu = readlane_d(s.u, q), ef = readlane_d(s.f, q), take = readlane_d(sh_u, ci);
                        if (!(ef >= take)) { ok = false; break; }
                        csf_remove(s, q, l.n, lane);
                        cs_remove(l, q, lane);
                        csf_append(s, eu + take, ef - take, l.n, l.cap, lane);
                        cs_append(l, cs_pack(cs_ch(en), 0, 0, cs_cap(en)), lane);
                        continue;
                    }
                    const int take = sel_used[ci];
                    if (cs_free(en) < take) { ok = false; break; }  // the reference raises here
                    cs_remove(l, q, lane);
                    cs_append(l, cs_pack(cs_ch(en), cs_used(en) + take, cs_free(en) - take, cs_cap(en)), lane);
                }
                if (ok) {
                    if constexpr (CONT) csf_store(gcsf, key, s, l.n, p.cs_len, lane);
                    cs_store(gcs, gcs_n, key, l, lane);
                    if (lane == 0) { ws->c[1] += 1; ws->c[3] += 1; ws->c[5] += demand; ws->c[7] += demand; }
                    accepted = true;
                    // _add_release, written out here and in the physical branch: as ONE function of (flags, lane's halfword, share) no
                    // shape gave the parent's code -- 39 342 to 53 626 differing lines of assembly over the four kernels, scratch of
                    // <5,true,true,0> 448 -> 416 B with the queue test inside and n_running / next_seq by reference (round 9)
                    if (n_running < Q) {
                        if (lane == 0) gq[n_running] = ws->req_arrival + ws->req_holding;
                        {
                            uint32_t hw_v = lane < nsel ? (uint32_t)(sel_ch[lane] | (sel_used[lane] << 9) | (1 << 14)) : 0xffffu;
                            if constexpr (CONT) {   // the share in svc_f; partial = channel[1] != channel[3] (_release_path :784)
                                if (lane < nsel) {
                                    hw_v = (uint32_t)(sel_ch[lane] | ((sh_u != (double)sel_cap[lane] ? 1 : 0) << 14));
                                    gsvf[(size_t)n_running * ORLG_PHY_MAX_CH + lane] = sh_u;
                                }
                            }
                            rec_store(grec + n_running, &ws->req_arrival, (uint32_t)next_seq, gid, nsel, 1 | (dirbit ? 2 : 0), hw_v, lane);
                            if (DF && gsum) svc_side_store(gsum, gseq, n_running, gid, 1 | (dirbit ? 2 : 0), nsel, hw_v, (uint32_t)next_seq, lane);
                        }
                        {   // _add_release: the release joins the near-term buffer when it falls before the horizon
                            const double rel = readlane_d(ws->req_arrival + ws->req_holding, 0);
                            const int qidx = n_running;
                            n_running += 1;
                            if (rel <= nb.horizon) {
                                if (nb.n < ORLG_PHY_NB) {
                                    if (lane == 0) { nb.t[nb.n] = rel; nb.qi[nb.n] = (uint16_t)qidx; }
                                    nb.n += 1;
                                } else {
                                    wave_sync();
                                    if (!nb_rebuild(nb, gq, n_running, current_time, phy_holding_lambda(p.holding_lambda, env), lane) && lane == 0) ws->q_overflow |= 8;
                                }
                            }
                        }
                        next_seq += 1;
                    } else if (lane == 0) {
                        ws->q_overflow |= 1;
                    }
                    wave_sync();
                }
            } else if (a_path >= 0 && a_path < K && nsel > 0) {
                const int gid = base + a_path;
                const OrlgPathRec *rec = tb.recs + gid;
                const int hops = rec->hops;
                // requested now, used after the checks: the GSNR of the chosen channels (lane i: channel i) and, when a channel is
                // only partly used, the channel_state list it will join
                const int cs_key_p = (req_src * N + req_dst) * K + a_path;
                const int my_ch = lane < nsel ? sel_ch[lane] : 0;
                const bool ch_ok = lane < nsel && my_ch >= 0 && my_ch < C;
                const double my_gsnr = ch_ok ? p.gsnr_t[(size_t)(row * K + a_path) * p.cpad + my_ch] : 0.0;
                const int my_used = lane < nsel ? sel_used[lane] : 0, my_cap = lane < nsel ? sel_cap[lane] : 0;
                // continuous: a channel joins channel_state when its free share is not 0 (channel[2] != 0, :600)
                const double my_uf = CONT && lane < nsel ? sh_u : 0.0, my_ff = CONT && lane < nsel ? sh_f : 0.0;
                const bool any_partial_p = ballot(lane < nsel && (CONT ? my_ff != 0.0 : my_used != my_cap)) != 0ull;
                CsList csl;
                csl.e = 0u; csl.n = 0; csl.cap = p.cs_len;
                if (any_partial_p) csl = cs_load(gcs, gcs_n, cs_key_p, lane, p.cs_len);
                CsShares csfl{0.0, 0.0};
                if (CONT && any_partial_p) csfl = csf_load(gcsf, cs_key_p, lane, csl.n, p.cs_len);
                // is_path_free_on_channels (:1019-1027): lanes = (channel, hop) pairs
                // (the heuristics pick among the channels that are free on the path right now: only external actions need the look)
                bool pass = true;
                if (policy == ORLG_PHY_POLICY_EXTERNAL) {
                    bool bad = false;
                    for (int i = lane; i < nsel * hops; i += 64) {
                        const int ci = i / hops, h = i - ci * hops;
                        const int ch = sel_ch[ci];
                        if (ch < 0 || ch >= C) { bad = true; } else {
                            bad = bad || !((occ[(int)rec->link[h] * W + (ch >> 6)] >> (ch & 63)) & 1ull);
                        }
                    }
                    pass = ballot(bad) == 0ull;
                }
                if (GN && p.gn_on && pass) {
                    // GN gate (not in the reference): every chosen channel must reach the level the table promised
                    const int mrow_g = (row * K + a_path) * p.cpad;
                    for (int ci = 0; ci < nsel && pass; ++ci) {
                        const double gdb = gn_gsnr<W>(p, occ, rec, mrow_g, sel_ch[ci], lane SEC_ARGS);
                        const int level = popc64(ballot(gdb >= gn_thr_l));   // thresholds reached (lane q: threshold q)
                        gn_last = gdb;
                        if (level < sel_cap[ci]) pass = false;
                    }
                }
                if (pass) {
                    // _provision_path (:544-623): one lane per hop clears the channels on its link
                    for (int ci = 0; ci < nsel; ++ci) mc_before(occ, mc, sel_ch[ci], lane);
                    {
                        u64 clr[W];   // the chosen channels as masks (wave-uniform): one read-modify-write per word and link
#pragma unroll
                        for (int w = 0; w < W; ++w) clr[w] = 0ull;
                        for (int ci = 0; ci < nsel; ++ci) {
                            const int ch = __builtin_amdgcn_readlane(my_ch, ci);
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                if ((ch >> 6) == w) clr[w] |= 1ull << (ch & 63);
                        }
                        if (lane < hops) {
                            u64 *rowp = occ + (int)rec->link[lane] * W;
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                if (clr[w] != 0ull) rowp[w] &= ~clr[w];
                        }
                    }
                    if (mc.on) {
                        wave_sync();
                        for (int ci = 0; ci < nsel; ++ci) mc_after<LT>(occ, mc, sel_ch[ci], lane);
                    }
                    if (gnv) {   // the nodes of the path lose free links on these channels
                        uint4 cv;
                        if (!RSSP && policy != ORLG_PHY_POLICY_EXTERNAL) {   // the pair's records are on lanes (nvq)
                            cv.x = (uint32_t)__builtin_amdgcn_readlane((int)nvq.x, 2 * a_path); cv.y = (uint32_t)__builtin_amdgcn_readlane((int)nvq.y, 2 * a_path);
                            cv.z = (uint32_t)__builtin_amdgcn_readlane((int)nvq.z, 2 * a_path); cv.w = (uint32_t)__builtin_amdgcn_readlane((int)nvq.w, 2 * a_path);
                        } else {
                            cv = p.nvrec[2 * gid];
                        }
                        if (lane < nsel) nv_update(gnv, cv, my_ch, false);
                    }
                    // statistics, in channel order (the GSNR sum is a float64 accumulation)
                    double tg = ws->total_gsnr;
                    for (int ci = 0; ci < nsel; ++ci) tg += readlane_d(my_gsnr, ci);
                    if (lane == 0) {
                        long long tm = ws->total_mod;
                        for (int ci = 0; ci < nsel; ++ci) tm += sel_cap[ci];
                        ws->total_gsnr = tg; ws->total_mod = tm;
                        ws->channels_accepted += nsel;
                        // _service_acceptance(False) (:767-778)
                        ws->c[1] += 1; ws->c[3] += 1; ws->c[5] += demand; ws->c[7] += demand;
                        ws->total_path_length += tb.path_len[gid];
                        ws->total_path_index += a_path + 1;
                        ws->physical_accepted += 1;
                    }
                    // (the loads above are consumed: from here on stores)
                    // partially used channels enter channel_state (:600-602)
                    if (any_partial_p) {
                        bool overflow = false;
                        for (int ci = 0; ci < nsel; ++ci) {
                            const int cap = sel_cap[ci], used = sel_used[ci];
                            if constexpr (CONT) {
                                const double ff = readlane_d(my_ff, ci);
                                if (ff != 0.0) {
                                    csf_append(csfl, readlane_d(my_uf, ci), ff, csl.n, csl.cap, lane);
                                    if (!cs_append(csl, cs_pack(sel_ch[ci], 0, 0, cap), lane)) overflow = true;
                                }
                                continue;
                            }
                            if (used != cap) {
                                if (!cs_append(csl, cs_pack(sel_ch[ci], used, cap - used, cap), lane)) overflow = true;
                            }
                        }
                        if constexpr (CONT) csf_store(gcsf, cs_key_p, csfl, csl.n, p.cs_len, lane);
                        cs_store(gcs, gcs_n, cs_key_p, csl, lane);
                        if (overflow && lane == 0) ws->q_overflow |= 4;
                    }
                    accepted = true;
                    // _add_release: compact queue, append at n_running
                    if (n_running < Q) {
                        if (lane == 0) gq[n_running] = ws->req_arrival + ws->req_holding;
                        {
                            uint32_t hw_p = lane < nsel ? (uint32_t)(my_ch | (my_used << 9) | ((my_used != my_cap ? 1 : 0) << 14)) : 0xffffu;
                            if constexpr (CONT) {
                                if (lane < nsel) {
                                    hw_p = (uint32_t)(my_ch | ((my_uf != (double)my_cap ? 1 : 0) << 14));
                                    gsvf[(size_t)n_running * ORLG_PHY_MAX_CH + lane] = my_uf;
                                }
                            }
                            rec_store(grec + n_running, &ws->req_arrival, (uint32_t)next_seq, gid, nsel, dirbit ? 2 : 0, hw_p, lane);
                            if (DF && gsum) svc_side_store(gsum, gseq, n_running, gid, dirbit ? 2 : 0, nsel, hw_p, (uint32_t)next_seq, lane);
                        }
                        {   // _add_release: the release joins the near-term buffer when it falls before the horizon
                            const double rel = readlane_d(ws->req_arrival + ws->req_holding, 0);
                            const int qidx = n_running;
                            n_running += 1;
                            if (rel <= nb.horizon) {
                                if (nb.n < ORLG_PHY_NB) {
                                    if (lane == 0) { nb.t[nb.n] = rel; nb.qi[nb.n] = (uint16_t)qidx; }
                                    nb.n += 1;
                                } else {
                                    wave_sync();
                                    if (!nb_rebuild(nb, gq, n_running, current_time, phy_holding_lambda(p.holding_lambda, env), lane) && lane == 0) ws->q_overflow |= 8;
                                }
                            }
                        }
                        next_seq += 1;
                    } else if (lane == 0) {
                        ws->q_overflow |= 1;
                    }
                    wave_sync();
                }
            }

            SEC(6);  // outputs  (written out: as a function 60 331 differing lines, scratch of <2,true,false,2> 256 -> 272 B)
            // per-step outputs
            if (p.out_mask) {
                const int om = p.out_mask;
                const size_t o = (size_t)t * p.B + env;
                double cuts = 0.0, rss = 0.0;
                const bool want_c = om & (1 << ORLG_PHY_OUT_CUTS), want_r = om & (1 << ORLG_PHY_OUT_RSS);
                if (mc.on) {
                    cuts = (double)mc.total_runs / (double)C;
                    if (want_r && mc.defer) {
                        mc.stamp += 1;   // this step's output point: its sum is formed with the block's (mc_flush, below)
                    } else if (want_r) {
                        // the terms lane 0 rewrote in this step are complete (same wave: in order).  Through LDS, then the
                        // reference's channel-order float64 sum: 8 terms per LDS round trip (one trip per term made this sum
                        // half of the step), the zero terms past C leave the sum as it is
                        nv_fence();
                        if (!LT) {
#pragma unroll
                            for (int w = 0; w < W; ++w) scratch_d[64 * w + lane] = 64 * w + lane < C ? mc.cterm[64 * w + lane] : 0.0;
                            wave_sync();
                        }
                        const double r = ordered_sum_lds(scratch_d, C);
                        wave_sync();
                        rss = r / (double)C;
                    }
                } else if (want_c || want_r) {
                    int tr_unused;
                    phy_column_metrics<W>(occ, tb.sqrt_tab, E, C, lane, scratch_d, want_c, want_r, p.use_masks != 0, cuts, rss, tr_unused);
                }
                if (om & (1 << ORLG_PHY_OUT_CHANNELS)) {
                    auto oc = ORLG_GPTR(int16_t, tb.outs[ORLG_PHY_OUT_CHANNELS]) + o * ORLG_PHY_MAX_CH;
                    if (lane < ORLG_PHY_MAX_CH) oc[lane] = lane < nsel ? (int16_t)sel_ch[lane] : (int16_t)-1;
                }
                if (om & (1 << ORLG_PHY_OUT_CH_USED)) {
                    auto oc = ORLG_GPTR(int16_t, tb.outs[ORLG_PHY_OUT_CH_USED]) + o * ORLG_PHY_MAX_CH;
                    // (continuous: the shares are not whole units -- 0 here, the float64 output carries them)
                    if (lane < ORLG_PHY_MAX_CH) oc[lane] = lane < nsel && !CONT ? (int16_t)sel_used[lane] : (int16_t)0;
                }
                if (lane == 0) {
                    if (om & (1 << ORLG_PHY_OUT_PATH)) ORLG_GPTR(int32_t, tb.outs[ORLG_PHY_OUT_PATH])[o] = a_path;
                    if (om & (1 << ORLG_PHY_OUT_NCH)) ORLG_GPTR(int32_t, tb.outs[ORLG_PHY_OUT_NCH])[o] = nsel;
                    if (om & (1 << ORLG_PHY_OUT_ACCEPTED)) ORLG_GPTR(uint8_t, tb.outs[ORLG_PHY_OUT_ACCEPTED])[o] = accepted ? 1 : 0;
                    if (om & (1 << ORLG_PHY_OUT_REQUEST))
                        ORLG_GPTR(orlg_v4i, tb.outs[ORLG_PHY_OUT_REQUEST])[o] = orlg_v4i{req_sid, req_src, req_dst, demand};
                    if (om & (1 << ORLG_PHY_OUT_ARRIVAL)) ORLG_GPTR(double, tb.outs[ORLG_PHY_OUT_ARRIVAL])[o] = ws->req_arrival;
                    if (om & (1 << ORLG_PHY_OUT_HOLDING)) ORLG_GPTR(double, tb.outs[ORLG_PHY_OUT_HOLDING])[o] = ws->req_holding;
                    if (om & (1 << ORLG_PHY_OUT_DEFRAG)) {  // the counters as the info dict sees them: before this step's defragmentation
                        auto od = ORLG_GPTR(int32_t, tb.outs[ORLG_PHY_OUT_DEFRAG]) + o * 3;
                        od[0] = ws->counted_moves; od[1] = ws->counted_moves_groom; od[2] = ws->counted_defrag_cycles;
                    }
                    if (om & (1 << ORLG_PHY_OUT_GN)) ORLG_GPTR(double, tb.outs[ORLG_PHY_OUT_GN])[o] = gn_last;
                    if (want_c) ORLG_GPTR(double, tb.outs[ORLG_PHY_OUT_CUTS])[o] = cuts;
                    if (want_r && !mc.defer) ORLG_GPTR(double, tb.outs[ORLG_PHY_OUT_RSS])[o] = rss;
                }
                // a block of deferred sums is due: 64 steps, or a log that the next step's rewrites might overrun
                if (mc.defer && (mc.stamp == 64 || mc.nlog > ORLG_RLOG_CAP - 160)) {
                    nv_fence();
                    mc_flush<W>(mc, scratch_d, reinterpret_cast<u64 *>(scratch), C, p.cpad, lane, tb.outs[ORLG_PHY_OUT_RSS], (size_t)p.B);
                    wave_sync();
                }
            }
            if constexpr (CONT) {   // the chosen channels' float64 (used, free): selected_channels[i][1], [i][2]
                if (p.out_share && lane < ORLG_PHY_MAX_CH) {
                    double *os = p.out_share + (((size_t)t * p.B + env) * ORLG_PHY_MAX_CH + lane) * 2;
                    os[0] = lane < nsel ? sh_u : 0.0;
                    os[1] = lane < nsel ? sh_f : 0.0;
                }
            }
            new_service = 0;
        } else if (p.mode == ORLG_MODE_EPISODE_RESET) {
            // reset(only_episode_counters=True) (phy_rmsa_env.py:426-472)
            eproc = new_service ? 1 : 0;
            if (lane == 0) {
                ws->c[2] = new_service ? 1 : 0; ws->c[3] = 0; ws->c[6] = new_service ? (CONT ? p.br_lower + req_br : tb.bit_rates[req_br]) : 0; ws->c[7] = 0;
                ws->total_path_length = 0.0; ws->total_gsnr = 0.0; ws->total_path_index = 0; ws->total_mod = 0;
                ws->channels_accepted = 0; ws->physical_accepted = 0;
                ws->counted_moves = 0; ws->counted_moves_groom = 0; ws->counted_defrag_cycles = 0;
            }
            wave_sync();
        }

        bool defrag_now = false;   // this step ends with a defragmentation cycle (services_processed % defrag_period == 0)
        SEC(7);  // next arrival  (SEC(7), (8) written out: as a function, ring_fetch one too, 45 601 differing lines, scratch unchanged)
        // ============================================================== _next_service (phy_rmsa_env.py:969-1017)
        if (p.mode != ORLG_MODE_EPISODE_RESET && !new_service) {
            // the arrival process does not depend on the network state: requests come from the ring of pre-generated arrivals
            // (five random() draws each, rmsa-style: phy_rmsa_env.py:971-986), refilled 64 at a time when it runs dry
            constexpr bool from_trace = TRACE;
            if (TRACE && ring_cnt == 0) {
                SEC(8);  // refill: the next requests of the trace -- no staging buffer, no lock, no generator state
                const auto kq = kernarg_as<OrlgPhyParams>();
                const int got = refill_requests_trace<false>(kq->tr_arrival, kq->tr_holding, kq->tr_req, kq->ring_iat + (size_t)env * ORLG_RING,
                                                             kq->ring_ht + (size_t)env * ORLG_RING, kq->ring_req + (size_t)env * ORLG_RING,
                                                             &mt_idx, kq->tr_len, env);
                ring_visible();
                ring_cnt = got; ring_pos = 0;
                SEC(7);
            } else if (ring_cnt == 0) {
                SEC(8);  // refill (the sequence of orlg_group_kernels.hip, written out in both: orlg_requests.h says why)
                static_assert(ORLG_MT_N * 4 == 156 * 16, "MT19937 state = 156 rows of 16 bytes");
                const auto kq = kernarg_as<OrlgPhyParams>();
                const uint4 *g_mt = reinterpret_cast<const uint4 *>(kq->mt + (size_t)env * ORLG_MT_N);
                uint4 *l_mt = reinterpret_cast<uint4 *>(mt_lds);
                uint4 m0 = g_mt[lane], m1 = g_mt[lane + 64], m2 = make_uint4(0u, 0u, 0u, 0u);
                if (lane < 156 - 128) m2 = g_mt[lane + 128];
                if (lane == 0) {
                    while (atomicCAS(mt_lock, 0, 1) != 0) __builtin_amdgcn_s_sleep(4);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                l_mt[lane] = m0; l_mt[lane + 64] = m1;
                if (lane < 156 - 128) l_mt[lane + 128] = m2;
                wave_sync();
                int idx_s = mt_idx;
                double arrival_lambda = p.arrival_lambda, holding_lambda = p.holding_lambda;
                orlg_env_rates(kq->rates, env, arrival_lambda, holding_lambda);   // (a sweep: the environment's own)
                const int got = CONT   // rng.randint(lower, higher) (phy_rmsa_env.py:127-129): the ring entry holds r, the rate is lower + r
                    ? refill_requests_cont<false>(mt_lds, kq->ring_iat + (size_t)env * ORLG_RING, kq->ring_ht + (size_t)env * ORLG_RING,
                                                  kq->ring_req + (size_t)env * ORLG_RING, tb.src_cum, tb.dst_cum, &idx_s, N, NBR,
                                                  arrival_lambda, holding_lambda)
                    : refill_requests<false>(mt_lds, kq->ring_iat + (size_t)env * ORLG_RING, kq->ring_ht + (size_t)env * ORLG_RING,
                                             kq->ring_req + (size_t)env * ORLG_RING, tb.src_cum, tb.dst_cum, tb.br_cum, &idx_s, N, NBR,
                                             arrival_lambda, holding_lambda, env);
                m0 = l_mt[lane]; m1 = l_mt[lane + 64];
                if (lane < 156 - 128) m2 = l_mt[lane + 128];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // this wave's reads of the buffer are done
                if (lane == 0) atomicExch(mt_lock, 0);
                uint4 *o_mt = reinterpret_cast<uint4 *>(kq->mt + (size_t)env * ORLG_MT_N);
                o_mt[lane] = m0; o_mt[lane + 64] = m1;
                if (lane < 156 - 128) o_mt[lane + 128] = m2;
                ring_visible();
                mt_idx = idx_s; ring_cnt = got; ring_pos = 0;
                SEC(7);
            }
            if (!pf_ring_ok) ring_fetch();   // the ring was empty when this step began (or the launch does not step)
            const double r_iat = __hiloint2double(__builtin_amdgcn_readlane((int)pf_ring, 1), __builtin_amdgcn_readlane((int)pf_ring, 0));
            const double ht = __hiloint2double(__builtin_amdgcn_readlane((int)pf_ring, 3), __builtin_amdgcn_readlane((int)pf_ring, 2));
            const uint32_t rq = (uint32_t)__builtin_amdgcn_readlane((int)pf_ring, 4);
            const bool have_next = pf_next_ok;
            const double next_iat = __hiloint2double(__builtin_amdgcn_readlane((int)pf_ring, 9), __builtin_amdgcn_readlane((int)pf_ring, 8));
            ring_pos += 1; ring_cnt -= 1;
            if (p.mode == ORLG_MODE_STEP) ring_fetch();   // the entry of the next step
            else pf_ring_ok = false;
            const double at = from_trace ? r_iat : current_time + r_iat;   // (a trace's ring holds the arrival time itself)
            current_time = at;
            const int src = (int)(rq & 0xffu), dst = (int)((rq >> 8) & 0xffu), bri = (int)(rq >> 16);
            req_sid = eproc;
            req_src = src; req_dst = dst; req_br = bri;
            new_service = 1;
            eproc += 1;
            if (lane == 0) {
                const int br_val = CONT ? p.br_lower + bri : tb.bit_rates[bri];
                ws->c[0] += 1; ws->c[2] += 1; ws->c[4] += br_val; ws->c[6] += br_val;
                ws->req_arrival = at; ws->req_holding = ht;
            }
            SEC(9);  // release: buffer / rebuild  (SEC(9), (10) written out: as a function 60 265 differing lines, scratch 448 / 48 / 256 -> 432 / 32 / 240 B)
            // ---- release every service with release time <= now in time order (:1009-1017, _release_path :781-861):
            // with the virtual layer the order of simultaneous releases decides who frees a shared channel
            wave_sync();
            if (current_time > nb.horizon) {
                if (!nb_rebuild(nb, gq, n_running, current_time, phy_holding_lambda(p.holding_lambda, env), lane) && lane == 0) ws->q_overflow |= 8;
            }
            // the scan looks one arrival ahead: the earliest release up to the NEXT arrival's time is this step's victim when it
            // is due now, and otherwise the service the next step will release first -- its record is requested right away
            // (ReleaseAhead; a defragmentation cycle in between drops the look-ahead)
            const double look_time = have_next ? (from_trace ? next_iat : current_time + next_iat) : current_time;
            int ahead_q = -1;
            for (;;) {
                int victim, vpos;
                double vt;
                nb_first_due(nb, look_time, lane, victim, vpos, vt);
                if (victim >= 0 && vt > current_time) { ahead_q = victim; victim = -1; }
                if (victim < 0) break;
                SEC(10);  // release apply
                const bool ahead = victim == ra.q;   // the service looked up at the start of the step: its data is here
                // the record stays on lanes (lane i < 12: dword i): no array of channels in private memory
                const uint32_t rv = ahead ? ra.rec : rec_dword(grec, victim, lane);
                const uint32_t d3 = (uint32_t)__builtin_amdgcn_readlane((int)rv, 3);
                const int sv_gid = (int)(d3 & 0xffffu), sv_nch = (int)((d3 >> 16) & 0xffu), sv_flags = (int)(d3 >> 24);
                // lane i < nch: channel i of the service (channel | used << 9 | partial << 14)
                const uint32_t pair_dw = (uint32_t)__shfl((int)rv, 4 + (lane >> 1));
                const int raw_l = lane < sv_nch ? (int)((pair_dw >> (16 * (lane & 1))) & 0xffffu) : 0;
                const OrlgPathRec *rec = tb.recs + sv_gid;
                const int pair = tb.path_pair[sv_gid];
                const int pa = pair / N, pb = pair - pa * N;
                const int ssrc = (sv_flags & 2) ? pb : pa, sdst = (sv_flags & 2) ? pa : pb;
                const int idp = sv_gid - tb.pair_base[pair];
                const int key = (ssrc * N + sdst) * K + idp;
                u64 freemask[W];  // channels to return on every link of the path
                const bool any_partial = ballot(lane < sv_nch && (raw_l & (1 << 14))) != 0ull;
#pragma unroll
                for (int w = 0; w < W; ++w) freemask[w] = 0ull;
                for (int ci = 0; ci < sv_nch; ++ci) {
                    const int raw = __builtin_amdgcn_readlane(raw_l, ci);
                    if (!(raw & (1 << 14))) {
                        const int ch = raw & 0x1ff;
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            if ((ch >> 6) == w) freemask[w] |= 1ull << (ch & 63);
                    }
                }
                // every load of this release first (what was not requested ahead), every store last
                const bool move_last = victim != n_running - 1;
                uint32_t lastv = 0u;   // the queue's last record (lanes 0..11) and release time (12, 13): it takes the victim's place
                if (move_last) {
                    lastv = lane < 12 ? reinterpret_cast<const uint32_t *>(grec + (n_running - 1))[lane]
                                      : lane < 14 ? reinterpret_cast<const uint32_t *>(gq + (n_running - 1))[lane - 12] : 0u;
                    if (DF && gsum) {   // its side-array entries travel with it (lanes 14, 15: summary; 16: seq)
                        if (lane == 14 || lane == 15) lastv = reinterpret_cast<const uint32_t *>(gsum + (n_running - 1))[lane - 14];
                        if (lane == 16) lastv = gseq[n_running - 1];
                    }
                }
                uint32_t cvl = 0u;
                if (gnv && lane < 4) cvl = reinterpret_cast<const uint32_t *>(p.nvrec + 2 * sv_gid)[lane];
                double mine_f = 0.0, last_f = 0.0;   // continuous: the victim's shares (lane i: channel i), the last record's
                if constexpr (CONT) {
                    if (lane < sv_nch) mine_f = gsvf[(size_t)victim * ORLG_PHY_MAX_CH + lane];
                    if (move_last && lane < ORLG_PHY_MAX_CH) last_f = gsvf[(size_t)(n_running - 1) * ORLG_PHY_MAX_CH + lane];
                }
                CsList l;
                l.e = 0u; l.n = 0; l.cap = p.cs_len;
                CsShares s{0.0, 0.0};
                if (any_partial) {
                    l = cs_load(gcs, gcs_n, key, lane, p.cs_len);
                    if constexpr (CONT) s = csf_load(gcsf, key, lane, l.n, p.cs_len);
                    for (int ci = 0; ci < sv_nch; ++ci) {
                        const int raw = __builtin_amdgcn_readlane(raw_l, ci);
                        if (!(raw & (1 << 14))) continue;
                        const int ch = raw & 0x1ff, mine = (raw >> 9) & 0x1f;
                        const int q = cs_find(l, ch, lane);
                        if (q < 0) continue;  // cannot happen for states produced by this kernel
                        const uint32_t en = cs_get(l, q);
                        if constexpr (CONT) {   // result[1] == channel[1]: dark; else (r0, r1 - c1, r2 + c1, r3) appended (:823-838)
                            const double eu = readlane_d(s.u, q), ef = readlane_d(s.f, q), mf = readlane_d(mine_f, ci);
                            csf_remove(s, q, l.n, lane);
                            cs_remove(l, q, lane);
                            if (eu == mf) {
#pragma unroll
                                for (int w = 0; w < W; ++w)
                                    if ((ch >> 6) == w) freemask[w] |= 1ull << (ch & 63);
                            } else {
                                csf_append(s, eu - mf, ef + mf, l.n, l.cap, lane);
                                cs_append(l, cs_pack(ch, 0, 0, cs_cap(en)), lane);
                            }
                            continue;
                        }
                        cs_remove(l, q, lane);
                        if (cs_used(en) == mine) {  // last user of the channel: it goes dark
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                if ((ch >> 6) == w) freemask[w] |= 1ull << (ch & 63);
                        } else {
                            cs_append(l, cs_pack(ch, cs_used(en) - mine, cs_free(en) + mine, cs_cap(en)), lane);
                        }
                    }
                }
                if (mc.on) {
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        for (u64 m = readlane64(freemask[w], 0); m; m &= m - 1) mc_before(occ, mc, 64 * w + ctz64(m), lane);
                }
                if (lane < rec->hops) {
                    u64 *rowp = occ + (int)rec->link[lane] * W;
#pragma unroll
                    for (int w = 0; w < W; ++w) rowp[w] |= freemask[w];
                }
                if (mc.on) {
                    wave_sync();
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        for (u64 m = readlane64(freemask[w], 0); m; m &= m - 1) mc_after<LT>(occ, mc, 64 * w + ctz64(m), lane);
                }
                if (gnv) {   // the returned channels: lane = channel of word w, the nodes of the path gain free links
                    uint4 cv_rel;
                    cv_rel.x = (uint32_t)__builtin_amdgcn_readlane((int)cvl, 0); cv_rel.y = (uint32_t)__builtin_amdgcn_readlane((int)cvl, 1);
                    cv_rel.z = (uint32_t)__builtin_amdgcn_readlane((int)cvl, 2); cv_rel.w = (uint32_t)__builtin_amdgcn_readlane((int)cvl, 3);
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        if (freemask[w] != 0ull && ((freemask[w] >> lane) & 1ull)) nv_update(gnv, cv_rel, 64 * w + lane, true);
                }
                // the stores: the rewritten channel_state list ...
                if (CONT && any_partial) csf_store(gcsf, key, s, l.n, p.cs_len, lane);
                if (any_partial) cs_store(gcs, gcs_n, key, l, lane);
                // ... and the swap-remove: the last live entry takes the victim's place (its near-buffer entry follows it) ...
                n_running -= 1;
                if (move_last) {
                    if (CONT && lane < ORLG_PHY_MAX_CH) gsvf[(size_t)victim * ORLG_PHY_MAX_CH + lane] = last_f;
                    if (lane < 12) reinterpret_cast<uint32_t *>(grec + victim)[lane] = lastv;
                    else if (lane < 14) reinterpret_cast<uint32_t *>(gq + victim)[lane - 12] = lastv;
                    else if (DF && gsum && lane < 16) reinterpret_cast<uint32_t *>(gsum + victim)[lane - 14] = lastv;
                    else if (DF && gsum && lane == 16) gseq[victim] = lastv;
                    for (int c0 = 0; c0 < nb.n; c0 += 64) {
                        const int c = c0 + lane;
                        if (c < nb.n && (int)nb.qi[c] == n_running) nb.qi[c] = (uint16_t)victim;
                    }
                }
                wave_sync();
                // ... and the victim's own buffer entry is replaced by the buffer's last one
                nb.n -= 1;
                if (vpos != nb.n && lane == 0) { nb.t[vpos] = nb.t[nb.n]; nb.qi[vpos] = nb.qi[nb.n]; }
                wave_sync();
                ra.q = -1;   // the queue has changed: what was looked up ahead is stale
            }
            ra.q = -1;
            if (DF && p.mode == ORLG_MODE_STEP && p.defrag_period > 0) defrag_now = uni((int)(ws->c[0] % p.defrag_period)) == 0;
            if (ahead_q >= 0 && !defrag_now && p.mode == ORLG_MODE_STEP) { ra.q = ahead_q; ra.rec = rec_dword(grec, ahead_q, lane); }
        }

        if (DF && p.mode == ORLG_MODE_STEP && p.defrag_period > 0) {
        SEC(11);  // defragmentation
            // periodic defragmentation (phy_rmsa_env.py:355-417): services_processed % defrag_period == 0
            wave_sync();
            if (__builtin_expect(defrag_now, 1)) {   // (most of the time of such a launch is spent in here: its loops get the registers)
                const bool park = LT && mc.on && mc.want_rss;
                if (park) {
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        if (64 * w + lane < C) mc.cterm[64 * w + lane] = scratch_d[64 * w + lane];
                    wave_sync();
                }
                phy_defragmentation<W>(p, tb, occ, ws, grec, gsum, gseq, gcs, gcs_n, gcand, sel_ch, scratch_d, n_running, next_seq, current_time, req_src, req_dst, lane, gnv, mc SEC_ARGS);
                if (park) {   // (the cycle's own updates went to the HBM array; the terms past C are zero: ordered_sum_lds)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
                    for (int w = 0; w < W; ++w) scratch_d[64 * w + lane] = 64 * w + lane < C ? mc.cterm[64 * w + lane] : 0.0;
                    wave_sync();
                }
            }
        }

        if (p.mode == ORLG_MODE_STEP) {
            const bool done = (eproc == p.episode_length);
            if (lane == 0 && (p.out_mask & (1 << ORLG_PHY_OUT_DONE)))
                ORLG_GPTR(uint8_t, tb.outs[ORLG_PHY_OUT_DONE])[(size_t)t * p.B + env] = done ? 1 : 0;
            if (done && p.auto_reset) {
                eproc = 1;
                if (lane == 0) {
                    ws->episodes_done += 1;
                    ws->c[2] = 1; ws->c[3] = 0; ws->c[6] = CONT ? p.br_lower + req_br : tb.bit_rates[req_br]; ws->c[7] = 0;
                    ws->total_path_length = 0.0; ws->total_gsnr = 0.0; ws->total_path_index = 0; ws->total_mod = 0;
                    ws->channels_accepted = 0; ws->physical_accepted = 0;
                    ws->counted_moves = 0; ws->counted_moves_groom = 0; ws->counted_defrag_cycles = 0;
                }
                wave_sync();
            }
        }
    }

    if (mc.defer) {   // the last block's sums
        wave_sync();
        if (mc.stamp > 0) mc_flush<W>(mc, scratch_d, reinterpret_cast<u64 *>(scratch), C, p.cpad, lane, tb.outs[ORLG_PHY_OUT_RSS], (size_t)p.B);
        if (mc.log_overflow && lane == 0) ws->q_overflow |= 16;
        wave_sync();
    }
    SEC(13);  // state store
    // (written out: as a function of the running scalars by value it gave the parent's code in 478 of the 480 instantiations;
    // <1,false,true,0,true> and <1,false,true,1,true> differed in two instructions each, registers and scratch unchanged: round 9)
    // ------------------------------------------------------------------ LDS -> HBM
    wave_sync();
    {
        const auto kp = kernarg_as<OrlgPhyParams>();
        u64 *g = kp->occ + (size_t)env * NW;
        for (int i = lane; i < NW; i += 64) g[i] = occ[i];
        OrlgPhyScalars *go = kp->scal + env;
        if (lane < 8) go->c[lane] = ws->c[lane];
        if (lane == 0) {
            go->current_time = current_time;
            go->req_arrival = ws->req_arrival; go->req_holding = ws->req_holding;
            go->total_path_length = ws->total_path_length; go->total_gsnr = ws->total_gsnr;
            go->total_path_index = ws->total_path_index; go->total_mod = ws->total_mod;
            go->channels_accepted = ws->channels_accepted; go->physical_accepted = ws->physical_accepted;
            go->episodes_done = ws->episodes_done;
            go->n_running = n_running;
            go->req_src = req_src; go->req_dst = req_dst; go->req_br = req_br; go->req_sid = req_sid;
            go->mt_idx = mt_idx; go->new_service = new_service; go->q_overflow = ws->q_overflow;
            go->ring_pos = ring_pos; go->ring_cnt = ring_cnt;
            if (ws->q_overflow) *kp->err_flag = 1;   // reported by the next entry point that waits for the stream
            go->next_seq = next_seq; go->counted_moves = ws->counted_moves; go->counted_moves_groom = ws->counted_moves_groom;
            go->counted_defrag_cycles = ws->counted_defrag_cycles;
        }
    }
    wave_sync();
    SEC(0);
    }  // work queue
    SEC_FLUSH;
}
