// orlg_gn_slots_kernels.hip -- the GN-model admission check over the WHOLE spectrum, for the whole batch (include/orlg.h
// orlg_gn_admission_slots): for the pending request of every environment, every candidate path p and every start slot s
//     gsnr[p][s]    the GSNR the step would compare for the window [s, s + n) on p; NaN where there is no such free window
//     margin[p][s]  the neighbour margin of a protecting handle with that window lit; NaN where that check would not run
//     mask bit      window && gsnr >= thr && !(margin < 0): the step's predicate, the outcome of orlg_step_gn_protect(EXTERNAL, [p, s])
//     best_slot[p]  the lowest start among the admitted windows with the largest worst margin w = min(gsnr - thr, margin); S = none
// The outer shape is orlg_gn_admission_masks_kernel's: tables staged once per workgroup, one wave per environment striding over the
// batch, the occupancy row and the live descriptors of the release ring in LDS from head 0.  What is new is the lane layout of the
// two checks.  The GSNR of a candidate depends on its start only through its centre frequency, so START SLOTS sit on lanes, 64 to
// a chunk, and the running services are walked wave-uniformly:
//     own check        the services that share a link with the path are compacted once per path (their ring offsets, in ring
//                      order, in LDS).  Per chunk with a free start, per such service: the two asinh and phi_mod (b_i / |df|) 5/3
//                      once per lane, added into one accumulator per hop of the path where the service's path holds the hop's
//                      link -- a wave-uniform test of a 14-bit hop mask; only l_eff / L differs between the hops.  Then the span
//                      sums and 10 log10 as rmsa_gn_gsnr has them.  A lane sums in ring order, the step by a wave reduction per
//                      64 ring entries: ~1e-15 relative.  A window whose GSNR - threshold comes out within ORLG_GN_SLOTS_BAND_DB
//                      of zero is evaluated again by rmsa_gn_gsnr itself, so that the bit is the step's.
//     neighbour check  victim-major (rmsa_gn_neighbour_margins, orlg_rmsa_gn_admission.h) with the start slots as the candidates:
//                      the victims of every window of a path are the compacted services; each one's interferer sums are walked
//                      ONCE per path, on the step's chunks of the ring, then every chunk that holds a window that passed its own
//                      check adds the candidate's term behind the wave sums, finishes the GSNR and updates the lane's minimum with
//                      the step's rule in rank order: the margin has the step's bits and needs no band.
// It reads state and writes only the caller's buffers.  LDS per wave: the occupancy row, Q descriptors, Q compacted offsets.
#pragma once
#include "orlg_gn_admission_kernels.hip"

#define ORLG_GN_SLOTS_BAND_DB 1e-9

// the value of chunk c of a per-lane array of W doubles, c wave-uniform: a chain of selects on constant indices (an array indexed
// by a loop variable would live in scratch)
template <int W>
DEV double gn_slots_get(const double (&a)[W], int c) {
    double v = a[0];
#pragma unroll
    for (int w = 1; w < W; ++w) v = w == c ? a[w] : v;
    return v;
}
template <int W>
DEV void gn_slots_set(double (&a)[W], int c, double v) {
#pragma unroll
    for (int w = 0; w < W; ++w) a[w] = w == c ? v : a[w];
}

// The interferer sums of the running service at ring offset vj (record `rec`, window [s, s + n)) over the OTHER running services:
// the ring walk of rmsa_gn_victim_gsnr up to its candidate, as rmsa_gn_neighbour_margins repeats it -- lane h = hop h of the victim,
// one wave sum per hop per 64 ring entries.  Hands back the links' constants of the victim's hops on the same lanes.
DEV double gn_slots_victim_sums(const Wave &wv, const Tab &tb, OrlgGnTable gn, bool wide, int q_n, int vj, const OrlgPathRec *rec, int hops,
                                double fc, double &lk_leff, double &lk_ratio, double &lk_e1, int &lk_spans, int &my_link) {
    const double beta_2 = -21.3e-27, pi = 3.141592653589793;
    const int lane = wv.lane;
    const double f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT], l_eff_a = gn[ORLG_GN_LEFF_A];
    my_link = (int)rec->link[lane < hops ? lane : 0];
    lk_leff = gn[ORLG_GN_LINK0 + 4 * my_link];
    lk_ratio = gn[ORLG_GN_LINK0 + 4 * my_link + 1];
    lk_e1 = gn[ORLG_GN_LINK0 + 4 * my_link + 2];
    lk_spans = (int)gn[ORLG_GN_LINK0 + 4 * my_link + 3];
    double sp = 0.0;   // lane h: interferer sum of hop h
    for (int j0 = 0; j0 < q_n; j0 += 64) {
        const bool valid = j0 + lane < q_n && j0 + lane != vj;
        const uint32_t d = wv.qdesc[j0 + lane < q_n ? j0 + lane : 0];
        const OrlgPathRec ri = tb.recs[d & 0x3fffu];
        const int s_i = (int)((d >> 14) & 0x3ffu), n_i = (int)tb.nslots[(d >> 24) * ORLG_NSLOT_STRIDE + ri.se];
        u64 m0, m1, m2, m3;
        rmsa_gn_link_mask_of(ri, wide, m0, m1, m2, m3);
        const double sb = (double)n_i * slot, sf = f0 + ((double)s_i + 0.5 * (double)n_i) * slot;
        const double df = valid ? sf - fc : slot;   // (windows on a shared link are disjoint: df != 0 where it is used)
        const double pm = rmsa_gn_phi_mod((int)ri.se);
        const double A = asinh(pi * pi * fabs(beta_2) * l_eff_a * sb * (df + (sb / 2))) -
                         asinh(pi * pi * fabs(beta_2) * l_eff_a * sb * (df - (sb / 2)));
        const double B = pm * (sb / fabs(df)) * 5 / 3;
        for (int h = 0; h < hops; ++h) {
            const int l = uni((int)rec->link[h]), w = l >> 6;
            const u64 m = w == 0 ? m0 : w == 1 ? m1 : w == 2 ? m2 : m3;
            const bool lit = valid && ((m >> (l & 63)) & 1ull);
            const double tot = wave_add_f64(lit ? A - (B * readlane_d(lk_ratio, h)) : 0.0);
            if (lane == h) sp += tot;
        }
    }
    return sp;
}

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
    uint32_t *cidx = reinterpret_cast<uint32_t *>(wb + occ_bytes + q_bytes);   // ring offsets of the services that meet the path
    const Wave &wv = aw.wv;
    const int N = p.N, K = p.K, S = p.S, Q = p.Q, E = p.E;
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const OrlgGnTable gn = ORLG_GPTR(const double, p.gn);
    const bool wide = E > 64;
    const int g8 = lane >> 3, w8 = lane & 7;
    const double beta_2 = -21.3e-27, gamma = 1.3e-3, h_plank = 6.626e-34, pi = 3.141592653589793;
    const double density = gn[ORLG_GN_DENSITY], f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT], att = gn[ORLG_GN_ATT];
    const double nf = gn[ORLG_GN_NF], l_eff_a = gn[ORLG_GN_LEFF_A];
    const double nan = __longlong_as_double(0x7ff8000000000000ll), ninf = __longlong_as_double((long long)0xfff0000000000000ull);
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = uni(sc->req_src), dst = uni(sc->req_dst), br = uni(sc->req_br);
        gn_admit_load_env(aw, p, env, lane);
        const int q_n = aw.q_n;
        const int base = tb.pair_base[src * N + dst];
        u64 fit_l = 0ull;   // the free-start bitmaps of eight paths: path (idp & ~7) + g on the 8-lane group g, one word per lane
        for (int idp = 0; idp < K; ++idp) {
            if ((idp & 7) == 0) {   // orlg_action_masks_kernel's "slots" words, by its device functions on its lane layout
                const int ip = idp + g8;
                const bool on = ip < K && w8 < W;
                int se_l, hops_l;
                const u64 xw = path_word_rec<W>(wv.occ, tb.recs, base + ip, w8, on, se_l, hops_l);
                int n_l = 1;
                if (on) n_l = tb.nslots[br * ORLG_NSLOT_STRIDE + se_l];
                fit_l = run_starts<W>(xw, n_l, w8);
            }
            const OrlgPathRec *rec = tb.recs + (base + idp);
            const int hops = uni((int)rec->hops), se = uni((int)rec->se);
            const int n = uni((int)tb.nslots[br * ORLG_NSLOT_STRIDE + se]);
            const double thr = gn[ORLG_GN_THR0 + se - 1];
            const size_t row = (size_t)env * K + idp;
            // the links' constants of the path's hops: lane h = hop h, read back per hop by readlane
            const int my_link = (int)rec->link[lane < hops ? lane : 0];
            const double lk_leff = gn[ORLG_GN_LINK0 + 4 * my_link], lk_ratio = gn[ORLG_GN_LINK0 + 4 * my_link + 1];
            const double lk_e1 = gn[ORLG_GN_LINK0 + 4 * my_link + 2];
            const int lk_spans = (int)gn[ORLG_GN_LINK0 + 4 * my_link + 3];
            const double bw = (double)n * slot, pw = density * bw;
            const double c_pm = rmsa_gn_phi_mod(se);
            u64 c0, c1, c2, c3;   // the path's links
            rmsa_gn_link_mask_of(*rec, wide, c0, c1, c2, c3);
            u64 any_free = 0ull;
#pragma unroll
            for (int w = 0; w < W; ++w) any_free |= readlane64(fit_l, ((idp & 7) << 3) + w);
            // ---- the running services that share a link with the path, compacted in ring order: the interferers of every window of
            // the path, and the victims of every one of them
            int n_c = 0;
            if (any_free) {
                for (int j0 = 0; j0 < q_n; j0 += 64) {
                    const bool valid = j0 + lane < q_n;
                    const uint32_t d = wv.qdesc[valid ? j0 + lane : 0];
                    u64 m0, m1, m2, m3;
                    rmsa_gn_link_mask_of(tb.recs[d & 0x3fffu], wide, m0, m1, m2, m3);
                    const bool hit = valid && ((m0 & c0) | (m1 & c1) | (m2 & c2) | (m3 & c3)) != 0ull;
                    const u64 hb = ballot(hit);
                    if (hit) cidx[n_c + popc64(hb & ((1ull << lane) - 1ull))] = (uint32_t)(j0 + lane);
                    n_c += popc64(hb);
                }
                wave_sync();
            }
            // ---- own check: lanes = start slots, the compacted services walked wave-uniformly
            double own[W], worst[W];
            u64 pass_l = 0ull;   // lane c: the starts of chunk c that passed their own check
#pragma unroll
            for (int w = 0; w < W; ++w) { own[w] = nan; worst[w] = nan; }
            for (int c = 0; c < W; ++c) {
                const u64 xc = readlane64(fit_l, ((idp & 7) << 3) + c);
                if (!xc) continue;
                const bool free_l = (xc >> lane) & 1ull;
                const double fc = f0 + ((double)(64 * c + lane) + 0.5 * (double)n) * slot;
                double acc[ORLG_MAX_HOPS];
#pragma unroll
                for (int h = 0; h < ORLG_MAX_HOPS; ++h) acc[h] = 0.0;
                for (int i0 = 0; i0 < n_c; i0 += 64) {
                    // 64 interferers on lanes: bandwidth, centre, phi_mod, and the hops of the path whose link the interferer's path holds
                    const uint32_t d = wv.qdesc[cidx[i0 + lane < n_c ? i0 + lane : 0]];
                    const OrlgPathRec ri = tb.recs[d & 0x3fffu];
                    const int s_i = (int)((d >> 14) & 0x3ffu), n_i = (int)tb.nslots[(d >> 24) * ORLG_NSLOT_STRIDE + ri.se];
                    u64 m0, m1, m2, m3;
                    rmsa_gn_link_mask_of(ri, wide, m0, m1, m2, m3);
                    const double sb_l = (double)n_i * slot, sf_l = f0 + ((double)s_i + 0.5 * (double)n_i) * slot;
                    const double pm_l = rmsa_gn_phi_mod((int)ri.se);
                    int hm_l = 0;
                    for (int h = 0; h < hops; ++h) {
                        const int l = __builtin_amdgcn_readlane(my_link, h), w = l >> 6;
                        const u64 m = w == 0 ? m0 : w == 1 ? m1 : w == 2 ? m2 : m3;
                        hm_l |= (int)((m >> (l & 63)) & 1ull) << h;
                    }
                    const int cnt = n_c - i0 < 64 ? n_c - i0 : 64;
                    for (int b = 0; b < cnt; ++b) {
                        const double sb = readlane_d(sb_l, b), sf = readlane_d(sf_l, b), pm = readlane_d(pm_l, b);
                        const int hm = __builtin_amdgcn_readlane(hm_l, b);
                        const double df = sf - fc;   // (a free window is disjoint from the interferer's on the link they share: df != 0 where it is used)
                        const double A = asinh(pi * pi * fabs(beta_2) * l_eff_a * sb * (df + (sb / 2))) -
                                         asinh(pi * pi * fabs(beta_2) * l_eff_a * sb * (df - (sb / 2)));
                        const double Bt = pm * (sb / fabs(df)) * 5 / 3;
#pragma unroll
                        for (int h = 0; h < ORLG_MAX_HOPS; ++h)
                            if ((hm >> h) & 1) acc[h] += A - (Bt * readlane_d(lk_ratio, h));
                    }
                }
                double inv = 0.0;
                {
                    const double self_phi = asinh(pi * pi * fabs(beta_2) * (bw * bw) / (4 * att));
#pragma unroll
                    for (int h = 0; h < ORLG_MAX_HOPS; ++h) {
                        if (h < hops) {
                            const double sum_phi = self_phi + acc[h];
                            const double r = pw / bw;
                            const double power_nli_span = (r * r * r) * (8 / (27 * pi * fabs(beta_2))) * (gamma * gamma) * readlane_d(lk_leff, h) * sum_phi * bw;
                            const double power_ase = bw * h_plank * fc * readlane_d(lk_e1, h) * nf;
                            const double gh = 1 / (pw / (power_ase + power_nli_span));
                            const int ns = __builtin_amdgcn_readlane(lk_spans, h);
                            for (int sx = 0; sx < ns; ++sx) inv += gh;
                        }
                    }
                }
                double g = 10 * log10(1 / inv);
                // the band: the step's own routine decides a window this close to its threshold
                for (u64 near = ballot(free_l && fabs(g - thr) < ORLG_GN_SLOTS_BAND_DB); near; near &= near - 1ull) {
                    const int b = ctz64(near);
                    const double gs = rmsa_gn_gsnr(wv, tb, gn, E, Q, 0, q_n, rec, 64 * c + b, n);
                    if (lane == b) g = gs;
                }
                gn_slots_set<W>(own, c, free_l ? g : nan);
                const u64 pb = ballot(free_l && g >= thr);
                if (lane == c) pass_l = pb;
            }
            // ---- neighbour check: every victim's sums once, then the chunks that hold a window that passed
            if (protect && ballot(pass_l != 0ull)) {
                const double c_sb = bw;
                for (int vi = 0; vi < n_c; ++vi) {
                    const int vj = uni((int)cidx[vi]);
                    const uint32_t dv = (uint32_t)uni((int)wv.qdesc[vj]);
                    const OrlgPathRec *vr = tb.recs + (dv & 0x3fffu);
                    const int v_hops = uni((int)vr->hops), v_se = uni((int)vr->se);
                    const int v_s = (int)((dv >> 14) & 0x3ffu), v_n = uni((int)tb.nslots[(dv >> 24) * ORLG_NSLOT_STRIDE + v_se]);
                    const double v_bw = (double)v_n * slot, v_fc = f0 + ((double)v_s + 0.5 * (double)v_n) * slot, v_pw = density * v_bw;
                    double v_leff, v_ratio, v_e1;
                    int v_spans, v_link;
                    const double sp = gn_slots_victim_sums(wv, tb, gn, wide, q_n, vj, vr, v_hops, v_fc, v_leff, v_ratio, v_e1, v_spans, v_link);
                    // the victim's hops whose link the path holds: where every window of the path adds its term
                    const int lw = v_link >> 6;
                    const u64 cm = lw == 0 ? c0 : lw == 1 ? c1 : lw == 2 ? c2 : c3;
                    const int shared = (int)ballot(lane < v_hops && ((cm >> (v_link & 63)) & 1ull));
                    const double v_thr = gn[ORLG_GN_THR0 + v_se - 1];
                    const double self_phi = asinh(pi * pi * fabs(beta_2) * (v_bw * v_bw) / (4 * att));
                    for (int c = 0; c < W; ++c) {
                        const u64 pb = readlane64(pass_l, c);
                        if (!pb) continue;
                        const double c_sf = f0 + ((double)(64 * c + lane) + 0.5 * (double)n) * slot;
                        const double df = c_sf - v_fc;   // (the candidate's window is free on every link of its path: disjoint from the victim's there)
                        const double A = asinh(pi * pi * fabs(beta_2) * l_eff_a * c_sb * (df + (c_sb / 2))) -
                                         asinh(pi * pi * fabs(beta_2) * l_eff_a * c_sb * (df - (c_sb / 2)));
                        const double Bt = c_pm * (c_sb / fabs(df)) * 5 / 3;
                        double inv = 0.0;
                        for (int h = 0; h < v_hops; ++h) {
                            const double ratio_h = readlane_d(v_ratio, h), leff_h = readlane_d(v_leff, h), e1_h = readlane_d(v_e1, h);
                            double sp_h = readlane_d(sp, h);
                            if ((shared >> h) & 1) sp_h += A - (Bt * ratio_h);
                            const double sum_phi = self_phi + sp_h;
                            const double r = v_pw / v_bw;
                            const double power_nli_span = (r * r * r) * (8 / (27 * pi * fabs(beta_2))) * (gamma * gamma) * leff_h * sum_phi * v_bw;
                            const double power_ase = v_bw * h_plank * v_fc * e1_h * nf;
                            const double gh = 1 / (v_pw / (power_ase + power_nli_span));
                            const int ns = __builtin_amdgcn_readlane(v_spans, h);
                            for (int sx = 0; sx < ns; ++sx) inv += gh;
                        }
                        const double mg = 10 * log10(1 / inv) - v_thr;
                        const double wc = gn_slots_get<W>(worst, c);
                        const bool mine = (pb >> lane) & 1ull;
                        gn_slots_set<W>(worst, c, mine && (mg < wc || wc != wc) ? mg : wc);   // the step's update rule, in rank order
                    }
                }
            }
            // ---- the rows, the mask words and the best window of the path
            double b_w = ninf;
            int b_s = S;
            for (int c = 0; c < W; ++c) {
                const int s = 64 * c + lane;
                const double g = gn_slots_get<W>(own, c), wc = gn_slots_get<W>(worst, c);
                const bool pass = (readlane64(pass_l, c) >> lane) & 1ull;
                const bool ok = pass && !(wc < 0.0);   // the step's own predicate: NaN refuses nothing
                const u64 okm = ballot(ok);
                if (mask && lane == 0) mask[row * W + c] = okm;
                if (s < S) {
                    if (gsnr) gsnr[row * S + s] = g;
                    if (margin) margin[row * S + s] = pass ? wc : nan;
                }
                const double own_m = g - thr;
                const double wm = ok ? (wc == wc && wc < own_m ? wc : own_m) : ninf;
                if (wm > b_w) { b_w = wm; b_s = s; }
            }
            if (best_slot || best_margin) {
                const double top = wave_max_f64(b_w);
                const int first = wave_min_i32(b_w == top && top > ninf ? b_s : S);
                if (lane == 0) {
                    if (best_slot) best_slot[row] = (int16_t)first;
                    if (best_margin) best_margin[row] = first < S ? top : nan;
                }
            }
            wave_sync();   // (the next path compacts into the same offsets)
        }
        wave_sync();
    }
}
