// orlg_rmsa_gn_protect.h -- the second half of the GN-model admission check of the wave-per-environment step kernel
// (orlg_kernels.hip, rmsa_body<.., GN, .., PROTECT>; include/orlg.h orlg_set_gn_protect): a candidate that closes its own
// budget (orlg_rmsa_gn.h) is provisioned only if no running lightpath that shares a link with it falls below the threshold of its own
// modulation once the candidate is lit.  rmsa_gn_neighbour_margin evaluates the reference's examples/calculate_osnr.py:9-56 for every
// such lightpath -- the "victim" -- over the links of the victim's own path, with the candidate as one more interferer on the hops
// they share (calculate_osnr.py:33-45: the per-interferer term), and returns the smallest GSNR - threshold.  Not in rmsa_env.py, and
// nothing in the reference calls calculate_osnr: the check is this project's.
//
// A running lightpath may sit below its threshold without any newcomer: a release can move a neighbour's sum either way, and a
// snapshot of a handle that does not protect can be loaded.  Nothing is torn down then; every candidate that touches such a
// lightpath is refused while it lasts.
#pragma once
#include "orlg_rmsa_gn.h"

// the links of a path record as a bitmask of four words (E <= 255), as rmsa_gn_gsnr builds it per ring entry
DEV void rmsa_gn_link_mask(const OrlgPathRec &r, bool wide, u64 &m0, u64 &m1, u64 &m2, u64 &m3) {
    m0 = m1 = m2 = m3 = 0ull;
#pragma unroll
    for (int h = 0; h < ORLG_MAX_HOPS; ++h) {
        const int l = (int)r.link[h];
        const u64 bit = h < (int)r.hops ? 1ull << (l & 63) : 0ull;
        if (!wide) {
            m0 |= bit;
        } else {
            const int w = l >> 6;
            m0 |= w == 0 ? bit : 0ull; m1 |= w == 1 ? bit : 0ull; m2 |= w == 2 ? bit : 0ull; m3 |= w == 3 ? bit : 0ull;
        }
    }
}

// phi_mod of calculate_osnr.py:36-43 by spectral efficiency
DEV double rmsa_gn_phi_mod(int se) { return se <= 2 ? 1.0 : se == 3 ? 2.0 / 3 : se == 4 ? 17.0 / 25 : se == 5 ? 69.0 / 100 : 13.0 / 21; }

// GSNR [dB] of the running service at ring offset `vj` (its record `rec`, window [s, s + n)) once the candidate (record `cand`, window
// [cs, cs + cn)) is lit.  The shape of rmsa_gn_gsnr: lanes = ring entries in chunks of 64, the victim's own entry left out (it is in
// no list: the reference's stale-phi quirk never fires), one wave sum per hop of the victim; the candidate's term is added behind
// the wave sums on the hops whose link the candidate's path holds (c0..c3: its link mask).  Wave-uniform.
DEV double rmsa_gn_victim_gsnr(const Wave &wv, const Tab &tb, OrlgGnTable gn, int E, int Q, int q_head, int q_n, int vj, const OrlgPathRec *rec,
                               int s, int n, const OrlgPathRec *cand, int cs, int cn, u64 c0, u64 c1, u64 c2, u64 c3) {
    const double beta_2 = -21.3e-27, gamma = 1.3e-3, h_plank = 6.626e-34, pi = 3.141592653589793;
    const int lane = wv.lane;
    const double density = gn[ORLG_GN_DENSITY], f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT], att = gn[ORLG_GN_ATT];
    const double nf = gn[ORLG_GN_NF], l_eff_a = gn[ORLG_GN_LEFF_A];
    const int hops = rec->hops;
    const int my_link = (int)rec->link[lane < hops ? lane : 0];   // lane h = hop h of the victim
    const double lk_leff = gn[ORLG_GN_LINK0 + 4 * my_link], lk_ratio = gn[ORLG_GN_LINK0 + 4 * my_link + 1];
    const double lk_e1 = gn[ORLG_GN_LINK0 + 4 * my_link + 2];
    const int lk_spans = (int)gn[ORLG_GN_LINK0 + 4 * my_link + 3];
    const double bw = (double)n * slot, fc = f0 + ((double)s + 0.5 * (double)n) * slot, pw = density * bw;
    const bool wide = E > 64;
    double sp = 0.0;   // lane h: interferer sum of hop h
    for (int j0 = 0; j0 < q_n; j0 += 64) {
        const bool valid = j0 + lane < q_n && j0 + lane != vj;
        int pos = q_head + (j0 + lane < q_n ? j0 + lane : 0);
        pos -= pos >= Q ? Q : 0;
        const uint32_t d = wv.qdesc[pos];
        const OrlgPathRec ri = tb.recs[d & 0x3fffu];
        const int s_i = (int)((d >> 14) & 0x3ffu), n_i = (int)tb.nslots[(d >> 24) * ORLG_NSLOT_STRIDE + ri.se];
        u64 m0, m1, m2, m3;
        rmsa_gn_link_mask(ri, wide, m0, m1, m2, m3);
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
    {   // the candidate, the last interferer: on the hops of the victim whose link its path holds
        const double sb = (double)cn * slot, sf = f0 + ((double)cs + 0.5 * (double)cn) * slot;
        const double df = sf - fc;   // (the candidate's window is free on every link of its path: disjoint from the victim's there)
        const double pm = rmsa_gn_phi_mod((int)cand->se);
        const double A = asinh(pi * pi * fabs(beta_2) * l_eff_a * sb * (df + (sb / 2))) -
                         asinh(pi * pi * fabs(beta_2) * l_eff_a * sb * (df - (sb / 2)));
        const double B = pm * (sb / fabs(df)) * 5 / 3;
        const int w = my_link >> 6;
        const u64 m = w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
        if (lane < hops && ((m >> (my_link & 63)) & 1ull)) sp += A - (B * lk_ratio);
    }
    double gv = 0.0;   // lane h: one span's share of 1 / GSNR on hop h
    {
        const double sum_phi = asinh(pi * pi * fabs(beta_2) * (bw * bw) / (4 * att)) + sp;
        const double r = pw / bw;
        const double power_nli_span = (r * r * r) * (8 / (27 * pi * fabs(beta_2))) * (gamma * gamma) * lk_leff * sum_phi * bw;
        const double power_ase = bw * h_plank * fc * lk_e1 * nf;
        if (lane < hops) gv = 1 / (pw / (power_ase + power_nli_span));
    }
    double acc = 0.0;
    for (int h = 0; h < hops; ++h) {
        const double g = readlane_d(gv, h);
        const int ns = __builtin_amdgcn_readlane(lk_spans, h);
        for (int sx = 0; sx < ns; ++sx) acc += g;
    }
    return 10 * log10(1 / acc);
}

// min over the running services whose path shares a link with the candidate's (record `cand`, window [s, s + n)) of
// GSNR_i - thresholds_db[SE_i - 1] with the candidate lit; NaN where no running service shares a link.  Wave-cooperative, the result
// is wave-uniform.  The affected set needs no storage: per chunk of 64 ring entries a ballot of the entries whose link mask meets the
// candidate's, and one evaluation per set bit.  No early exit: the minimum is over all of them, so that the output is defined.
// Not inlined: the routine is long and runs on a minority of steps; as a call the step kernels around it keep the registers they had
// (DESIGN 2.27 has the compiler's report for both).
__device__ __noinline__ double rmsa_gn_neighbour_margin(const Wave &wv, const Tab &tb, OrlgGnTable gn, int E, int Q, int q_head, int q_n,
                                                        const OrlgPathRec *cand, int s, int n) {
    const int lane = wv.lane;
    const bool wide = E > 64;
    u64 c0, c1, c2, c3;
    rmsa_gn_link_mask(*cand, wide, c0, c1, c2, c3);
    double worst = __longlong_as_double(0x7ff8000000000000ll);
    for (int j0 = 0; j0 < q_n; j0 += 64) {
        const bool valid = j0 + lane < q_n;
        int pos = q_head + (valid ? j0 + lane : 0);
        pos -= pos >= Q ? Q : 0;
        const uint32_t d = wv.qdesc[pos];
        u64 m0, m1, m2, m3;
        rmsa_gn_link_mask(tb.recs[d & 0x3fffu], wide, m0, m1, m2, m3);
        u64 hit = ballot(valid && ((m0 & c0) | (m1 & c1) | (m2 & c2) | (m3 & c3)) != 0ull);
        while (hit) {
            const int b = ctz64(hit);
            hit &= hit - 1ull;
            const uint32_t dv = (uint32_t)__builtin_amdgcn_readlane((int)d, b);
            const OrlgPathRec *vr = tb.recs + (dv & 0x3fffu);
            const int vs = (int)((dv >> 14) & 0x3ffu), vn = (int)tb.nslots[(dv >> 24) * ORLG_NSLOT_STRIDE + vr->se];
            const double g = rmsa_gn_victim_gsnr(wv, tb, gn, E, Q, q_head, q_n, j0 + b, vr, vs, vn, cand, s, n, c0, c1, c2, c3);
            const double margin = g - gn[ORLG_GN_THR0 + (int)vr->se - 1];
            worst = margin < worst || worst != worst ? margin : worst;
        }
    }
    return worst;
}
