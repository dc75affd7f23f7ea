// orlg_rmsa_gn_admission.h -- the second half of the GN-model admission check for MANY candidates of one pending request at once,
// for the queries that describe the step beforehand (orlg_gn_admission_kernels.hip; include/orlg.h orlg_gn_admission_masks /
// orlg_gn_admission_windows).  The step (orlg_kernels.hip, rmsa_body<.., GN, .., PROTECT>) has one candidate and calls
// rmsa_gn_neighbour_margin (orlg_rmsa_gn_protect.h): per running service that shares a link with the candidate -- the "victim" --
// one walk of the ring for the victim's per-hop interferer sums, the candidate's term added behind the wave sums, then the span loop
// and the logarithm.  A query has up to k (1 + j) candidates, and a victim's sums over the OTHER running services do not depend on
// the candidate.  rmsa_gn_neighbour_margins is victim-major: the running services in rank order; for each one whose links meet the
// union of the candidates' links the sums ONCE (the ring walk of rmsa_gn_victim_gsnr, its text repeated here: that header's
// routines are the step's and stay as they are); then, candidates on lanes, every candidate that shares a link with the victim adds
// its own term, finishes the GSNR and updates its running minimum with the step's update rule.  The operations a candidate's margin
// goes through are those of the step, in the step's order, on the step's chunks of the ring: the value has the step's bits.
#pragma once
#include "orlg_rmsa_gn.h"
#include "orlg_rmsa_gn_protect.h"

// rmsa_gn_link_mask with the flag constant in either arm: left as a run-time flag of the unrolled loop, the compiler keeps mask
// words in scratch
DEV void rmsa_gn_link_mask_of(const OrlgPathRec &r, bool wide, u64 &m0, u64 &m1, u64 &m2, u64 &m3) {
    if (wide) rmsa_gn_link_mask(r, true, m0, m1, m2, m3);
    else rmsa_gn_link_mask(r, false, m0, m1, m2, m3);
}

// Lane c = candidate c of this pass (at most 64): `mine` = the lane holds a candidate that passed its own check, on the window
// [cs, cs + cn) of the path record tb.recs[gid].  Returns, per lane, min over the running services whose path shares a link with
// the lane's candidate of GSNR_i - thresholds_db[SE_i - 1] with that candidate lit; NaN where no running service shares a link, and
// on lanes that are not `mine`.  The ring is linearised from head 0 with q_n live entries (the kernels' LDS copy).  Wave-cooperative,
// to be called in wave-uniform control flow.  No early exit: the minimum is over all of them, as in the step.
DEV double rmsa_gn_neighbour_margins(const Wave &wv, const Tab &tb, OrlgGnTable gn, int E, int q_n, bool mine, int gid, int cs, int cn) {
    const double beta_2 = -21.3e-27, gamma = 1.3e-3, h_plank = 6.626e-34, pi = 3.141592653589793;
    const int lane = wv.lane;
    const double density = gn[ORLG_GN_DENSITY], f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT], att = gn[ORLG_GN_ATT];
    const double nf = gn[ORLG_GN_NF], l_eff_a = gn[ORLG_GN_LEFF_A];
    const bool wide = E > 64;
    double worst = __longlong_as_double(0x7ff8000000000000ll);
    // the lane's candidate: its link mask, and what its interferer term is made of (rmsa_gn_victim_gsnr's "the candidate, the last
    // interferer")
    const OrlgPathRec crec = tb.recs[mine ? gid : 0];
    u64 c0, c1, c2, c3;
    rmsa_gn_link_mask_of(crec, wide, c0, c1, c2, c3);
    if (!mine) c0 = c1 = c2 = c3 = 0ull;
    const double c_sb = (double)cn * slot, c_sf = f0 + ((double)cs + 0.5 * (double)cn) * slot;
    const double c_pm = rmsa_gn_phi_mod((int)crec.se);
    // the union of the candidates' links: a running service that meets none of them is nobody's victim
    u64 u0 = 0ull, u1 = 0ull, u2 = 0ull, u3 = 0ull;
    for (u64 todo = ballot(mine); todo; todo &= todo - 1ull) {
        const int c = ctz64(todo);
        u0 |= readlane64(c0, c);
        if (wide) { u1 |= readlane64(c1, c); u2 |= readlane64(c2, c); u3 |= readlane64(c3, c); }
    }
    if (!(u0 | u1 | u2 | u3)) return worst;
    for (int v0 = 0; v0 < q_n; v0 += 64) {
        const bool v_valid = v0 + lane < q_n;
        const uint32_t vd = wv.qdesc[v_valid ? v0 + lane : 0];
        u64 vm0, vm1, vm2, vm3;
        rmsa_gn_link_mask_of(tb.recs[vd & 0x3fffu], wide, vm0, vm1, vm2, vm3);
        u64 hit = ballot(v_valid && ((vm0 & u0) | (vm1 & u1) | (vm2 & u2) | (vm3 & u3)) != 0ull);
        while (hit) {
            const int b = ctz64(hit);
            hit &= hit - 1ull;
            const int vj = v0 + b;
            const uint32_t dv = (uint32_t)__builtin_amdgcn_readlane((int)vd, b);
            const OrlgPathRec *rec = tb.recs + (dv & 0x3fffu);
            const int s = (int)((dv >> 14) & 0x3ffu), n = (int)tb.nslots[(dv >> 24) * ORLG_NSLOT_STRIDE + rec->se];
            const u64 w0 = readlane64(vm0, b), w1 = readlane64(vm1, b), w2 = readlane64(vm2, b), w3 = readlane64(vm3, b);
            // ---- the victim's sums over the other running services: rmsa_gn_victim_gsnr up to its candidate, lane h = hop h
            const int hops = rec->hops;
            const int my_link = (int)rec->link[lane < hops ? lane : 0];
            const double lk_leff = gn[ORLG_GN_LINK0 + 4 * my_link], lk_ratio = gn[ORLG_GN_LINK0 + 4 * my_link + 1];
            const double lk_e1 = gn[ORLG_GN_LINK0 + 4 * my_link + 2];
            const int lk_spans = (int)gn[ORLG_GN_LINK0 + 4 * my_link + 3];
            const double bw = (double)n * slot, fc = f0 + ((double)s + 0.5 * (double)n) * slot, pw = density * bw;
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
            // ---- lane c = candidate c: its term on the hops whose link its path holds, the span loop, the logarithm
            const bool share = ((w0 & c0) | (w1 & c1) | (w2 & c2) | (w3 & c3)) != 0ull;   // (a lane that is not `mine` has no links)
            const double df = share ? c_sf - fc : slot;   // (the candidate's window is free on every link of its path: disjoint from the victim's there)
            const double A = asinh(pi * pi * fabs(beta_2) * l_eff_a * c_sb * (df + (c_sb / 2))) -
                             asinh(pi * pi * fabs(beta_2) * l_eff_a * c_sb * (df - (c_sb / 2)));
            const double B = c_pm * (c_sb / fabs(df)) * 5 / 3;
            const double self_phi = asinh(pi * pi * fabs(beta_2) * (bw * bw) / (4 * att));
            double acc = 0.0;
            for (int h = 0; h < hops; ++h) {
                const int l = uni((int)rec->link[h]), w = l >> 6;
                const u64 m = w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
                const double ratio_h = readlane_d(lk_ratio, h), leff_h = readlane_d(lk_leff, h), e1_h = readlane_d(lk_e1, h);
                double sp_h = readlane_d(sp, h);
                if ((m >> (l & 63)) & 1ull) sp_h += A - (B * ratio_h);
                const double sum_phi = self_phi + sp_h;
                const double r = pw / bw;
                const double power_nli_span = (r * r * r) * (8 / (27 * pi * fabs(beta_2))) * (gamma * gamma) * leff_h * sum_phi * bw;
                const double power_ase = bw * h_plank * fc * e1_h * nf;
                const double g = 1 / (pw / (power_ase + power_nli_span));
                const int ns = __builtin_amdgcn_readlane(lk_spans, h);
                for (int sx = 0; sx < ns; ++sx) acc += g;
            }
            const double margin = 10 * log10(1 / acc) - gn[ORLG_GN_THR0 + (int)rec->se - 1];
            if (share) worst = margin < worst || worst != worst ? margin : worst;   // the step's update rule, in rank order
        }
    }
    return worst;
}
