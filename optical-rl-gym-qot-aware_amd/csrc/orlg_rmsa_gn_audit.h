// orlg_rmsa_gn_audit.h -- the GN-model GSNR of a RUNNING lightpath against the other running lightpaths of its environment, split
// into its ASE and NLI parts (include/orlg.h orlg_gn_audit): rmsa_gn_audit_victim is the victim evaluation of
// orlg_rmsa_gn_protect.h (rmsa_gn_victim_gsnr: the reference's examples/calculate_osnr.py:9-56 over the links of the service's own
// path, the service itself in no list) without a candidate's term.  Not in rmsa_env.py, and nothing in the reference calls
// calculate_osnr: the audit is this project's.
//
// What differs from the step's routine is where an interferer's decode lives.  The step evaluates a handful of victims per
// candidate and decodes every ring entry per victim; the audit evaluates ALL n, so the decode of an entry -- its path record, the
// 14-step link mask, bandwidth, centre and phi_mod -- is a value (OrlgGnAuditEntry) the caller may keep in registers across the
// whole victim loop where the ring fits one chunk of 64 lanes, and re-decodes per chunk only above that.
#pragma once
#include "orlg_qdesc.h"             // a descriptor of an adaptive handle carries the level its service runs at
#include "orlg_rmsa_gn_protect.h"   // rmsa_gn_link_mask, rmsa_gn_phi_mod

// one ring entry as an interferer: bandwidth, centre frequency, phi_mod of its modulation, the links of its path
struct OrlgGnAuditEntry {
    double sb, sf, pm;
    u64 m0, m1, m2, m3;
};

// the three values of one running service [dB]: GSNR, and its parts 10 log10(1 / sum over spans of P_ASE / P) and the same of P_NLI
struct OrlgGnAuditValue {
    double gsnr_db, ase_db, nli_db;
};

// entry `d` decoded as the step decodes it (orlg_rmsa_gn.h; adaptive: the handle's mode, OrlgParams::gn_adaptive != 0 -- orlg_qdesc.h)
DEV OrlgGnAuditEntry rmsa_gn_audit_decode(const Tab &tb, OrlgGnTable gn, uint32_t d, bool wide, bool adaptive) {
    const double f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT];
    const OrlgPathRec ri = tb.recs[orlg_qdesc_gid(d, adaptive)];
    const int se_i = orlg_qdesc_se(orlg_qdesc_level(d, adaptive), (int)ri.se);
    const int s_i = (int)((d >> 14) & 0x3ffu), n_i = (int)tb.nslots[(d >> 24) * ORLG_NSLOT_STRIDE + se_i];
    u64 m0, m1, m2, m3;
    // (a constant `wide` per call: with the flag left to its unrolled loop the compiler keeps two of the words in scratch)
    if (wide) rmsa_gn_link_mask(ri, true, m0, m1, m2, m3);
    else rmsa_gn_link_mask(ri, false, m0, m1, m2, m3);
    OrlgGnAuditEntry e;
    e.m0 = m0; e.m1 = m1; e.m2 = m2; e.m3 = m3;
    e.sb = (double)n_i * slot;
    e.sf = f0 + ((double)s_i + 0.5 * (double)n_i) * slot;
    e.pm = rmsa_gn_phi_mod(se_i);
    return e;
}

// The running service at rank `v` of the ring copied to wv.qdesc[0 .. q_n) in rank order.  Lanes = interferers in chunks of 64, the
// victim's own entry left out, one masked wave sum per hop of the victim kept on lane = hop, the spans of a link added span by span
// (rmsa_gn_victim_gsnr's shape and order); the ASE and NLI shares ride along in the span loop.  `resident`: q_n <= 64 and `mine` is
// the decode of entry `lane` (any value on the lanes past q_n); otherwise every chunk is decoded here.  Wave-uniform result.
DEV OrlgGnAuditValue rmsa_gn_audit_victim(const Wave &wv, const Tab &tb, OrlgGnTable gn, bool wide, int q_n, int v, bool resident,
                                          const OrlgGnAuditEntry &mine, bool adaptive) {
    const double beta_2 = -21.3e-27, gamma = 1.3e-3, h_plank = 6.626e-34, pi = 3.141592653589793;
    const int lane = wv.lane;
    const double density = gn[ORLG_GN_DENSITY], f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT], att = gn[ORLG_GN_ATT];
    const double nf = gn[ORLG_GN_NF], l_eff_a = gn[ORLG_GN_LEFF_A];
    const uint32_t dv = wv.qdesc[v];
    const OrlgPathRec *rec = tb.recs + orlg_qdesc_gid(dv, adaptive);
    const int se_v = orlg_qdesc_se(orlg_qdesc_level(dv, adaptive), (int)rec->se);
    const int s = (int)((dv >> 14) & 0x3ffu), n = (int)tb.nslots[(dv >> 24) * ORLG_NSLOT_STRIDE + se_v];
    const int hops = rec->hops;
    const int my_link = (int)rec->link[lane < hops ? lane : 0];   // lane h = hop h of the victim
    const double lk_leff = gn[ORLG_GN_LINK0 + 4 * my_link], lk_ratio = gn[ORLG_GN_LINK0 + 4 * my_link + 1];
    const double lk_e1 = gn[ORLG_GN_LINK0 + 4 * my_link + 2];
    const int lk_spans = (int)gn[ORLG_GN_LINK0 + 4 * my_link + 3];
    const double bw = (double)n * slot, fc = f0 + ((double)s + 0.5 * (double)n) * slot, pw = density * bw;
    double sp = 0.0;   // lane h: interferer sum of hop h
    for (int j0 = 0; j0 < q_n; j0 += 64) {
        const bool valid = j0 + lane < q_n && j0 + lane != v;
        OrlgGnAuditEntry e = mine;
        if (!resident) e = rmsa_gn_audit_decode(tb, gn, wv.qdesc[j0 + lane < q_n ? j0 + lane : 0], wide, adaptive);
        const double df = valid ? e.sf - fc : slot;   // (windows on a shared link are disjoint: df != 0 where it is used)
        const double A = asinh(pi * pi * fabs(beta_2) * l_eff_a * e.sb * (df + (e.sb / 2))) -
                         asinh(pi * pi * fabs(beta_2) * l_eff_a * e.sb * (df - (e.sb / 2)));
        const double B = e.pm * (e.sb / fabs(df)) * 5 / 3;
        for (int h = 0; h < hops; ++h) {
            const int l = uni((int)rec->link[h]), w = l >> 6;
            const u64 m = w == 0 ? e.m0 : w == 1 ? e.m1 : w == 2 ? e.m2 : e.m3;
            const bool lit = valid && ((m >> (l & 63)) & 1ull);
            const double tot = wave_add_f64(lit ? A - (B * readlane_d(lk_ratio, h)) : 0.0);
            if (lane == h) sp += tot;
        }
    }
    double gv = 0.0, av = 0.0, nv = 0.0;   // lane h: one span's share of 1 / GSNR on hop h, and its parts P_ASE / P and P_NLI / P
    {
        const double sum_phi = asinh(pi * pi * fabs(beta_2) * (bw * bw) / (4 * att)) + sp;
        const double r = pw / bw;
        const double power_nli_span = (r * r * r) * (8 / (27 * pi * fabs(beta_2))) * (gamma * gamma) * lk_leff * sum_phi * bw;
        const double power_ase = bw * h_plank * fc * lk_e1 * nf;
        if (lane < hops) {
            gv = 1 / (pw / (power_ase + power_nli_span));
            av = power_ase / pw;
            nv = power_nli_span / pw;
        }
    }
    double acc = 0.0, acc_a = 0.0, acc_n = 0.0;
    for (int h = 0; h < hops; ++h) {
        const double g = readlane_d(gv, h), a = readlane_d(av, h), b = readlane_d(nv, h);
        const int ns = __builtin_amdgcn_readlane(lk_spans, h);
        for (int sx = 0; sx < ns; ++sx) {
            acc += g;
            acc_a += a;
            acc_n += b;
        }
    }
    OrlgGnAuditValue r;
    r.gsnr_db = 10 * log10(1 / acc);
    r.ase_db = 10 * log10(1 / acc_a);
    r.nli_db = 10 * log10(1 / acc_n);
    return r;
}
