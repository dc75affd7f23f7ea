// orlg_rmsa_gn_am.h -- adaptive modulation behind the GN gate (include/orlg.h orlg_set_gn_modulation, orlg_step_modulation; DESIGN
// 2.33; not in the reference): what the AM instantiations of the wave-per-environment step kernel (orlg_kernels.hip,
// orlg_rmsa_am_kernel = rmsa_body<.., GN, .., AM>) and the modulation query (orlg_gn_modulation_kernels.hip) stand on.
//
// A level m in 1..M is the spectral efficiency a service runs at: n_m = nslots[rate][m] slots, threshold thresholds_db[m - 1].  The
// candidate (p, m) of the pending request is the reference's first fit of n_m on path p; its check is rmsa_gn_gsnr's (orlg_rmsa_gn.h)
// on that window.  Every running service interferes with its OWN stored level (orlg_qdesc.h): n_i and phi_mod are the level's.
//
// rmsa_gn_gsnr_am is rmsa_gn_gsnr with that decode and with the decode of the ring's first 64 entries taken out of the call: lanes =
// running services in rank order from the ring's head, the same expressions, the same masked wave sum per hop, the same span loop --
// on a state without levels its bits are rmsa_gn_gsnr's.  An interferer's bandwidth, centre, phi_mod and link mask do not depend on the
// candidate; the two asinh terms do and are evaluated per call.  Above 64 running services the later chunks are decoded per call.
#pragma once
#include "orlg_qdesc.h"
#include "orlg_rmsa_gn_protect.h"   // rmsa_gn_link_mask, rmsa_gn_phi_mod; through it orlg_rmsa_gn.h
#include "orlg_spectrum.h"

// one ring entry as an interferer: bandwidth, centre frequency, phi_mod of its level, the links of its path
struct OrlgAmEntry {
    double sb, sf, pm;
    u64 m0, m1, m2, m3;
};

// the ring entry at rank j0 + lane (rank 0 on the lanes past q_n, which do not use it), decoded as an adaptive handle stores it
DEV OrlgAmEntry am_ring_entry(const Wave &wv, const Tab &tb, OrlgGnTable gn, int E, int Q, int q_head, int q_n, int j0) {
    const double f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT];
    const bool valid = j0 + wv.lane < q_n;
    int pos = q_head + (valid ? j0 + wv.lane : 0);
    pos -= pos >= Q ? Q : 0;
    const uint32_t d = wv.qdesc[pos];
    const OrlgPathRec ri = tb.recs[orlg_qdesc_gid(d, true)];
    const int se = orlg_qdesc_se(orlg_qdesc_level(d, true), (int)ri.se);
    const int s_i = orlg_qdesc_slot(d), n_i = (int)tb.nslots[orlg_qdesc_rate(d) * ORLG_NSLOT_STRIDE + se];
    OrlgAmEntry e;
    // (a constant `wide` per call, as rmsa_gn_audit_decode: the unrolled loop then keeps its words in registers)
    if (E > 64) rmsa_gn_link_mask(ri, true, e.m0, e.m1, e.m2, e.m3);
    else rmsa_gn_link_mask(ri, false, e.m0, e.m1, e.m2, e.m3);
    e.sb = (double)n_i * slot;
    e.sf = f0 + ((double)s_i + 0.5 * (double)n_i) * slot;
    e.pm = rmsa_gn_phi_mod(se);
    return e;
}

// GSNR [dB] of a service on the window [s, s + n) of the path `rec` against the running services of an adaptive handle.  `first`:
// am_ring_entry(.., 0) of the ring as it stands.  Wave-cooperative, the result is wave-uniform.
DEV double rmsa_gn_gsnr_am(const Wave &wv, const Tab &tb, OrlgGnTable gn, int E, int Q, int q_head, int q_n, const OrlgPathRec *rec, int s, int n,
                           const OrlgAmEntry &first) {
    const double beta_2 = -21.3e-27, gamma = 1.3e-3, h_plank = 6.626e-34, pi = 3.141592653589793;
    const int lane = wv.lane;
    const double density = gn[ORLG_GN_DENSITY], f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT], att = gn[ORLG_GN_ATT];
    const double nf = gn[ORLG_GN_NF], l_eff_a = gn[ORLG_GN_LEFF_A];
    const int hops = rec->hops;
    const int my_link = (int)rec->link[lane < hops ? lane : 0];   // lane h = hop h
    const double lk_leff = gn[ORLG_GN_LINK0 + 4 * my_link], lk_ratio = gn[ORLG_GN_LINK0 + 4 * my_link + 1];
    const double lk_e1 = gn[ORLG_GN_LINK0 + 4 * my_link + 2];
    const int lk_spans = (int)gn[ORLG_GN_LINK0 + 4 * my_link + 3];
    const double bw = (double)n * slot, fc = f0 + ((double)s + 0.5 * (double)n) * slot, pw = density * bw;
    double sp = 0.0;   // lane h: interferer sum of hop h
    for (int j0 = 0; j0 < q_n; j0 += 64) {
        const bool valid = j0 + lane < q_n;
        OrlgAmEntry e = first;
        if (j0 > 0) e = am_ring_entry(wv, tb, gn, E, Q, q_head, q_n, j0);
        const double sb = e.sb;
        const double df = valid ? e.sf - fc : slot;   // (windows on a shared link are disjoint: df != 0 where it is used)
        const double A = asinh(pi * pi * fabs(beta_2) * l_eff_a * sb * (df + (sb / 2))) -
                         asinh(pi * pi * fabs(beta_2) * l_eff_a * sb * (df - (sb / 2)));
        const double B = e.pm * (sb / fabs(df)) * 5 / 3;
        for (int h = 0; h < hops; ++h) {
            const int l = uni((int)rec->link[h]), w = l >> 6;
            const u64 m = w == 0 ? e.m0 : w == 1 ? e.m1 : w == 2 ? e.m2 : e.m3;
            const bool lit = valid && ((m >> (l & 63)) & 1ull);
            const double tot = wave_add_f64(lit ? A - (B * readlane_d(lk_ratio, h)) : 0.0);
            if (lane == h) sp += tot;
        }
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

// what the levels of ONE path give the pending request: the walk M down to 1 of sp_ff_am / sap_ff_am / path_am_external
struct OrlgAmPath {
    int slot, se, n;        // the admitted candidate, se = 0: none was admitted
    double gsnr;
    int f_slot, f_se;       // the FIRST candidate checked, f_se = 0: the path has no window at any level
    double f_gsnr;
};

// x: the path's free bitmap (W words).  Levels M down to 1: the first fit of n_m below S - n_m, its check against thresholds_db[m - 1];
// the first admitted candidate ends the walk.  A level without a window ends it too: n_m does not fall with m, so no lower level has
// one.  Two neighbouring levels with the same n_m share the window, and with it the GSNR: it is evaluated once.  Wave-uniform.
template <int W>
DEV OrlgAmPath am_path_levels(const Wave &wv, const Tab &tb, OrlgGnTable gn, int E, int Q, int q_head, int q_n, const OrlgAmEntry &first,
                              const OrlgPathRec *rec, const u64 (&x)[W], int br, int M, int S) {
    OrlgAmPath r;
    r.slot = S; r.se = 0; r.n = 0; r.f_slot = S; r.f_se = 0;
    r.gsnr = r.f_gsnr = __longlong_as_double(0x7ff8000000000000ll);
    int n_prev = -1, s_prev = -1;
    double g_prev = r.gsnr;
    for (int m = M; m >= 1; --m) {
        const int n = uni((int)tb.nslots[br * ORLG_NSLOT_STRIDE + m]);
        int s0 = s_prev;
        double g = g_prev;
        if (n != n_prev) {
            s0 = uni(first_fit<W>(x, n, S - n, wv.lane));
            if (s0 < 0) break;
            g = rmsa_gn_gsnr_am(wv, tb, gn, E, Q, q_head, q_n, rec, s0, n, first);
            n_prev = n; s_prev = s0; g_prev = g;
        }
        if (!r.f_se) { r.f_slot = s0; r.f_se = m; r.f_gsnr = g; }
        if (uni((int)(g >= gn[ORLG_GN_THR0 + m - 1]))) {
            r.slot = s0; r.se = m; r.n = n; r.gsnr = g;
            break;
        }
    }
    return r;
}
