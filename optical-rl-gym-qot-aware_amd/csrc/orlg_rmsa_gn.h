// orlg_rmsa_gn.h -- the GN-model GSNR admission check of the wave-per-environment step kernel (orlg_kernels.hip, rmsa_body<.., GN>;
// include/orlg.h orlg_rmsa_gn_gate): rmsa_gn_gsnr, the arithmetic of the reference's examples/calculate_osnr.py:9-56
// for a candidate service on a slot window against the services the environment has running.  Not in rmsa_env.py: the gate is
// this project's.  Its table (OrlgParams::gn, ORLG_GN_* in orlg_device.h) is built by the host once per handle (orlg_set_gn_gate).
#pragma once
#include "orlg_rmsa_layout.h"

typedef const double __attribute__((address_space(1))) *OrlgGnTable;   // OrlgParams::gn: global memory, not a generic pointer

// GSNR [dB] of a service on the window [s, s + n) of the path `rec` (include/orlg.h orlg_rmsa_gn_gate).  Wave-cooperative, the
// result is wave-uniform.  Lanes = running services, in chunks of 64 over the release queue's ring [q_head, q_head + q_n): a
// lane decodes its entry into window, bandwidth, centre, spectral efficiency and the set of links of its path (a bitmask, E <= 255).
// The fibre is uniform, so the two asinh terms (A) and phi_mod (b_i / |df|) 5/3 (B) of an interferer are evaluated once and
// summed per hop of the candidate over the services whose path holds the hop's link: A - B l_eff / L, the reference's
// per-interferer term, summed in queue order by a wave reduction (the reference sums in provision order: ~1e-15 relative).  The
// spans of a link are equal; their contribution is added span by span like the reference does.
DEV double rmsa_gn_gsnr(const Wave &wv, const Tab &tb, OrlgGnTable gn, int E, int Q, int q_head, int q_n, const OrlgPathRec *rec,
                        int s, int n) {
    const double beta_2 = -21.3e-27, gamma = 1.3e-3, h_plank = 6.626e-34, pi = 3.141592653589793;
    const int lane = wv.lane;
    const double density = gn[ORLG_GN_DENSITY], f0 = gn[ORLG_GN_F0], slot = gn[ORLG_GN_SLOT], att = gn[ORLG_GN_ATT];
    const double nf = gn[ORLG_GN_NF], l_eff_a = gn[ORLG_GN_LEFF_A];
    const int hops = rec->hops;
    // the links' constants for every hop at once: lane h = hop h, read back per hop by readlane
    const int my_link = (int)rec->link[lane < hops ? lane : 0];   // (lanes past the path's end read hop 0's and do not use them)
    const double lk_leff = gn[ORLG_GN_LINK0 + 4 * my_link], lk_ratio = gn[ORLG_GN_LINK0 + 4 * my_link + 1];
    const double lk_e1 = gn[ORLG_GN_LINK0 + 4 * my_link + 2];
    const int lk_spans = (int)gn[ORLG_GN_LINK0 + 4 * my_link + 3];
    const double bw = (double)n * slot, fc = f0 + ((double)s + 0.5 * (double)n) * slot, pw = density * bw;
    const bool wide = E > 64;   // (wave-uniform: the links of most topologies fit one word of the mask)
    double sp = 0.0;   // lane h: interferer sum of hop h
    for (int j0 = 0; j0 < q_n; j0 += 64) {
        const bool valid = j0 + lane < q_n;
        int pos = q_head + (valid ? j0 + lane : 0);
        pos -= pos >= Q ? Q : 0;
        const uint32_t d = wv.qdesc[pos];
        const OrlgPathRec ri = tb.recs[d & 0x3fffu];
        const int s_i = (int)((d >> 14) & 0x3ffu), n_i = (int)tb.nslots[(d >> 24) * ORLG_NSLOT_STRIDE + ri.se];
        u64 m0 = 0ull, m1 = 0ull, m2 = 0ull, m3 = 0ull;
#pragma unroll
        for (int h = 0; h < ORLG_MAX_HOPS; ++h) {
            const int l = (int)ri.link[h];
            const u64 bit = h < (int)ri.hops ? 1ull << (l & 63) : 0ull;
            if (!wide) {
                m0 |= bit;
            } else {
                const int w = l >> 6;
                m0 |= w == 0 ? bit : 0ull; m1 |= w == 1 ? bit : 0ull; m2 |= w == 2 ? bit : 0ull; m3 |= w == 3 ? bit : 0ull;
            }
        }
        // asinh(..) - asinh(..) and phi_mod (b_i / |df|) 5/3 as calculate_osnr.py:33-45 writes them
        const double sb = (double)n_i * slot, sf = f0 + ((double)s_i + 0.5 * (double)n_i) * slot;
        const double df = valid ? sf - fc : slot;   // (windows on a shared link are disjoint: df != 0 where it is used)
        const int se = (int)ri.se;
        const double pm = se <= 2 ? 1.0 : se == 3 ? 2.0 / 3 : se == 4 ? 17.0 / 25 : se == 5 ? 69.0 / 100 : 13.0 / 21;
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
