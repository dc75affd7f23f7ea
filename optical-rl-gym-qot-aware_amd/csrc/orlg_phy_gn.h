// orlg_phy_gn.h -- the GN-model admission check of the QoT-aware step kernel (orlg_phy_kernels.hip; include/orlg.h
// orlg_gn_gate): gn_gsnr, the arithmetic of the reference's examples/calculate_osnr.py:9-56 against the live occupancy.  Not in
// phy_rmsa_env.py: the gate is this project's.  Its tables are built by orlg_gn_tables_kernel (orlg_phy_api.hip).
#pragma once
#include "orlg_phy_layout.h"
#include "orlg_sections.h"

// GN-model GSNR [dB] of channel `ch` on the path `rec` against the live occupancy (include/orlg.h orlg_gn_gate): the
// arithmetic of examples/calculate_osnr.py:9-56 for a service that is not yet in the links' lists.  Wave-cooperative, result
// wave-uniform.  Lanes = channels: the two asinh terms and the modulation term of an interferer depend on the fibre only
// through its attenuation, uniform here, so they are evaluated once per channel (A, B) and summed per link over the channels
// the link has lit (the reference's per-interferer sum, re-associated: ~1e-15 relative); the spans of a link are equal, their
// contribution is added span by span like the reference does.
template <int W>
DEV double gn_gsnr(const OrlgPhyParams &p, const u64 *occ, const OrlgPathRec *rec, int mrow_off, int ch_v, int lane SEC_PARAMS) {
    SEC(8);   // (section profile of the check: table rows | 11 hop sums | 12 span powers | 14 logarithm)
    const double beta_2 = -21.3e-27, gamma = 1.3e-3, h_plank = 6.626e-34, pi = 3.141592653589793;
    // the channel and the table row are wave-uniform, and the compiler has to know it: as values of lanes (they come out of LDS)
    // every table address was a 64-bit register pair per word -- spilled, and each reload's wait also waited for the loads before it
    const int ch = uni(ch_v);
    const uint8_t *mrow = p.mod_t + (size_t)uni(mrow_off);
    const double bw = p.gn_bw, pw = p.gn_pw, nf = p.gn_nf;
    const double fc = p.gn_cf[ch];
    // the interferer terms of the lane's channels against channel ch: rows of the tables (coalesced over the lanes)
    const double *rowA = p.gn_A + (size_t)ch * p.cpad, *rowR = p.gn_R + (size_t)ch * p.cpad;
    // (every load of the check is issued before the first value is used, none of them under a condition: a load inside
    // `if (valid)` has to be waited for inside it -- one memory round trip per word, and they were most of the check's time)
    double A[W], B[W];
    int se_w[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int c = 64 * w + lane;
        const int cc = c < p.C ? c : 0;   // a channel that exists: the value is dropped below
        se_w[w] = (int)mrow[cc]; A[w] = rowA[cc]; B[w] = rowR[cc];
    }
    const double base = p.gn_link[4 * p.E];
    const double r = pw / bw;
    double acc = 0.0;
    const int hops = rec->hops;
    // the links' constants (effective length, its ratio to the span length, exp(2 att len) - 1, spans) for every hop at once:
    // lane h = hop h, read back per hop by readlane -- one memory round trip per check instead of one per hop
    double lk0, lk1, lk2;
    int lkn;
    {
        const int lnk = (int)rec->link[lane < hops ? lane : 0];   // (lanes past the path's end read hop 0's constants and do not use them)
        lk0 = p.gn_link[4 * lnk]; lk1 = p.gn_link[4 * lnk + 1]; lk2 = p.gn_link[4 * lnk + 2];
        lkn = p.gn_nspans[lnk];
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int c = 64 * w + lane;
        const bool valid = c < p.C && c != ch;
        int se = se_w[w];
        se = se < 1 ? 1 : (se > 6 ? 6 : se);
        const double pm = se <= 2 ? 1.0 : se == 3 ? 2.0 / 3 : se == 4 ? 17.0 / 25 : se == 5 ? 69.0 / 100 : 13.0 / 21;
        A[w] = valid ? A[w] : 0.0;
        B[w] = valid ? pm * B[w] * 5 / 3 : 0.0;
    }
    // per hop only the interferer sum over the link's lit channels is wave-wide work; what follows from it -- the span's NLI
    // and ASE power and its share of 1 / GSNR: ~100 instructions with two divisions -- is done for ALL hops at once, lane h =
    // hop h, and the spans are then added hop by hop, span by span, as the reference adds them
    double sp = 0.0;   // lane h: sum_phi of hop h
    SEC(11);
    // three hops at a time: their occupancy words are requested together and their wave sums -- chains of dependent DPP steps --
    // run interleaved (the sums themselves are formed as before, hop by hop)
    constexpr int HB = 3;
    for (int h0 = 0; h0 < hops; h0 += HB) {
        double sphi[HB];
#pragma unroll
        for (int j = 0; j < HB; ++j) {
            sphi[j] = 0.0;
            const int h = h0 + j < hops ? h0 + j : hops - 1;   // (a hop past the path's end repeats the last one; its sum is not used)
            const int link = (int)rec->link[h];
            const double ratio = readlane_d(lk1, h);
            // per interferer asinh(..) - asinh(..) - phi_mod (B / |df|) 5/3 l_eff / L, as calculate_osnr.py:33-45 sums them
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const bool lit = !((occ[__mul24(link, W) + w] >> lane) & 1ull);   // (A, B are 0 on channels that do not exist)
                sphi[j] += lit ? (A[w] - (B[w] * ratio)) : 0.0;
            }
        }
#pragma unroll
        for (int j = 0; j < HB; ++j) {
            const double tot = base + wave_add_f64(sphi[j]);
            if (lane == h0 + j && h0 + j < hops) sp = tot;
        }
    }
    double gv = 0.0;
    SEC(12);
    {
        const double l_eff = lk0, e1 = lk2;
        const double power_nli_span = (r * r * r) * (8 / (27 * pi * fabs(beta_2))) * (gamma * gamma) * l_eff * sp * bw;
        const double power_ase = bw * h_plank * fc * e1 * nf;
        if (lane < hops) gv = 1 / (pw / (power_ase + power_nli_span));
    }
    for (int h = 0; h < hops; ++h) {
        const double g = readlane_d(gv, h);
        const int ns = __builtin_amdgcn_readlane(lkn, h);
#pragma unroll 4
        for (int sx = 0; sx < ns; ++sx) acc += g;
    }
    SEC(14);
    const double gsnr_db = 10 * log10(1 / acc);
    SEC(5);
    return gsnr_db;
}
