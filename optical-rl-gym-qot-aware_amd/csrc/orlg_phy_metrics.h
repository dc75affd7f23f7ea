// orlg_phy_metrics.h -- fragmentation metrics of the QoT-aware step kernel (orlg_phy_kernels.hip) and its defragmentation
// (orlg_phy_defrag.h).
//
// Reference: optical_rl_gym/envs/phy_rmsa_env.py -- calculate_r_cut (modified) :1123-1193, calculate_r_spatial :1085-1108,
// _calculate_total_cuts :1195-1203, calculate_total_r_spatial :1110-1121, the sort keys of the heuristics :1254-1737.
// The columns of the link x channel bitmap as bit vectors; the cut metric through per-node free degrees (NvRec, nv_*); a
// candidate path's channels as (level, metric) pairs (phy_row_metrics, phy_row_best) or as one integer key (ORLG_PHY_KEY,
// phy_row_keys, phy_keys_best); the per-step totals kept incrementally (MetricCache: mc_before / mc_after / mc_flush).
#pragma once
#include "orlg_phy_layout.h"

// ---- columns as bit vectors (E <= 32).  The RSS metric and the per-step totals look at one channel's column along the LINK
// axis: bit l of col = available_channels[link l][channel].  Built once per word, a column serves every candidate path:
//   rss:  sqrt(sum len^2) / (sum len + 1) over the runs of ones of col (after: col & ~path, released: col | path)
//   cuts of a column (free runs) = popc(col & ~(col << 1))
// (the cut metric of a candidate only reads the few links adjacent to its path: it keeps its adjacency lists)
template <int W>
DEV uint32_t column_bits(const u64 *occ, int E, int w, int lane) {  // lane = channel within word w
    uint32_t col = 0u;
    for (int l = 0; l < E; ++l) col |= (uint32_t)((occ[__mul24(l, W) + w] >> lane) & 1ull) << l;
    return col;
}
DEV uint32_t lane_column_bits(const u64 *occ, int E, int W, int ch) {  // any channel, per lane
    uint32_t col = 0u;
    const int w = ch >> 6, b = ch & 63;
    for (int l = 0; l < E; ++l) col |= (uint32_t)((occ[__mul24(l, W) + w] >> b) & 1ull) << l;
    return col;
}
DEV double rss_of_column(uint32_t col, const double *sqrt_tab) {
    const int sm = __builtin_popcount(col);
    int sq = 0;
    while (col) {
        col >>= __builtin_ctz(col);
        const uint32_t inv = ~col;
        const int len = inv ? __builtin_ctz(inv) : 32;
        sq += len * len;
        col = len >= 32 ? 0u : col >> len;
    }
    return ORLG_FDIV(sqrt_tab[sq], (double)(sm + 1));
}

// float64 sum of n per-channel terms in channel order (the reference accumulates them one by one: phy_rmsa_env.py:1117) out
// of an LDS array whose entries from n up to the next multiple of 8 are zero: 8 terms per LDS round trip
DEV double ordered_sum_lds(const double *terms, int n) {
    double r = 0.0;
    const double2 *sd2 = reinterpret_cast<const double2 *>(terms);
    const int n8 = (n + 7) / 8;
    // the next eight terms are requested before the current eight are added: the additions (dependent, ~8 cycles each) hide
    // the round trip
    double2 a0 = sd2[0], a1 = sd2[1], a2 = sd2[2], a3 = sd2[3];
    for (int c8 = 1; c8 < n8; ++c8) {
        const double2 b0 = sd2[4 * c8], b1 = sd2[4 * c8 + 1], b2 = sd2[4 * c8 + 2], b3 = sd2[4 * c8 + 3];
        r += a0.x; r += a0.y; r += a1.x; r += a1.y; r += a2.x; r += a2.y; r += a3.x; r += a3.y;
        a0 = b0; a1 = b1; a2 = b2; a3 = b3;
    }
    r += a0.x; r += a0.y; r += a1.x; r += a1.y; r += a2.x; r += a2.y; r += a3.x; r += a3.y;
    return r;
}
// _calculate_total_cuts (phy_rmsa_env.py:1195-1203) and calculate_total_r_spatial (:1110-1121): run-length statistics of
// every channel's column along the link axis.  Lane = channel; the link loop is wave-uniform.
template <int W>
DEV void phy_column_metrics(const u64 *occ, const double *sqrt_tab, int E, int C, int lane, double *scratch_d, bool want_cuts,
                            bool want_rss, bool use_masks, double &cuts_out, double &rss_out, int &total_runs_out) {
    int total_runs = 0;
    for (int w = 0; w < W; ++w) {
        const int ch = 64 * w + lane;
        int runs = 0, cur = 0, sumsq = 0, sum = 0;
        int prev = 0;
        if (use_masks) {
            const uint32_t col = column_bits<W>(occ, E, w, lane);
            runs = __builtin_popcount(col & ~(col << 1));
            if (want_rss) scratch_d[ch] = ch < C ? rss_of_column(col, sqrt_tab) : 0.0;
            if (ch >= C) runs = 0;
            total_runs += wave_add_i32(runs);
            continue;
        }
        for (int l = 0; l < E; ++l) {
            int b = (int)((occ[l * W + w] >> lane) & 1ull);
            runs += b & (prev ^ 1);
            if (want_rss) {
                if (b) {
                    cur += 1;
                } else {
                    sumsq += cur * cur; sum += cur; cur = 0;
                }
            }
            prev = b;
        }
        if (want_rss) {
            sumsq += cur * cur; sum += cur;
            double term = ch < C ? sqrt_tab[sumsq] / (double)(sum + 1) : 0.0;
            scratch_d[ch] = term;
        }
        if (ch >= C) runs = 0;
        // wave sum of the per-channel run counts (integers: order irrelevant)
        for (int off = 32; off > 0; off >>= 1) runs += __shfl_xor(runs, off);
        total_runs += runs;
    }
    cuts_out = (double)total_runs / (double)C;
    total_runs_out = total_runs;
    if (want_rss) {
        wave_sync();
        // the reference accumulates the per-channel terms in channel order in float64 (phy_rmsa_env.py:1117)
        rss_out = ordered_sum_lds(scratch_d, C) / (double)C;   // terms of channels >= C are zero (written above)
        wave_sync();
    }
    (void)want_cuts;
}

// ---- the cut metric through per-node free degrees (OrlgPhyParams::nv).  A path's record: c (16 node weights), wsum = sum of
// its adjacency weights, cq = c . (path links per node), its chords (links between two path nodes that are not path links).
struct NvRec { uint4 c; int wsum, cq, nchord; uint32_t cl_lo, cl_hi, cw_lo, cw_hi; };   // chord links / weights: bytes
DEV NvRec nv_unpack(const uint4 &a, const uint4 &b) {
    NvRec r;
    r.c = a;
    r.wsum = (int)(int16_t)(b.x & 0xffffu); r.cq = (int)(int16_t)(b.x >> 16);
    r.nchord = (int)(b.y & 0xffu);
    // bytes 21..25 chord links, 26..30 chord weights
    r.cl_lo = (b.y >> 8) | (b.z << 24); r.cl_hi = (b.z >> 8) & 0xffu;                 // links 0..3 | link 4
    r.cw_lo = (b.z >> 16) | (b.w << 16); r.cw_hi = (b.w >> 16) & 0xffu;               // weights 0..3 | weight 4
    return r;
}
DEV NvRec nv_load(const uint4 *nvrec, int gid) { return nv_unpack(nvrec[2 * gid], nvrec[2 * gid + 1]); }
// the record of candidate path i out of the lanes that fetched the pair's records together (lane 2 i, 2 i + 1)
DEV NvRec nv_from_lanes(const uint4 &q, int i) {
    uint4 a, b;
    a.x = (uint32_t)__builtin_amdgcn_readlane((int)q.x, 2 * i); a.y = (uint32_t)__builtin_amdgcn_readlane((int)q.y, 2 * i);
    a.z = (uint32_t)__builtin_amdgcn_readlane((int)q.z, 2 * i); a.w = (uint32_t)__builtin_amdgcn_readlane((int)q.w, 2 * i);
    b.x = (uint32_t)__builtin_amdgcn_readlane((int)q.x, 2 * i + 1); b.y = (uint32_t)__builtin_amdgcn_readlane((int)q.y, 2 * i + 1);
    b.z = (uint32_t)__builtin_amdgcn_readlane((int)q.z, 2 * i + 1); b.w = (uint32_t)__builtin_amdgcn_readlane((int)q.w, 2 * i + 1);
    return nv_unpack(a, b);
}
DEV int nv_dot(const uint4 &c, const uint4 &d) {
    uint32_t s = __builtin_amdgcn_udot4(c.x, d.x, 0u, false);
    s = __builtin_amdgcn_udot4(c.y, d.y, s, false);
    s = __builtin_amdgcn_udot4(c.z, d.z, s, false);
    return (int)__builtin_amdgcn_udot4(c.w, d.w, s, false);
}
// weighted free chords of the record on channel ch
DEV int nv_chords(const u64 *occ, const NvRec &r, int ch, int W) {
    int s = 0;
    for (int q = 0; q < r.nchord; ++q) {
        const int cl = (int)((q < 4 ? r.cl_lo >> (8 * q) : r.cl_hi) & 0xffu), cw = (int)((q < 4 ? r.cw_lo >> (8 * q) : r.cw_hi) & 0xffu);
        s += cw * (int)((occ[__mul24(cl, W) + (ch >> 6)] >> (ch & 63)) & 1ull);
    }
    return s;
}
// D of one channel as the LDS holds it (16 nibbles) -> the byte vectors the dot products take: x = nodes 0 2 4 6, y = nodes
// 8 10 12 14, z = nodes 1 3 5 7, w = nodes 9 11 13 15 (the records keep c in the same order)
DEV uint4 nv_split(u64 d) {
    const uint32_t lo = (uint32_t)d, hi = (uint32_t)(d >> 32);
    return make_uint4(lo & 0x0f0f0f0fu, hi & 0x0f0f0f0fu, (lo >> 4) & 0x0f0f0f0fu, (hi >> 4) & 0x0f0f0f0fu);
}
DEV u64 nv_nibbles(const uint4 &c) { return (u64)(c.x | (c.z << 4)) | ((u64)(c.y | (c.w << 4)) << 32); }
DEV uint4 nv_get(const u64 *dl, int ch, int C) { return nv_split(ch < C ? dl[ch] : 0ull); }
// D[ch] += c (the channel is returned on the path) or -= c (taken): nibbles never carry into their neighbours (a node has at
// least c[v] free / used links among the path's own), so one 64-bit LDS add without return does it
DEV void nv_update(u64 *dl, const uint4 &c, int ch, bool returned) {
    const u64 nb = nv_nibbles(c);
    atomicAdd(reinterpret_cast<unsigned long long *>(dl + ch), (unsigned long long)(returned ? nb : 0ull - nb));
}
// a wave reads D entries other lanes of it wrote: LDS operations of one wave complete in order
DEV void nv_fence() { wave_sync(); }
// D from the occupancy: every free link adds one to the nibbles of its two end nodes
template <int W>
DEV void nv_build(u64 *dl, const u64 *occ, const u64 *lnib, int E, int C, int lane) {
    u64 d[W];
#pragma unroll
    for (int w = 0; w < W; ++w) d[w] = 0ull;
    for (int l = 0; l < E; ++l) {
        const u64 nb = lnib[l];
        const u64 *rowp = occ + __mul24(l, W);
#pragma unroll
        for (int w = 0; w < W; ++w) d[w] += ((rowp[w] >> lane) & 1ull) ? nb : 0ull;
    }
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (64 * w + lane < C) dl[64 * w + lane] = d[w];
    wave_sync();
}

// Level and fragmentation metric of the lane's channel in every word of candidate path `idp` (level -1: not free).
//   cut (calculate_r_cut modified, phy_rmsa_env.py:1140-1193): for a channel free on the path the "cuts before minus
//   cuts after" against the links adjacent to the path's nodes reduce to  sum_j weight_j * (1 - 2 * available[link_j]);
//   rss (calculate_r_spatial, :1085-1108): sqrt(sum len^2) / (sum len + 1) over the free runs of the channel's column
//   along the link axis, after taking the channel on the path's links minus before.
template <int W>
DEV void phy_row_metrics(const u64 *occ, const PhyTab &tb, const OrlgPhyParams &p, u64 acc, int idp, int gid, const uint8_t *mrow,
                         int lane, int metric_mode /* 0 cut, 1 rss, 2 none */, bool flat_level, int (&lv)[W], double (&mt)[W],
                         const uint32_t (&cols)[W], const double *r0w /* LDS [W][64]: RSS of the lane's columns as they are */,
                         const uint4 (&dv)[W] /* D of the lane's channels (cut metric with node-degree vectors) */) {
    if (p.use_masks && metric_mode == 1) {
        // the columns and their RSS as they are were built once for all candidate paths: phy_columns
        const uint32_t pmask = (uint32_t)uni((int)tb.masks[gid].path);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const u64 x = readlane64(acc, idp * W + w);
            lv[w] = -1; mt[w] = 0.0;
            if (x != 0ull) {
                const int ch = 64 * w + lane;
                const bool fr = ((x >> lane) & 1ull) && ch < p.C;
                const double metric = rss_of_column(cols[w] & ~pmask, tb.sqrt_tab) - r0w[w * 64 + lane];
                if (fr) { lv[w] = flat_level ? 0 : (int)mrow[ch]; mt[w] = metric; }
            }
        }
        return;
    }
    if (metric_mode == 0 && p.use_nv) {
        // cut metric = wsum - 2 * (c . D[channel] - cq - free chords): four byte dot products per channel; the caller fetched D
        // of the lane's W channels once for all candidate paths
        const NvRec nr = nv_load(p.nvrec, gid);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const u64 x = readlane64(acc, idp * W + w);
            const int ch = 64 * w + lane;
            const bool fr = ((x >> lane) & 1ull) && ch < p.C;
            lv[w] = -1; mt[w] = 0.0;
            int s = nv_dot(nr.c, dv[w]) - nr.cq;
            if (nr.nchord) s -= nv_chords(occ, nr, ch, W);
            if (fr) { lv[w] = flat_level ? 0 : (int)mrow[ch]; mt[w] = (double)(nr.wsum - 2 * s); }
        }
        return;
    }
    const int a0 = tb.adj_off[gid], a1 = tb.adj_off[gid + 1];
    if (metric_mode == 0) {
        // cut metric of every word at once: the adjacency entries sit on lanes (one LDS read), every entry then costs one
        // wave-uniform read of its link's W words -- the per-word loop of dependent LDS reads was the latency of this kernel
        int cutm[W];
#pragma unroll
        for (int w = 0; w < W; ++w) cutm[w] = 0;
        for (int j0 = a0; j0 < a1; j0 += 64) {
            const int cnt = a1 - j0 < 64 ? a1 - j0 : 64;
            const int adjv = lane < cnt ? (int)tb.adj[j0 + lane] : 0;
            for (int j = 0; j < cnt; ++j) {
                const int aw = __builtin_amdgcn_readlane(adjv, j);
                const int wt = aw >> 8;
                const u64 *rowp = occ + __mul24(aw & 0xff, W);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const int b = (int)((rowp[w] >> lane) & 1ull);
                    cutm[w] += wt * (1 - 2 * b);
                }
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const u64 x = readlane64(acc, idp * W + w);
            const int ch = 64 * w + lane;
            const bool fr = ((x >> lane) & 1ull) && ch < p.C;
            lv[w] = -1; mt[w] = 0.0;
            if (fr) { lv[w] = flat_level ? 0 : (int)mrow[ch]; mt[w] = (double)cutm[w]; }
        }
        return;
    }
    // links of the path as a bit set (E <= 255: four words)
    const OrlgPathRec *rec = tb.recs + gid;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const u64 x = readlane64(acc, idp * W + w);
        lv[w] = -1; mt[w] = 0.0;
        if (x != 0ull) {
            const int ch = 64 * w + lane;
            const bool fr = ((x >> lane) & 1ull) && ch < p.C;
            const int level = (int)mrow[ch];
            double metric;
            if (metric_mode == 2) {
                metric = 0.0;
            } else if (metric_mode == 0) {
                int m = 0;
                for (int j = a0; j < a1; ++j) {
                    const unsigned aw = tb.adj[j];
                    const int link = (int)(aw & 0xffu), wt = (int)(aw >> 8);
                    const int b = (int)((occ[__mul24(link, W) + w] >> lane) & 1ull);
                    m += wt * (1 - 2 * b);
                }
                metric = (double)m;
            } else {
                int cur0 = 0, sq0 = 0, sm0 = 0, cur1 = 0, sq1 = 0, sm1 = 0;
                u64 pm[4] = {0ull, 0ull, 0ull, 0ull};  // the path's links as a bit set (wave-uniform)
                for (int h = 0; h < rec->hops; ++h) {
                    const int pl = (int)rec->link[h];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if ((pl >> 6) == q) pm[q] |= 1ull << (pl & 63);
                }
                for (int l = 0; l < p.E; ++l) {
                    const int b = (int)((occ[__mul24(l, W) + w] >> lane) & 1ull);
                    const u64 pw = (l >> 6) == 0 ? pm[0] : (l >> 6) == 1 ? pm[1] : (l >> 6) == 2 ? pm[2] : pm[3];
                    const bool on_path = (pw >> (l & 63)) & 1ull;
                    const int b1 = on_path ? 0 : b;
                    if (b) { cur0 += 1; } else { sq0 += cur0 * cur0; sm0 += cur0; cur0 = 0; }
                    if (b1) { cur1 += 1; } else { sq1 += cur1 * cur1; sm1 += cur1; cur1 = 0; }
                }
                sq0 += cur0 * cur0; sm0 += cur0; sq1 += cur1 * cur1; sm1 += cur1;
                const double r0 = ORLG_FDIV(tb.sqrt_tab[sq0], (double)(sm0 + 1));
                const double r1 = ORLG_FDIV(tb.sqrt_tab[sq1], (double)(sm1 + 1));
                metric = r1 - r0;
            }
            if (fr) { lv[w] = flat_level ? 0 : level; mt[w] = metric; }
        }
    }
}

// The same for the policies whose metric is an integer (cut: metric_mode 0) or absent (2): level, metric and channel of the
// lane's channel in one sortable key -- (level << 20) | (metric + 1024) << 9 | (511 - channel), -1 when the channel is not free
// on the path -- so that "best channel by (level desc, metric desc, channel asc)" is ONE integer maximum over the wave.
// |metric| <= sum of the adjacency weights < 1024 (checked at creation).
#define ORLG_PHY_KEY(level, metric, ch) (((level) << 20) | (((metric) + 1024) << 9) | (511 - (ch)))
// v_cndmask with a wave-uniform lane mask as the condition: lane l takes if_set when bit l of mask is set
DEV int select_by_lane_mask(u64 mask, int if_set, int if_clear) {
    int r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(mask));
    return r;
}
template <int W>
DEV void phy_row_keys(const u64 *occ, const PhyTab &tb, const OrlgPhyParams &p, u64 acc, int idp, int gid, const uint8_t *mrow,
                      int lane, int metric_mode /* 0 cut, 2 none */, bool flat_level, int (&key)[W],
                      const uint4 (&dv)[W] /* D of the lane's channels (cut metric with node-degree vectors) */,
                      const uint32_t (&lvk)[W] /* levels of the lane's channels on paths 0..3 (mod_k) */,
                      const uint32_t *mk_hi /* mod_k row of the lane's first channel, second word: paths 4.. */,
                      const uint4 &nvq /* lane 2 i, 2 i + 1: node record of candidate path i */) {
    // key = (level << 20) + (metric << 9) + kc, kc = (1024 << 9) | (511 - channel); bits of channels >= C are never set in the
    // occupancy (valid_mask), so "free on the path" (the lane's bit of the path's word) is the whole condition
    const int kc0 = (1024 << 9) + 511 - lane;
    const int lsh = 8 * (idp & 3);
    if (metric_mode == 0 && p.use_nv) {
        // cut metric = wsum - 2 * (c . D[channel] - cq - free chords): four byte dot products per channel
        const NvRec nr = nv_from_lanes(nvq, idp);
        const int kpath = kc0 + ((nr.wsum + 2 * nr.cq) << 9);
        int chs[W];   // weighted free chords of the lane's channels: per chord the link's W words in one go
#pragma unroll
        for (int w = 0; w < W; ++w) chs[w] = 0;
        for (int q = 0; q < nr.nchord; ++q) {
            const int cl = (int)((q < 4 ? nr.cl_lo >> (8 * q) : nr.cl_hi) & 0xffu), cw = (int)((q < 4 ? nr.cw_lo >> (8 * q) : nr.cw_hi) & 0xffu);
            const u64 *rowp = occ + __mul24(cl, W);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const u64 x = rowp[w];
                chs[w] += select_by_lane_mask(readlane64(x, 0), cw, 0);
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            int s = nv_dot(nr.c, dv[w]) - chs[w];
            const int lvl = flat_level ? 0 : (int)(((idp < 4 ? lvk[w] : mk_hi[128 * w]) >> lsh) & 0xffu);
            const int kk = (lvl << 20) + (kpath - 64 * w) - (s << 10);
            key[w] = select_by_lane_mask(readlane64(acc, idp * W + w), kk, -1);
        }
        return;
    }
    int m[W];
#pragma unroll
    for (int w = 0; w < W; ++w) m[w] = 0;
    if (metric_mode == 0) {
        // the adjacency entries sit on lanes (one LDS read), every entry then costs one wave-uniform read of its link's W words
        const int a0 = tb.adj_off[gid], a1 = tb.adj_off[gid + 1];
        for (int j0 = a0; j0 < a1; j0 += 64) {
            const int cnt = a1 - j0 < 64 ? a1 - j0 : 64;
            const int adjv = lane < cnt ? (int)tb.adj[j0 + lane] : 0;
            for (int j = 0; j < cnt; ++j) {
                const int aw = __builtin_amdgcn_readlane(adjv, j);
                const int wt = aw >> 8;
                const u64 *rowp = occ + __mul24(aw & 0xff, W);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const int b = (int)((rowp[w] >> lane) & 1ull);
                    m[w] += wt * (1 - 2 * b);
                }
            }
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int lvl = flat_level ? 0 : (int)(((idp < 4 ? lvk[w] : mk_hi[128 * w]) >> lsh) & 0xffu);
        const int kk = (lvl << 20) + (m[w] << 9) + (kc0 - 64 * w);
        key[w] = select_by_lane_mask(readlane64(acc, idp * W + w), kk, -1);
    }
}
template <int W>
DEV int phy_keys_best(const int (&key)[W]) {
    int h = key[0];
#pragma unroll
    for (int w = 1; w < W; ++w) h = key[w] > h ? key[w] : h;
    return wave_max_i32(h);
}

// the lane's channel columns of every word, built once per request for all candidate paths (mask mode only)
template <int W>
DEV void phy_columns(const u64 *occ, const PhyTab &tb, const OrlgPhyParams &p, int lane, int metric_mode, uint32_t (&cols)[W],
                     double *r0w /* LDS [W][64] */) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        cols[w] = 0u;
        if (p.use_masks && metric_mode == 1) {
            cols[w] = column_bits<W>(occ, p.E, w, lane);
            r0w[w * 64 + lane] = rss_of_column(cols[w], tb.sqrt_tab);   // read back by the same lane only
        }
    }
}

// Best remaining channel of a row in sorted order: max level, then max metric, then min channel (wave-wide).
template <int W>
DEV void phy_row_best(const int (&lv)[W], const double (&mt)[W], int lane, int &level, double &metric, int &channel) {
    int L = -1;
#pragma unroll
    for (int w = 0; w < W; ++w) L = lv[w] > L ? lv[w] : L;
    L = wave_max_i32(L);
    level = L; metric = 0.0; channel = -1;
    if (L < 0) return;
    double M = -__longlong_as_double((long long)ORLG_INF_BITS);  // lanes without a channel of that level stay at -inf
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (lv[w] == L && mt[w] > M) M = mt[w];
    M = wave_max_f64(M);
    metric = M;
    // lowest channel among the ties: the first word with a match, its lowest lane
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const u64 m = ballot(lv[w] == L && mt[w] == M);
        if (m) { channel = 64 * w + ctz64(m); return; }
    }
}

// ---- per-step totals kept incrementally (networks of at most 32 links).  _calculate_total_cuts (phy_rmsa_env.py:1195-1203)
// is an integer count of free runs over all channel columns; calculate_total_r_spatial (:1110-1121) a float64 sum of one term
// per channel IN CHANNEL ORDER.  Both change only in the columns a provision / release / move touches: every such site
// subtracts the column's runs before it changes the occupancy and adds them back afterwards (mc_before / mc_after, wave
// uniform: the column = one ballot over link lanes), and rewrites the column's term; the per-step output is then the integer
// total and the ordered sum of the cached terms instead of a rebuild of all 268 columns.
struct MetricCache {
    bool on, want_rss;
    // the channel-order float64 sum of the RSS terms is a chain of C dependent additions per step -- a fifth of a step with the
    // metrics written.  A launch of many steps defers it: every rewritten term is logged (value, channel, the number
    // of output points passed in the block), and once per block of up to 64 steps the sums of ALL its steps are formed at once,
    // lane = step, every lane the same chain over ITS step's terms (mc_flush): C additions per block instead of per step.
    bool defer, log_overflow;
    int nlog, stamp, t0, env;   // (the log's arrays are addressed from the kernel arguments where they are used: OrlgPhyParams::rlog_*)
    int total_runs;
    double *cterm;          // HBM [cpad]
    double __attribute__((address_space(3))) *lterm;   // the same terms in LDS (mc_after<true>)
    const double *sqrt_tab;
    int E, W;
};
DEV uint32_t mc_column(const u64 *occ, const MetricCache &mc, int ch, int lane) {
    const bool bit = lane < mc.E && ((occ[__mul24(lane, mc.W) + (ch >> 6)] >> (ch & 63)) & 1ull);
    return (uint32_t)ballot(bit);
}
DEV void mc_before(const u64 *occ, MetricCache &mc, int ch, int lane) {
    if (!mc.on) return;
    const uint32_t col = mc_column(occ, mc, ch, lane);
    mc.total_runs -= __builtin_popcount(col & ~(col << 1));
}
// LT: the terms live in the wave's LDS (lterm) instead of the HBM scratch array -- the kernels whose steps leave the per-channel
// LDS scratch alone (no RSS-metric policy, no defragmentation): no HBM round trip per step for the channel-order sum
template <bool LT = false>
DEV void mc_after(const u64 *occ, MetricCache &mc, int ch, int lane) {
    if (!mc.on) return;
    const uint32_t col = mc_column(occ, mc, ch, lane);
    mc.total_runs += __builtin_popcount(col & ~(col << 1));
    if (mc.want_rss) {
        const double t = rss_of_column(col, mc.sqrt_tab);
        if (lane == 0) {
            if (LT) mc.lterm[ch] = t; else mc.cterm[ch] = t;
        }
        if (mc.defer) {
            if (mc.nlog < ORLG_RLOG_CAP) {
                if (lane == 0) {
                    const auto kq = kernarg_as<OrlgPhyParams>();
                    const size_t at = (size_t)mc.env * ORLG_RLOG_CAP + mc.nlog;
                    kq->rlog_val[at] = t; kq->rlog_key[at] = (uint32_t)ch | ((uint32_t)mc.stamp << 16);
                }
                mc.nlog += 1;
            } else {
                mc.log_overflow = true;   // (reported: more than 160 terms rewritten in one step)
            }
        }
    }
}
// The deferred sums of a block: lane t = the block's step t.  Channel by channel in the reference's order (calculate_total_r_spatial
// adds the terms one by one, phy_rmsa_env.py:1117): the term as it was at the block's start, unless the log holds a rewrite
// the step has seen (stamp <= t; the last such).  Channels without a logged rewrite (a bit mask in LDS tells) cost one addition.
template <int W>
DEV void mc_flush(MetricCache &mc, const double *terms_now /* LDS [W*64] */, u64 *ormask /* LDS [W] */, int C, int cpad, int lane,
                  uint64_t out_rss, size_t B) {
    constexpr int SL = ORLG_RLOG_CAP / 64;
    const auto kq = kernarg_as<OrlgPhyParams>();
    const uint32_t *lkey = kq->rlog_key + (size_t)mc.env * ORLG_RLOG_CAP;
    const double *lval = kq->rlog_val + (size_t)mc.env * ORLG_RLOG_CAP;
    double *lt0 = kq->rlog_t0 + (size_t)mc.env * cpad;
    const int nb = mc.stamp, nlog = mc.nlog;
    uint32_t key[SL];
    double val[SL];
#pragma unroll
    for (int q = 0; q < SL; ++q) {
        const int i = lane + 64 * q;
        key[q] = 0xffffffffu; val[q] = 0.0;
        if (i < nlog) { key[q] = lkey[i]; val[q] = lval[i]; }
    }
    if (lane < W) ormask[lane] = 0ull;
    wave_sync();
#pragma unroll
    for (int q = 0; q < SL; ++q)
        if (lane + 64 * q < nlog) {
            const int ch = (int)(key[q] & 0xffffu);
            atomicOr(reinterpret_cast<unsigned long long *>(ormask + (ch >> 6)), 1ull << (ch & 63));
        }
    wave_sync();
    double S = 0.0;
    for (int w = 0; w < W; ++w) {
        const double t0v = lt0[64 * w + lane];   // (one round trip per word and block: a block is 64 steps)
        const u64 m = readlane64(ormask[w], 0);
        const int cmax = C - 64 * w < 64 ? C - 64 * w : 64;
        for (int c = 0; c < cmax; ++c) {
            double v = readlane_d(t0v, c);
            if ((m >> c) & 1ull) {
                const uint32_t chk = (uint32_t)(64 * w + c);
#pragma unroll
                for (int q = 0; q < SL; ++q) {
                    if (64 * q >= nlog) continue;
                    for (u64 mm = ballot((key[q] & 0xffffu) == chk); mm; mm &= mm - 1) {   // in log order: ascending lane, then slot
                        const int l = ctz64(mm);
                        const int st = (int)((uint32_t)__builtin_amdgcn_readlane((int)key[q], l) >> 16);
                        const double vv = readlane_d(val[q], l);
                        if (lane >= st) v = vv;
                    }
                }
            }
            S += v;
        }
    }
    if (lane < nb) ORLG_GPTR(double, out_rss)[(size_t)(mc.t0 + lane) * B + mc.env] = S / (double)C;
    // the next block starts from the terms as they are now (what the log held after the last output point is in them)
#pragma unroll
    for (int w = 0; w < W; ++w) lt0[64 * w + lane] = terms_now[64 * w + lane];
    mc.t0 += nb;
    mc.nlog = 0; mc.stamp = 0;
}
