// orlg_link_stats.h -- the statistics the RMSA environments keep per link and for the network.
//
// numpy's pairwise float64 sum for the info dict's means (np_pairwise_block, np_pairwise_256, np_mean); network_compactness from
// the maintained integer sums; link_stats_update: the run statistics of a list of links' bitmaps, the per-link (span, gaps) cache
// and the time-weighted floats, for the wave-per-environment kernel (the four-environments-per-wave kernel has its own form,
// group_link_stats, and shares network_compactness, np_mean and link_replay); link_replay: the logged link updates of the DEFER
// instantiations worked off, one link per lane.  ORLG_LLOG_FLUSH: the log length that asks for a replay (the log's capacity,
// ORLG_LLOG_CAP, sizes a host allocation: orlg_device.h).
//
// Reference: optical_rl_gym/envs/rmsa_env.py _update_network_stats :537-560, _update_link_stats :562-641,
// _get_network_compactness :806-851; numpy/core/src/umath/loops_utils.h.src pairwise_sum.
#pragma once
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// numpy's float64 add.reduce order (pairwise_sum in numpy/core/src/umath/loops_utils.h.src: 8 running
// accumulators, fixed combination tree, blocks of <= 128) so that np.mean(...) in the info dict is reproduced
// bit for bit; n <= 255 here (one link per element).  The elements are summed in link-index order, the reference's list is in
// the graph's edge order (rmsa_env.py:311-322, topology.edges()): bit for bit when the link list is in graph order
// (FrozenTopology.links_in_graph_order; every shipped list is), within 2 E 2^-53 relative otherwise -- two orders of summing
// the same E non-negative terms (tests/test_many_links.py).  The split (n > 128) runs from 129 links on: tests/test_gpu_many_links.py.
DEV double np_pairwise_block(const double *a, int n) {
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; i++) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; i++) res += a[i];
    return res;
}
DEV double np_pairwise_256(const double *a, int n) {  // n <= 256: at most one split
    if (n <= 128) return np_pairwise_block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_block(a, n2) + np_pairwise_block(a + n2, n - n2);
}
DEV double np_mean(const double *a, int n) {  // n <= 512: at most two levels of splitting
    double s;
    if (n <= 128) {
        s = np_pairwise_block(a, n);
    } else {
        int n2 = n / 2;
        n2 -= n2 % 8;
        s = np_pairwise_256(a, n2) + np_pairwise_256(a + n2, n - n2);
    }
    return s / (double)n;
}

// _get_network_compactness (rmsa_env.py:844-851) from the maintained integer sums
DEV double network_compactness(int sum_span, int sum_slots_hops, int sum_gaps, int E) {
    if (sum_gaps > 0)
        return ORLG_FDIV((double)sum_span, (double)sum_slots_hops) * ORLG_FDIV((double)E, (double)sum_gaps);
    return 1.0;
}

#define ORLG_LLOG_FLUSH 40    // a link that reaches this many asks for a replay
// The logged link updates (DEFER instantiations), worked off: lane gl of a row of GL lanes = link gl (+ GL, ...) of the row's
// environment (GL = 16: four environments per wave, GL = 64: one); every lane runs through its link's entries in their order with the link's four statistics in registers -- the
// float64 operations of _update_link_stats (rmsa_env.py:562-641) as link_stats_update / group_link_stats do them, one update after the other.
template <int GL>
DEV void link_replay(const int lane, double *lst, int32_t *lint, const Tab &tb, int S, int E, const uint4 *llog) {
    const int gl = lane & (GL - 1);
    // the entries other lanes of this wave logged: the stores only have to be complete (same CU)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    for (int l0 = 0; l0 < E; l0 += GL) {
        const int link = l0 + gl;
        const bool on = link < E;
        const int li = on ? lint[link] : 0;
        const int n = (int)((uint32_t)li >> 26);
        if (ballot(n > 0) == 0ull) continue;
        double s_util = 0.0, s_ef = 0.0, s_c = 0.0, s_lu = 0.0;
        if (on && n > 0) { s_util = lst[link]; s_ef = lst[E + link]; s_c = lst[2 * E + link]; s_lu = lst[3 * E + link]; }
        const uint4 *row = llog + __mul24(on ? link : 0, ORLG_LLOG_CAP);
        const int nmax = wave_max_i32(n);
        uint4 e_nx = make_uint4(0u, 0u, 0u, 0u);
        if (n > 0) e_nx = row[0];
        for (int k = 0; k < nmax; ++k) {
            const uint4 ev = e_nx;
            if (k + 1 < n) e_nx = row[k + 1];   // (the next entry is requested before this one is worked on)
            if (k < n) {
                const int freec = (int)(ev.x & 0x3ffu), max_empty = (int)((ev.x >> 10) & 0x3ffu), span = (int)(ev.x >> 20), U = (int)ev.y;
                const double now = __hiloint2double((int)ev.w, (int)ev.z);
                if (now > 0) {
                    const double ynow = recip_refine(now);
                    const double cur0 = tb.div_s[S - freec];  // (S - free) / S
                    double cur1 = 0.0, cur2 = 0.0;
                    if (freec > 0) {
                        cur1 = 1.0 - ORLG_FDIV((double)max_empty, (double)freec);
                        cur2 = U > 1 ? ORLG_FDIV((double)span, (double)(S - freec)) * tb.inv_k[U] : 1.0;
                    }
                    const double time_diff = now - s_lu;
                    s_util = div_by((s_util * s_lu) + (cur0 * time_diff), now, ynow);
                    s_ef = div_by((s_ef * s_lu) + (cur1 * time_diff), now, ynow);
                    s_c = div_by((s_c * s_lu) + (cur2 * time_diff), now, ynow);
                }
                s_lu = now;
            }
        }
        if (on && n > 0) {
            lst[link] = s_util; lst[E + link] = s_ef; lst[2 * E + link] = s_c; lst[3 * E + link] = s_lu;
            lint[link] = li & 0x03ffffff;
        }
    }
    wave_sync();
}

// ---------------------------------------------------------------------------------------- link statistics
// Rebuild, for a list of links, the integer run statistics of the link's free bitmap and (LINKF) the
// time-weighted floats of _update_link_stats (rmsa_env.py:562-641).  Maintains the per-link (span, gaps)
// cache whose sums give _get_network_compactness (rmsa_env.py:806-851):
//     span = lambda_max - lambda_min, gaps = free runs inside the used span = used runs - 1
// for links with more than one used run, 0 otherwise.  links == nullptr means links 0..nlinks-1.
// GRAPH: after the last chunk also perform _update_network_stats (rmsa_env.py:537-560) -- its two
// time-weighted averages ride on lanes 62 / 63 of the same fp64 instruction stream as the links'.
template <int W, bool LINKF, bool GRAPH, bool DEFER = false>
DEV void link_stats_update(Wave &wv, const Tab &tb, int S, int E, const uint8_t *links, int nlinks, double now,
                           int &sum_span, int &sum_gaps, double &comp_cur, int sum_sh, double cur_thr, uint4 *llog = nullptr) {
    // DEFER (see group_link_stats, orlg_group_kernels.hip): the links' float64 recurrences are not done here -- what they consume is
    // logged per link and link_replay works the logs off with one link per lane; the graph statistics stay (one chain per environment)
    static_assert(W <= 8, "a link group is 8 lanes");
    bool need_replay = false;
    constexpr int HPC = 8;  // links per chunk: lane = link slot * 8 + word
    const int lane = wv.lane;
    const int hl = lane >> 3, w = lane & 7;
    double ynow = 0.0;
    if ((LINKF || GRAPH) && now > 0) ynow = recip_refine(now);
    for (int h0 = 0; h0 < nlinks; h0 += HPC) {
        const int nl = nlinks - h0 < HPC ? nlinks - h0 : HPC;
        const bool last_chunk = h0 + HPC >= nlinks;
        // ---- per (link, word) lane: the word's run statistics ...
        int link = 0, packed = 0, lo = 0x7fff, hi = 0, ml = 0;
        if (hl < nl) link = links ? (int)links[h0 + hl] : h0 + hl;
        // the link's words sit on consecutive lanes of its group: the neighbouring words arrive by DPP, not by further LDS
        // reads (every DPP read stands outside any condition: a lane switched off by a branch is not a readable source)
        u64 x = 0ull;
        if (hl < nl && w < W) x = wv.occ[__mul24(link, W) + w];
        const u64 prev = lane_prev_u64(x);
        int e = 0;  // free slots that continue a run reaching this word's end into the next words
        if (LINKF) {
            const int lead = x == ~0ull ? 64 : ctz64(~x);  // free slots at the word's start
            const int nlead_raw = lane_next_i32(lead);
            const int nlead = w < W - 1 ? nlead_raw : 0;
            e = nlead;
#pragma unroll
            for (int i = 0; i < W - 2; ++i) {
                const int ne_raw = lane_next_i32(e);
                const int ne = w < W - 1 ? ne_raw : 0;
                e = nlead == 64 ? 64 + ne : nlead;
            }
        }
        const bool first_free = x & 1ull;  // meaningful on the link's first lane
        // slot S - 1 sits in word (S - 1) >> 6 -- not always the last of the W words (S = 400 runs on the 8-word layout)
        const int lw = (S - 1) >> 6;
        const int last_free_bit = w == lw ? (int)((x >> ((S - 1) & 63)) & 1ull) : 0;
        bool last_free;
        if (lw == W - 1) last_free = W == 1 ? last_free_bit != 0 : lane_ahead_i32<(W > 1 ? W - 1 : 1)>(last_free_bit) != 0;  // wave-uniform branch
        else last_free = group8_max(last_free_bit) != 0;
        if (hl < nl && w < W) {
            u64 u = ~x & valid_mask(S, w);
            u64 carry_f = w > 0 ? (prev >> 63) : 0ull;
            u64 carry_u = w > 0 ? ((~prev) >> 63) : 0ull;
            u64 fstarts = x & ~((x << 1) | carry_f);
            u64 ustarts = u & ~((u << 1) | carry_u);
            packed = popc64(x) | (popc64(fstarts) << 10) | (popc64(ustarts) << 20);  // free slots, free runs, used runs
            lo = u ? 64 * w + ctz64(u) : 0x7fff;
            hi = u ? 64 * w + 64 - clz64(u) : 0;
            if (LINKF) {
                u64 st = fstarts;
                while (st) {
                    int b = ctz64(st);
                    st &= st - 1;
                    int len = free_run_length((~x) >> b, 64 - b + e);
                    ml = len > ml ? len : ml;
                }
            }
        }
        // ---- ... combined over the link's words inside its 8-lane group (no LDS round trip)
        packed = group8_add(packed);
        const int lmin = group8_min(lo), lmax = group8_max(hi);
        if (LINKF) ml = group8_max(ml);
        const int freec = packed & 0x3ff, F = (packed >> 10) & 0x3ff, U = packed >> 20;
        const bool link_lane = hl < nl && w == 0;  // one lane per link carries on
        int dspan = 0, dgaps = 0;
        if (link_lane) {
            int nspan = U > 1 ? lmax - lmin : 0, ngaps = U > 1 ? U - 1 : 0;
            int old = wv.lint[link];
            int cnt = 0;
            if (LINKF && DEFER) {
                cnt = (int)((uint32_t)old >> 26);
                const int max_empty = (F > 1 && !(F == 2 && first_free && last_free)) ? ml : 0;
                if (cnt < ORLG_LLOG_CAP - 1) {
                    llog[__mul24(link, ORLG_LLOG_CAP) + cnt] =
                        make_uint4((uint32_t)freec | ((uint32_t)max_empty << 10) | ((uint32_t)(lmax - lmin) << 20), (uint32_t)U,
                                   (uint32_t)__double2loint(now), (uint32_t)__double2hiint(now));
                    cnt += 1;
                }
                if (cnt >= ORLG_LLOG_FLUSH) need_replay = true;
                old &= 0x03ffffff;
            }
            wv.lint[link] = nspan | (ngaps << 16) | (cnt << 26);
            dspan = nspan - (old & 0xffff);
            dgaps = ngaps - (old >> 16);
        }
        for (int q = 0; q < nl; ++q) {
            sum_span += __builtin_amdgcn_readlane(dspan, q * 8);
            sum_gaps += __builtin_amdgcn_readlane(dgaps, q * 8);
        }
        const bool graph_now = GRAPH && last_chunk;
        if (graph_now) comp_cur = network_compactness(sum_span, sum_sh, sum_gaps, E);
        // ---- floats: links on their group's first lane, graph throughput / compactness on lanes 62 / 63
        if (((LINKF && !DEFER) || graph_now) && now > 0) {
            const bool is_link = LINKF && !DEFER && link_lane;
            const bool is_graph = graph_now && lane >= 62;
            if (is_link || is_graph) {
                double *l_util = wv.lst, *l_ef = wv.lst + E, *l_c = wv.lst + 2 * E, *l_lu = wv.lst + 3 * E;
                double last_update, last0, cur0;
                double last1 = 0.0, last2 = 0.0, cur1 = 0.0, cur2 = 0.0;
                if (is_link) {
                    last_update = l_lu[link];
                    last0 = l_util[link]; last1 = l_ef[link]; last2 = l_c[link];
                    cur0 = tb.div_s[S - freec];  // (S - free) / S
                    if (freec > 0) {
                        int max_empty = (F > 1 && !(F == 2 && first_free && last_free)) ? ml : 0;
                        cur1 = 1.0 - ORLG_FDIV((double)max_empty, (double)freec);
                        cur2 = U > 1 ? ORLG_FDIV((double)(lmax - lmin), (double)(S - freec)) * tb.inv_k[U] : 1.0;
                    }
                } else {
                    last_update = wv.wsc->g_lu;
                    last0 = lane == 62 ? wv.wsc->g_thr : wv.wsc->g_comp;
                    cur0 = lane == 62 ? cur_thr : comp_cur;
                }
                double time_diff = now - last_update;
                double n0 = div_by((last0 * last_update) + (cur0 * time_diff), now, ynow);
                if (is_link) {
                    double n1 = div_by((last1 * last_update) + (cur1 * time_diff), now, ynow);
                    double n2 = div_by((last2 * last_update) + (cur2 * time_diff), now, ynow);
                    l_util[link] = n0; l_ef[link] = n1; l_c[link] = n2;
                } else if (lane == 62) {
                    wv.wsc->g_thr = n0;
                } else {
                    wv.wsc->g_comp = n0;
                }
            }
        }
        if (LINKF && !DEFER && link_lane) wv.lst[3 * E + link] = now;
        wave_sync();
        if (graph_now && lane == 0) wv.wsc->g_lu = now;
        wave_sync();
    }
    if (DEFER && ballot(need_replay) != 0ull) {
        link_replay<64>(lane, wv.lst, wv.lint, tb, S, E, llog);
        vm_drain();   // the cold block ends drained: the step it rejoins then does not wait for its own log stores
    }
}
