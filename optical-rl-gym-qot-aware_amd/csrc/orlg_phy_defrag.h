// orlg_phy_defrag.h -- the periodic defragmentation of the QoT-aware step kernel (orlg_phy_kernels.hip): phy_defragmentation and
// what only it uses (a service's channel_state key, the metrics of ONE channel on one lane, the smallest key of a wave).
//
// Reference: optical_rl_gym/envs/phy_rmsa_env.py -- step :355-417 (defrag_period, number_moves, metric), _move :662-697,
// _groom_defragmentation :703-733, _move_virtual :735-764.
#pragma once
#include "orlg_phy_metrics.h"
#include "orlg_phy_virtual.h"
#include "orlg_sections.h"
#include "orlg_spectrum.h"   // path_word

// channel_state list of a running service: (source, destination, k-path) key from its path record and direction flag
DEV int svc_key(const PhyTab &tb, int N, int K, int gid, int flags) {
    const int pair = tb.path_pair[gid];
    const int pa = pair / N, pb = pair - pa * N;
    const int s = (flags & 2) ? pb : pa, d = (flags & 2) ? pa : pb;
    return (s * N + d) * K + (gid - tb.pair_base[pair]);
}

// calculate_r_cut(modified=True) on ONE lane for channel `ch` of path `gid`: sum_j weight_j * (1 - 2 * available[link_j][ch])
// = cuts before minus after taking a free channel; the negative is the gain of releasing an occupied one (defrag_flag=True)
DEV int lane_cut_sum(const u64 *occ, const PhyTab &tb, int gid, int ch, int W) {
    int m = 0;
    const int w = ch >> 6, b = ch & 63;
    for (int j = tb.adj_off[gid]; j < tb.adj_off[gid + 1]; ++j) {
        const unsigned aw = tb.adj[j];
        const int bit = (int)((occ[__mul24((int)(aw & 0xffu), W) + w] >> b) & 1ull);
        m += (int)(aw >> 8) * (1 - 2 * bit);
    }
    return m;
}

// calculate_r_spatial on ONE lane (phy_rmsa_env.py:1085-1108): RSS of channel ch's column with the path's links forced
// to `force` (0: taken, 1: released = defrag_flag) minus the RSS of the column as it is
DEV double lane_rss_delta(const u64 *occ, const double *sqrt_tab, const OrlgPathRec *rec, int ch, int E, int W, int force,
                          const OrlgPathMasks *masks /* nullptr: no masks */) {
    if (masks) {
        const uint32_t col = lane_column_bits(occ, E, W, ch);
        return rss_of_column(force ? col | masks->path : col & ~masks->path, sqrt_tab) - rss_of_column(col, sqrt_tab);
    }
    u64 pm[4] = {0ull, 0ull, 0ull, 0ull};
    const int hops = rec->hops;
    for (int h = 0; h < hops; ++h) {
        const int pl = (int)rec->link[h];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((pl >> 6) == q) pm[q] |= 1ull << (pl & 63);
    }
    const int w = ch >> 6, bpos = ch & 63;
    int cur0 = 0, sq0 = 0, sm0 = 0, cur1 = 0, sq1 = 0, sm1 = 0;
    for (int l = 0; l < E; ++l) {
        const int b = (int)((occ[__mul24(l, W) + w] >> bpos) & 1ull);
        const u64 pw = (l >> 6) == 0 ? pm[0] : (l >> 6) == 1 ? pm[1] : (l >> 6) == 2 ? pm[2] : pm[3];
        const int b1 = ((pw >> (l & 63)) & 1ull) ? force : b;
        if (b) { cur0 += 1; } else { sq0 += cur0 * cur0; sm0 += cur0; cur0 = 0; }
        if (b1) { cur1 += 1; } else { sq1 += cur1 * cur1; sm1 += cur1; cur1 = 0; }
    }
    sq0 += cur0 * cur0; sm0 += cur0; sq1 += cur1 * cur1; sm1 += cur1;
    return ORLG_FDIV(sqrt_tab[sq1], (double)(sm1 + 1)) - ORLG_FDIV(sqrt_tab[sq0], (double)(sm0 + 1));
}

// smallest of the lanes' keys (sequence numbers: below 2^31); lanes without a key pass has = false; returns -1.0 when no lane has one
DEV double wave_min_key(uint32_t key, bool has) {
    const int m = wave_min_i32(has ? (int)key : 0x7fffffff);
    return m == 0x7fffffff ? -1.0 : (double)m;
}

// The periodic defragmentation of PhyRMSAEnv.step (phy_rmsa_env.py:355-417), run when services_processed is a multiple of
// defrag_period, right after _next_service.  Two passes:
//  1. _groom_defragmentation (:703-733): a service that is the ONLY user of a partially used channel moves that share
//     onto another lit channel of its (source, destination, k-path) with enough residual capacity (_move_virtual); the
//     old channel goes dark.  The reference walks running_services / service.channels while it mutates them (remove +
//     append): the element after a moved one is skipped and the moved one is met again at the end.  Eligibility can only
//     be lost during the pass (residual capacities shrink, users are only added), so the services eligible at the start
//     -- found by all lanes in parallel -- plus the ones re-appended by a move are the only ones the walk can act on;
//     they are visited in list order (ascending seq) and re-checked exactly at their turn.
//  2. physical pass (:359-417): every channel a service fills, whose release would improve the metric, is a candidate
//     (metric gain, age); in (gain, age) order each candidate looks for a free channel of the same modulation level on
//     its path and moves there (_move, :662-697) when placing costs less than releasing gains.
template <int W>
DEV void phy_defragmentation(const OrlgPhyParams &p, const PhyTab &tb, u64 *occ, PhyWaveScalars *ws, OrlgPhySvc *grec, u64 *gsum,
                             uint32_t *gseq, uint32_t *gcs,
                             uint8_t *gcs_n, OrlgPhyCand *cand, int *lch /* LDS [16] */, double *r0w /* LDS [W][64] */, int n_running,
                             int &next_seq, double current_time, int req_src, int req_dst, int lane, u64 *gnv, MetricCache &mc SEC_PARAMS) {
    const int N = p.N, K = p.K, E = p.E;
    const bool rss = p.defrag_metric != 0;
    bool overflow = false;
    // ------------------------------------------------------------------ 1. grooming pass
    // Which services can the walk act on?  A service whose partially used channel has no other user (the list entry's `used` is
    // its own share) and whose channel_state list holds another entry with enough residual capacity.  Both are properties of the
    // LIST: (a) one pass over the lists of the environment (lane = list, coalesced) flags every entry (key, channel, used) that
    // has such a target in a small Bloom bitmap in LDS; (b) one pass over the 8-byte record summaries (lane = service) tests the
    // service's partial channels against the bitmap -- no gather per service; (c) the few that pass are resolved exactly against
    // their list (lane = service again).  The walk of round 2 read every 48-byte record and, per service with a partial channel
    // (three in four), its list: 190 KB per cycle where this reads 30.
    int n_el = 0;
    {
        // (the per-channel LDS scratch holds both: W x 512 bytes)
        constexpr int BM_WORDS = W >= 3 ? 128 : 16 * W;             // 4096 bits (512 / 1024 for one / two words of channels)
        constexpr int KU = W >= 3 ? 4 : 1;                          // summaries per lane requested at a time
        uint32_t *bm = reinterpret_cast<uint32_t *>(r0w);
        uint16_t *maybe = reinterpret_cast<uint16_t *>(bm + BM_WORDS);   // record indices that passed the bitmap
        constexpr int MAYBE_CAP = (W * 64 * 8 - BM_WORDS * 4) / 2 < 512 ? (W * 64 * 8 - BM_WORDS * 4) / 2 : 512;
        static_assert(MAYBE_CAP >= 2 * 64 * KU, "room for the services of two rounds that pass the bitmap");
        for (int q = lane; q < BM_WORDS; q += 64) bm[q] = 0u;
        wave_sync();
        auto bm_hash = [](int key, int ch, int used) { return (uint32_t)(key * 37 + ch * 11 + used * 1031) & (BM_WORDS * 32 - 1); };
        // (a) the lists
        const int n_lists = N * N * K;
        for (int k0 = 0; k0 < n_lists; k0 += 64) {
            const int key = k0 + lane;
            // (length and first eight entries requested together: the entries do not wait for the length)
            const uint32_t *lst = gcs + (size_t)(key < n_lists ? key : 0) * p.cs_len;
            const int n = key < n_lists ? (int)gcs_n[key] : 0;
            const uint4 e03 = reinterpret_cast<const uint4 *>(lst)[0], e47 = reinterpret_cast<const uint4 *>(lst)[1];
            if (n >= 2) {
                const uint32_t e8[8] = {e03.x, e03.y, e03.z, e03.w, e47.x, e47.y, e47.z, e47.w};
                if (n <= 8) {
                    // greatest and second greatest residual capacity: entry a has a target iff some OTHER entry's free >= used_a
                    int f1 = -1, f2 = -1, a1 = -1;
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if (t < n) {
                            const int fr = cs_free(e8[t]);
                            if (fr > f1) { f2 = f1; f1 = fr; a1 = t; } else if (fr > f2) { f2 = fr; }
                        }
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if (t < n) {
                            const int best_other = t == a1 ? f2 : f1;
                            if (best_other >= cs_used(e8[t])) {
                                const uint32_t h = bm_hash(key, cs_ch(e8[t]), cs_used(e8[t]));
                                atomicOr(bm + (h >> 5), 1u << (h & 31));
                            }
                        }
                } else {
                    int f1 = -1, f2 = -1, a1 = -1;
                    for (int t = 0; t < n; ++t) {
                        const int fr = cs_free(lst[t]);
                        if (fr > f1) { f2 = f1; f1 = fr; a1 = t; } else if (fr > f2) { f2 = fr; }
                    }
                    for (int t = 0; t < n; ++t) {
                        const uint32_t en = lst[t];
                        if ((t == a1 ? f2 : f1) >= cs_used(en)) {
                            const uint32_t h = bm_hash(key, cs_ch(en), cs_used(en));
                            atomicOr(bm + (h >> 5), 1u << (h & 31));
                        }
                    }
                }
            }
        }
        wave_sync();
        // (c) exact check of the services that passed, lane = service: as the reference's loop body up to the move
        int n_maybe = 0;
        auto resolve = [&]() {
            for (int m0 = 0; m0 < n_maybe; m0 += 64) {
                const bool on = m0 + lane < n_maybe;
                const int idx = on ? (int)maybe[m0 + lane] : 0;
                bool elig = false;
                uint32_t seq = 0u;
                int ekey = 0;
                if (on) {
                    const OrlgPhySvc *r = grec + idx;
                    // (path and direction from the summary: the list's address does not wait for the record)
                    const u64 sw = gsum[idx];
                    const int gid = sum_gid(sw), nch = sum_nch(sw), flags = sum_flags(sw);
                    seq = gseq[idx];
                    const int key = svc_key(tb, N, K, gid, flags);
                    ekey = key;
                    const uint32_t *lst = gcs + (size_t)key * p.cs_len;
                    const int n = gcs_n[key];
                    const uint4 e03 = reinterpret_cast<const uint4 *>(lst)[0], e47 = reinterpret_cast<const uint4 *>(lst)[1];
                    const uint32_t e8[8] = {e03.x, e03.y, e03.z, e03.w, e47.x, e47.y, e47.z, e47.w};
                    for (int j = 0; j < nch && !elig; ++j) {
                        const int raw = r->ch[j];
                        if (raw & (1 << 14)) {
                            const int ch = raw & 0x1ff, mine = (raw >> 9) & 0x1f;
                            bool sole = false, target = false;
#pragma unroll
                            for (int t = 0; t < 8; ++t)
                                if (t < n) {
                                    if (cs_ch(e8[t]) == ch) sole = sole || cs_used(e8[t]) == mine;
                                    else target = target || cs_free(e8[t]) >= mine;
                                }
                            for (int t = 8; t < n; t += 4) {  // four independent loads per round trip
                                uint32_t en[4];
#pragma unroll
                                for (int q = 0; q < 4; ++q) en[q] = t + q < n ? lst[t + q] : 0u;
#pragma unroll
                                for (int q = 0; q < 4; ++q)
                                    if (t + q < n) {
                                        if (cs_ch(en[q]) == ch) sole = sole || cs_used(en[q]) == mine;
                                        else target = target || cs_free(en[q]) >= mine;
                                    }
                            }
                            elig = sole && target;
                        }
                    }
                }
                const u64 m = ballot(elig);
                if (m) {
                    const int pos = n_el + popc64(m & ((1ull << lane) - 1ull));
                    if (elig && pos < p.cand_cap) { cand[pos].seq = seq; cand[pos].idx = (uint16_t)idx; cand[pos].gid = (uint16_t)ekey; }
                    n_el += popc64(m);
                }
            }
            n_maybe = 0;
            wave_sync();
        };
        // (b) the services: KU summaries per lane requested at a time
        for (int i0 = 0; i0 < n_running; i0 += 64 * KU) {
            u64 sv[KU];
#pragma unroll
            for (int k = 0; k < KU; ++k) {
                const int i = i0 + 64 * k + lane;
                sv[k] = 0ull;
                if (i < n_running) sv[k] = gsum[i];
            }
#pragma unroll
            for (int k = 0; k < KU; ++k) {
                const int i = i0 + 64 * k + lane;
                bool hit = false;
                if (i < n_running) {
                    const u64 sw = sv[k];
                    const int nch = sum_nch(sw);
                    const int h0 = sum_ch(sw, 0), h1 = nch > 1 ? sum_ch(sw, 1) : 0;
                    if (nch > 2) {
                        hit = true;     // (channels beyond the summary: looked at exactly)
                    } else if ((h0 | h1) & (1 << 14)) {
                        const int key = svc_key(tb, N, K, sum_gid(sw), sum_flags(sw));
                        if (h0 & (1 << 14)) { const uint32_t h = bm_hash(key, h0 & 0x1ff, (h0 >> 9) & 0x1f); hit = (bm[h >> 5] >> (h & 31)) & 1u; }
                        if (!hit && (h1 & (1 << 14))) { const uint32_t h = bm_hash(key, h1 & 0x1ff, (h1 >> 9) & 0x1f); hit = (bm[h >> 5] >> (h & 31)) & 1u; }
                    }
                }
                const u64 m = ballot(hit);
                if (m) {
                    if (hit) maybe[n_maybe + popc64(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
                    n_maybe += popc64(m);
                }
            }
            wave_sync();
            if (n_maybe > MAYBE_CAP - 64 * KU) resolve();
        }
        if (n_maybe > 0) resolve();
    }
    if (n_el > p.cand_cap) { overflow = true; n_el = p.cand_cap; }
    int gmoves = 0;
    SEC(8);   // defragmentation: grooming walk
    {
        // The eligible services (seq, record index, list key) sit on lanes -- a cycle of the load-1400 workload has about a dozen,
        // moves re-append theirs -- and a visit requests the service's record and its channel_state list together: one HBM round
        // trip per visit.  More than a wavefront of them: the entries stay in the work list and every visit searches it.
        const bool ereg = n_el + p.number_moves <= 64;
        uint32_t eseq = 0u, ekx = 0u;    // lane e < n_el: entry e (seq; idx | key << 16)
        if (ereg && lane < n_el) { eseq = cand[lane].seq; ekx = (uint32_t)cand[lane].idx | ((uint32_t)cand[lane].gid << 16); }
        // A move makes the list iterator skip the service that FOLLOWED the moved one (it slides into its place): the walk needs
        // the successor in list order of every entry it moves -- the smallest seq above the entry's own among all running
        // services.  One pass over the dense seq array finds them all: the entries' seqs sorted in LDS, every service bisects
        // for the entry it follows and lowers that entry's successor (LDS atomic minimum).  (Round 2 searched all records after
        // every move: a third of the cycle's HBM traffic.)  Services that moved before an entry's turn lie below it in list
        // order; the re-appended ones take consecutive seqs from ns_first on and follow every original service.
        uint32_t esucc = 0xffffffffu;
        const int ns_first = next_seq;
        if (ereg && n_el > 0) {
            int erank = 0;
            for (int l2 = 0; l2 < n_el; ++l2) erank += ((uint32_t)__builtin_amdgcn_readlane((int)eseq, l2) < eseq) ? 1 : 0;
            uint32_t *ss = reinterpret_cast<uint32_t *>(r0w), *sx = ss + 64;   // [64] sorted seqs, [64] their successors
            if (lane < n_el) ss[erank] = eseq;
            sx[lane] = 0xffffffffu;
            wave_sync();
            const int steps = 32 - __builtin_clz((unsigned)n_el);   // bisection over 0 .. n_el
            for (int i0 = 0; i0 < n_running; i0 += 256) {
                uint32_t v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = i0 + 64 * k + lane;
                    v[k] = 0u;   // (below every entry: follows none)
                    if (i < n_running) v[k] = gseq[i];
                }
                int lo[4], hi[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { lo[k] = 0; hi[k] = n_el; }
                for (int it = 0; it < steps; ++it) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {   // entries with a seq below v[k]: the first `lo` of the sorted ones
                        const int mid = (lo[k] + hi[k]) >> 1;
                        const bool open = lo[k] < hi[k];
                        const uint32_t sm_ = ss[open ? mid : 0];
                        if (open) { if (sm_ < v[k]) lo[k] = mid + 1; else hi[k] = mid; }
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (lo[k] > 0) atomicMin(sx + (lo[k] - 1), v[k]);
            }
            wave_sync();
            if (lane < n_el) esucc = sx[erank];
            wave_sync();
        }
        long long cursor = -1;
        bool stop = p.number_moves == 0;  // the reference returns at its first check
        for (int visit = 0; visit < 2 * p.cand_cap && !stop; ++visit) {  // every visit moves the cursor up the list
            uint32_t seq0;
            int idx, key;
            if (ereg) {
                const bool has = lane < n_el && (long long)eseq > cursor;
                const double kmin = wave_min_key(eseq, has);
                if (kmin < 0.0) break;
                seq0 = (uint32_t)kmin;
                const uint32_t kx = (uint32_t)__builtin_amdgcn_readlane((int)ekx, ctz64(ballot(has && eseq == seq0)));
                idx = (int)(kx & 0xffffu); key = (int)(kx >> 16);
            } else {
                uint32_t bs = 0u;
                int bi = -1;
                for (int c = lane; c < n_el; c += 64) {
                    const uint32_t sq = cand[c].seq;
                    if ((long long)sq > cursor && (bi < 0 || sq < bs)) { bs = sq; bi = (int)((uint32_t)cand[c].idx | ((uint32_t)cand[c].gid << 16)); }
                }
                const double kmin = wave_min_key(bs, bi >= 0);
                if (kmin < 0.0) break;
                seq0 = (uint32_t)kmin;
                const uint32_t kx = (uint32_t)__builtin_amdgcn_readlane(bi, ctz64(ballot(bi >= 0 && bs == seq0)));
                idx = (int)(kx & 0xffffu); key = (int)(kx >> 16);
            }
            const OrlgPhySvc *r = grec + idx;
            // record and list, requested together
            const uint32_t d3 = reinterpret_cast<const uint32_t *>(r)[3];   // gid | nch << 16 | flags << 24
            const int chl = lane < ORLG_PHY_MAX_CH ? (int)r->ch[lane] : 0xffff;
            CsList l = cs_load(gcs, gcs_n, key, lane, p.cs_len);
            const int gid = uni((int)(d3 & 0xffffu)), nch = uni((int)((d3 >> 16) & 0xffu)), flags = uni((int)(d3 >> 24));
            if (lane < ORLG_PHY_MAX_CH) lch[lane] = lane < nch ? chl : 0xffff;
            wave_sync();
            const OrlgPathRec *rec = tb.recs + gid;
            bool moved = false;
            for (int j = 0; j < nch; ++j) {  // the list keeps its length: every move is remove + append
                const int raw = lch[j];
                if (raw & (1 << 14)) {
                    const int ch = raw & 0x1ff, mine = (raw >> 9) & 0x1f;
                    const int q = cs_find(l, ch, lane);
                    if (q >= 0 && cs_used(cs_get(l, q)) == mine) {
                        const u64 tm = ballot(lane < l.n && cs_ch(l.e) != ch && cs_free(l.e) >= mine);
                        if (tm) {
                            const uint32_t tg = cs_get(l, ctz64(tm));
                            cs_remove(l, ctz64(tm), lane);
                            cs_remove(l, cs_find(l, ch, lane), lane);
                            cs_append(l, cs_pack(cs_ch(tg), cs_used(tg) + mine, cs_free(tg) - mine, cs_cap(tg)), lane);
                            cs_store(gcs, gcs_n, key, l, lane);   // (the list stays on lanes for the service's other channels)
                            // _move_virtual (:735-764): the old channel goes dark on the path, the list entry moves to the end
                            mc_before(occ, mc, ch, lane);
                            if (lane < rec->hops) occ[(int)rec->link[lane] * W + (ch >> 6)] |= 1ull << (ch & 63);
                            if (gnv && lane == 0) nv_update(gnv, p.nvrec[2 * gid], ch, true);
                            wave_sync();
                            mc_after(occ, mc, ch, lane);
                            const int nxt = (lane >= j && lane + 1 < nch) ? lch[lane + 1] : 0;
                            wave_sync();
                            if (lane >= j && lane + 1 < nch) lch[lane] = nxt;
                            if (lane == nch - 1) lch[lane] = cs_ch(tg) | (mine << 9) | (1 << 14);
                            wave_sync();
                            moved = true;
                            gmoves += 1;
                        }
                    }
                }
                if (gmoves == p.number_moves) { stop = true; break; }
            }
            if (moved) {
                const int ns = next_seq;
                next_seq += 1;
                if (lane < nch) grec[idx].ch[lane] = (uint16_t)lch[lane];
                if (lane == 0) {
                    grec[idx].seq = (uint32_t)ns;
                    gsum[idx] = svc_summary(gid, flags, nch, (uint32_t)lch[0], nch > 1 ? (uint32_t)lch[1] : 0u);
                    gseq[idx] = (uint32_t)ns;
                }
                // the list iterator skips the service that followed this one (it slid into its place): the smallest seq above
                // seq0, from the dense seq array -- eight coalesced requests per lane in flight (the strided reads of the 48-byte
                // records were a third of the defragmentation's HBM traffic)
                uint32_t sm = 0u;
                bool hs = false;
                if (ereg) {
                    // the entry's successor from the table; none: it was the list's last service (then the first re-appended one
                    // follows, or it follows itself), or a re-appended one (consecutive seqs)
                    uint32_t sc = 0xffffffffu;
                    if (seq0 < (uint32_t)ns_first) sc = (uint32_t)__builtin_amdgcn_readlane((int)esucc, ctz64(ballot(lane < n_el && eseq == seq0)));
                    if (sc == 0xffffffffu) sc = seq0 < (uint32_t)ns_first ? (uint32_t)ns_first : seq0 + 1u;   // (<= ns: ns is this service's own new seq)
                    sm = sc; hs = true;
                } else if (!stop) {   // (the walk is over with the last move: nobody asks for the cursor)
                    for (int i0 = 0; i0 < n_running; i0 += 512) {
                        uint32_t v[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const int i = i0 + 64 * k + lane;
                            v[k] = 0u;
                            if (i < n_running && i != idx) v[k] = gseq[i];
                        }
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const int i = i0 + 64 * k + lane;
                            const uint32_t sq = i == idx ? (uint32_t)ns : v[k];   // (this service's own new key: not read back)
                            if (i < n_running && sq > seq0 && (!hs || sq < sm)) { sm = sq; hs = true; }
                        }
                    }
                }
                {
                    const double nk = wave_min_key(sm, hs);   // this service itself carries a later key: never "none"
                    cursor = nk < 0.0 ? (long long)seq0 : (long long)nk;
                }
                if (ereg) {
                    if (lane == n_el) { eseq = (uint32_t)ns; ekx = (uint32_t)idx | ((uint32_t)key << 16); }
                    n_el += 1;
                } else if (n_el < p.cand_cap) {
                    if (lane == 0) { cand[n_el].seq = (uint32_t)ns; cand[n_el].idx = (uint16_t)idx; cand[n_el].gid = (uint16_t)key; }
                    n_el += 1;
                } else {
                    overflow = true;
                }
            } else {
                cursor = (long long)seq0;
            }
            wave_sync();
        }
    }
    int cmoves = 0, cycles = 0;
    // ------------------------------------------------------------------ 2. physical pass
    SEC(12);  // defragmentation: candidate scan
    if (gmoves <= p.number_moves) {
        int nc = 0;
        const int base_cur = tb.pair_base[req_src * N + req_dst];
        if (gnv) nv_fence();   // the grooming pass may have returned channels
        // lane = service, from the record summaries (8 bytes: path, channel count, the first two channels) and the dense seq array;
        // the record itself is read for the arrival time of a candidate and for the channels beyond the second -- one service in
        // ten has them: those are set aside (LDS list) and scored afterwards, a wavefront of them at a time, instead of making
        // every round of 64 services loop to the longest channel list among them.  The next 64 summaries are requested before the
        // current ones are scored.
        auto score = [&](int gid_, int ch_, const NvRec &nr_) -> double {
            if (rss) return lane_rss_delta(occ, tb.sqrt_tab, tb.recs + gid_, ch_, E, W, 1, p.use_masks ? tb.masks + gid_ : nullptr);
            if (gnv) {
                // the service holds the channel on its whole path: c . D[ch] counts the free links towards off-path nodes and the
                // free chords; gain of releasing = 2 * (that - chords) - wsum
                int sdot = nv_dot(nr_.c, nv_get(gnv, ch_, p.C));
                if (nr_.nchord) sdot -= nv_chords(occ, nr_, ch_, W);
                return (double)(2 * sdot - nr_.wsum);
            }
            return (double)(-lane_cut_sum(occ, tb, gid_, ch_, W));
        };
        auto emit = [&](bool is_c, double diff, int idx, int jpos, int ch, int gid_, uint32_t seq_) {
            const u64 m = ballot(is_c);
            if (m) {
                const int pos = nc + popc64(m & ((1ull << lane) - 1ull));
                if (is_c && pos < p.cand_cap) {
                    // (age, modulation level and table row are filled in when the candidates are ranked: cand_fill)
                    OrlgPhyCand c;
                    c.diff = diff; c.age = 0.0; c.seq = seq_; c.idx = (uint16_t)idx; c.chj = (uint16_t)(ch | (jpos << 9));
                    c.gid = (uint16_t)gid_; c.pad0 = 0; c.pad1 = 0u;
                    cand[pos] = c;
                }
                nc += popc64(m);
            }
        };
        uint16_t *more = reinterpret_cast<uint16_t *>(r0w);   // services with more than two channels
        constexpr int MORE_CAP = W * 64 * 8 / 2;
        int n_more = 0;
        auto score_more = [&]() {   // channels 2 .. of the services set aside: lane = service
            for (int m0 = 0; m0 < n_more; m0 += 64) {
                const bool act = m0 + lane < n_more;
                const int idx = act ? (int)more[m0 + lane] : 0;
                u64 sw = 0ull;
                uint32_t my_seq = 0u, x5 = 0u, x6 = 0u, x7 = 0u;   // ch[2..7] of the record
                if (act) {
                    const uint32_t *rr = reinterpret_cast<const uint32_t *>(grec + idx);
                    sw = gsum[idx]; my_seq = gseq[idx]; x5 = rr[5]; x6 = rr[6]; x7 = rr[7];
                }
                const int my_n = act ? sum_nch(sw) : 0, my_gid = sum_gid(sw);
                NvRec nr = nv_unpack(make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u));
                if (!rss && gnv && act) nr = nv_load(p.nvrec, my_gid);
                const int maxn = wave_max_i32(my_n);
                for (int jj = 2; jj < maxn; ++jj) {
                    bool is_c = false;
                    double diff = 0.0;
                    int ch = 0;
                    if (jj < my_n) {
                        const int raw = jj < 8 ? (int)(((jj < 4 ? x5 : jj < 6 ? x6 : x7) >> (16 * (jj & 1))) & 0xffffu) : (int)grec[idx].ch[jj];
                        if (!(raw & (1 << 14))) {  // only channels the service fills are reallocated
                            ch = raw & 0x1ff;
                            diff = score(my_gid, ch, nr);
                            is_c = diff > 0.0;
                        }
                    }
                    emit(is_c, diff, idx, jj, ch, my_gid, my_seq);
                }
            }
            n_more = 0;
            wave_sync();
        };
        u64 sw_n = 0ull;
        uint32_t seq_n = 0u;
        if (lane < n_running) { sw_n = gsum[lane]; seq_n = gseq[lane]; }
        for (int i0 = 0; i0 < n_running; i0 += 64) {
            const int idx = i0 + lane;
            const bool act = idx < n_running;
            const u64 sw = sw_n;
            const uint32_t my_seq = seq_n;
            if (idx + 64 < n_running) { sw_n = gsum[idx + 64]; seq_n = gseq[idx + 64]; }
            const int my_n = act ? sum_nch(sw) : 0, my_gid = sum_gid(sw);
            NvRec nr = nv_unpack(make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u));
            if (!rss && gnv && act) nr = nv_load(p.nvrec, my_gid);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                bool is_c = false;
                double diff = 0.0;
                int ch = 0;
                if (jj < my_n) {
                    const int raw = sum_ch(sw, jj);
                    if (!(raw & (1 << 14))) {  // only channels the service fills are reallocated
                        ch = raw & 0x1ff;
                        diff = score(my_gid, ch, nr);
                        is_c = diff > 0.0;
                    }
                }
                emit(is_c, diff, idx, jj, ch, my_gid, my_seq);
            }
            const u64 mm = ballot(my_n > 2);
            if (mm) {
                if (my_n > 2) more[n_more + popc64(mm & ((1ull << lane) - 1ull))] = (uint16_t)idx;
                n_more += popc64(mm);
                wave_sync();
                if (n_more > MORE_CAP - 64) score_more();
            }
        }
        if (n_more > 0) score_more();
        if (nc > p.cand_cap) { overflow = true; nc = p.cand_cap; }
        wave_sync();
        SEC(14);  // defragmentation: candidate rounds
        // The rounds are sequential (a move changes what the next candidate sees), but the ORDER of the candidates is fixed once
        // they are scanned -- sorted(key=(-diff, -age)), stable -- and a candidate's table data (its path's node weights, the
        // modulation level of every channel on that path) do not depend on the moves either.  So: every candidate's rank in the
        // sorted order is counted once (all pairs, the keys are distinct; lane l holds candidates l, l + 64, ...: up to 256, the
        // load-1400 workload has 90-190 per cycle), each lane writes its candidates to their sorted position behind the work list,
        // and round q reads record q -- requested one round ahead, one dword per lane.  The service record is only read when a move
        // actually happens.  More candidates than that: the keys stay where they are and every round searches them.
        constexpr int RC = 4;                      // candidates per lane while the ranks are counted
        const bool sorted = nc <= 64 * RC && 2 * nc <= p.cand_cap;
        OrlgPhyCand *scand = cand + (p.cand_cap >> 1);
        // the rest of a candidate's record, one candidate per lane: its age (the service's arrival time: one gather) and what its
        // round will ask the QoT table -- the reference looks the candidate's path up among the k paths of the PENDING request
        // (:388-394): right when both serve the same node pair, otherwise its loop runs out and leaves k - 1 -- the level of its
        // channel on that column (:395) and the column itself
        auto cand_fill = [&](uint4 &a, uint4 &b) {
            const int idx_ = (int)(b.y & 0xffffu), ch_ = (int)((b.y >> 16) & 0x1ffu), gid_ = (int)(b.z & 0xffffu);
            const double age = current_time - grec[idx_].arrival;
            const int ridp = tb.pair_row[tb.path_pair[gid_]] * K + ((gid_ >= base_cur && gid_ < base_cur + K) ? gid_ - base_cur : K - 1);
            const uint32_t level = (uint32_t)p.mod_t[(size_t)ridp * p.cpad + ch_];
            a.z = (uint32_t)__double2loint(age); a.w = (uint32_t)__double2hiint(age);
            b.z = (uint32_t)gid_ | (level << 16); b.w = (uint32_t)ridp;
        };
        if (!sorted) {
            for (int c = lane; c < nc; c += 64) {
                uint4 a = reinterpret_cast<const uint4 *>(cand + c)[0], b = reinterpret_cast<const uint4 *>(cand + c)[1];
                cand_fill(a, b);
                reinterpret_cast<uint4 *>(cand + c)[0] = a; reinterpret_cast<uint4 *>(cand + c)[1] = b;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            wave_sync();
        }
        SEC(15);  // defragmentation: candidate ranks
        if (sorted) {
            uint4 v0[RC], v1[RC];                  // the lane's candidates: diff, age | seq, idx | chj << 16, gid, -
            int rank[RC];
#pragma unroll
            for (int s = 0; s < RC; ++s) {
                const int c = lane + 64 * s;
                v0[s] = make_uint4(0u, 0u, 0u, 0u); v1[s] = v0[s];
                rank[s] = 0;
                if (c < nc) { v0[s] = reinterpret_cast<const uint4 *>(cand + c)[0]; v1[s] = reinterpret_cast<const uint4 *>(cand + c)[1]; }
            }
#pragma unroll
            for (int s = 0; s < RC; ++s)
                if (lane + 64 * s < nc) cand_fill(v0[s], v1[s]);
            // All pairs, but on ONE 64-bit key per candidate that decides nearly every pair: the integer gain and the age rounded
            // to float32 (cut metric), the gain's bits (RSS metric).  A greater key precedes, a smaller one does not (rounding
            // is monotone); only equal keys -- the channels of one service, ages closer than 2^-24 -- take the exact three-part
            // comparison.  3 instead of 7 vector instructions per pair.
            u64 kf[RC];
#pragma unroll
            for (int s = 0; s < RC; ++s) {
                const double rd = __hiloint2double((int)v0[s].y, (int)v0[s].x), ra = __hiloint2double((int)v0[s].w, (int)v0[s].z);
                kf[s] = rss ? (u64)__double_as_longlong(rd) : (((u64)(uint32_t)(int)rd << 32) | (u64)__float_as_uint((float)ra));
                if (lane + 64 * s >= nc) kf[s] = 0ull;
            }
#pragma unroll
            for (int t = 0; t < RC; ++t) {
                const int cnt = nc - 64 * t < 64 ? nc - 64 * t : 64;
                for (int l = 0; l < cnt; ++l) {   // candidate (l, t) against every lane's own
                    const u64 jk = readlane64(kf[t], l);
                    int ties = 0;
#pragma unroll
                    for (int s = 0; s < RC; ++s) {
                        if (64 * s >= nc) continue;   // (wave-uniform: no candidate in this slot of any lane)
                        rank[s] += jk > kf[s] ? 1 : 0;
                        ties += popc64(ballot(jk == kf[s]));
                    }
                    if (ties > 1) {   // (itself is one)
                        const double jd = __hiloint2double(__builtin_amdgcn_readlane((int)v0[t].y, l), __builtin_amdgcn_readlane((int)v0[t].x, l));
                        const double ja = __hiloint2double(__builtin_amdgcn_readlane((int)v0[t].w, l), __builtin_amdgcn_readlane((int)v0[t].z, l));
                        const uint32_t jx = (uint32_t)__builtin_amdgcn_readlane((int)v1[t].x, l), jc = (uint32_t)__builtin_amdgcn_readlane((int)v1[t].y, l);
                        const u64 jo = ((u64)jx << 4) | (u64)(jc >> 25);   // order among equal (diff, age): running_services, then channel position
#pragma unroll
                        for (int s = 0; s < RC; ++s) {
                            const double rd = __hiloint2double((int)v0[s].y, (int)v0[s].x), ra = __hiloint2double((int)v0[s].w, (int)v0[s].z);
                            const u64 ro = ((u64)v1[s].x << 4) | (u64)(v1[s].y >> 25);
                            if (jk == kf[s]) rank[s] += (jd > rd || (jd == rd && (ja > ra || (ja == ra && jo < ro)))) ? 1 : 0;
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < RC; ++s) {
                const int c = lane + 64 * s;
                if (c < nc) { reinterpret_cast<uint4 *>(scand + rank[s])[0] = v0[s]; reinterpret_cast<uint4 *>(scand + rank[s])[1] = v1[s]; }
            }
            // other lanes of this wave read the sorted records back: the stores only have to be complete (same CU)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            wave_sync();
        }
        // The rounds, eight candidates at a time.  A group's records sit on the lanes (lane 8 c + d: dword d of candidate c, one
        // coalesced load, requested two groups ahead), and so does what the tables say about their paths (lane 8 c + w: the mask
        // of the channels of candidate c's modulation level in word w; lane 8 c + d: dword d of its path's node weights --
        // requested a group ahead): a round waits for no memory.  The free words of all eight paths come from ONE pass over
        // (candidate, word) lanes, as the policy reads its k candidate paths; then the candidates take their turns: free words
        // AND level mask off the lanes, D from LDS, the vote "does any channel beat -diff", the reduction to the best channel
        // only when it passes.  A move (one round in fifteen) changes what the later candidates of the group would see: the
        // next group starts right behind it.
        SEC(14);  // defragmentation: candidate rounds
        constexpr int GR = 8;
        uint32_t rec_a = 0u, rec_b = 0u, tn_a = 0u;
        u64 tm_a = 0ull;
        const int gc = lane >> 3, gd = lane & 7;   // candidate of the group, dword / word
        auto load_recs = [&](int q0) -> uint32_t {  // records q0 .. q0 + 7 of the sorted list
            uint32_t v = 0u;
            if (q0 + gc < nc) v = reinterpret_cast<const uint32_t *>(scand + q0)[lane];
            return v;
        };
        auto issue_tables = [&](uint32_t rv, int gsz, u64 &tm, uint32_t &tn) {
            const uint32_t x6 = (uint32_t)__shfl((int)rv, (lane & ~7) + 6), ridp = (uint32_t)__shfl((int)rv, (lane & ~7) + 7);
            tm = 0ull; tn = 0u;
            if (gc < gsz) {
                if (gd < W) tm = p.lvl_mask[((size_t)ridp * 32 + ((x6 >> 16) & 31u)) * W + gd];
                if (gnv && !rss) tn = reinterpret_cast<const uint32_t *>(p.nvrec + 2 * (x6 & 0xffffu))[gd];
            }
        };
        int q0 = 0;
        bool fresh = true;   // the group's inputs have to be fetched now (the first group, the group behind a move)
        while (q0 < nc) {
            uint32_t rv, tnq = 0u;
            u64 tmq = 0ull;
            int gsz;
            if (sorted) {
                gsz = nc - q0 < GR ? nc - q0 : GR;
                if (fresh) {
                    rec_a = load_recs(q0);
                    rec_b = load_recs(q0 + GR);
                    issue_tables(rec_a, gsz, tm_a, tn_a);
                    fresh = false;
                }
                rv = rec_a; tmq = tm_a; tnq = tn_a;
                rec_a = rec_b;
                rec_b = load_recs(q0 + 2 * GR);
                if (q0 + GR < nc) issue_tables(rec_a, nc - q0 - GR < GR ? nc - q0 - GR : GR, tm_a, tn_a);
            } else {
                // next candidate of sorted(key=(-diff, -age)) (stable: running_services order, then channel order): a group of one
                double bd = -1.0, ba = 0.0;
                u64 bo = ~0ull;
                int bc = -1;
                for (int c = lane; c < nc; c += 64) {
                    const double d = cand[c].diff, a = cand[c].age;
                    const u64 o = ((u64)cand[c].seq << 4) | (u64)(cand[c].chj >> 9);
                    if (d > 0.0 && (d > bd || (d == bd && (a > ba || (a == ba && o < bo))))) { bd = d; ba = a; bo = o; bc = c; }
                }
                // lexicographic maximum over the lanes' bests: greatest diff, then greatest age, then lowest order key (36 bits:
                // exact as a double); the lane that holds it hands out the candidate
                const double ninf = -__longlong_as_double((long long)ORLG_INF_BITS);
                const double D = wave_max_f64(bc >= 0 ? bd : ninf);
                if (!(D > 0.0)) break;
                const double A = wave_max_f64((bc >= 0 && bd == D) ? ba : ninf);
                const double O = -wave_max_f64((bc >= 0 && bd == D && ba == A) ? -(double)bo : ninf);
                const int wl = ctz64(ballot(bc >= 0 && bd == D && ba == A && (double)bo == O));
                const int cb = __builtin_amdgcn_readlane(bc, wl);
                rv = lane < 8 ? reinterpret_cast<const uint32_t *>(cand + cb)[lane] : 0u;
                wave_sync();
                if (lane == 0) cand[cb].diff = -1.0;
                gsz = 1;
                issue_tables(rv, 1, tmq, tnq);
            }
            // free on the path and of the candidate's modulation level: only those channels can take it over -- all candidates of
            // the group at once, lane = (candidate, word)
            u64 acc_g;
            {
                const int gid_l = (int)((uint32_t)__shfl((int)rv, (lane & ~7) + 6) & 0xffffu);
                const bool on = gc < gsz && gd < W;
                acc_g = path_word<W>(occ, tb.recs, gid_l, gd < W ? gd : 0, on) & (on ? tmq : 0ull);
            }
            bool moved_in_group = false;
            int c = 0;
            for (; c < gsz; ++c) {
                const int l8 = 8 * c;
                const double diff = __hiloint2double(__builtin_amdgcn_readlane((int)rv, l8 + 1), __builtin_amdgcn_readlane((int)rv, l8));
                const uint32_t x5 = (uint32_t)__builtin_amdgcn_readlane((int)rv, l8 + 5);
                const int idx = (int)(x5 & 0xffffu), ch = (int)((x5 >> 16) & 0x1ffu);
                const int gid = (int)((uint32_t)__builtin_amdgcn_readlane((int)rv, l8 + 6) & 0xffffu);
                const OrlgPhySvc *r = grec + idx;
                const OrlgPathRec *rec = tb.recs + gid;
                u64 xw[W];
                u64 any = 0ull;
#pragma unroll
                for (int w = 0; w < W; ++w) { xw[w] = readlane64(acc_g, l8 + w); any |= xw[w]; }
                int l0 = -1, c0 = -1;
                double m0 = 0.0;
                if (any != 0ull) {
                    if (gnv && !rss) {
                        // cut metric of the lane's channels from D (LDS) and the path's node weights: an integer; the best channel
                        // = greatest metric, then lowest channel number, as ONE key.  Four rounds in five find a free channel of
                        // that level, one in fifteen moves: the vote comes first, the reduction only when it passes.
                        uint4 qa, qb;
                        qa.x = (uint32_t)__builtin_amdgcn_readlane((int)tnq, l8 + 0); qa.y = (uint32_t)__builtin_amdgcn_readlane((int)tnq, l8 + 1);
                        qa.z = (uint32_t)__builtin_amdgcn_readlane((int)tnq, l8 + 2); qa.w = (uint32_t)__builtin_amdgcn_readlane((int)tnq, l8 + 3);
                        qb.x = (uint32_t)__builtin_amdgcn_readlane((int)tnq, l8 + 4); qb.y = (uint32_t)__builtin_amdgcn_readlane((int)tnq, l8 + 5);
                        qb.z = (uint32_t)__builtin_amdgcn_readlane((int)tnq, l8 + 6); qb.w = (uint32_t)__builtin_amdgcn_readlane((int)tnq, l8 + 7);
                        const NvRec nr = nv_unpack(qa, qb);
                        int key = -1;
                        // -metric < diff with an integer metric and an integer-valued diff: metric + 1024 > 1024 - diff
                        const int kthr = ((1024 - (int)diff) << 9) | 511;
#pragma unroll
                        for (int w = 0; w < W; ++w) {
                            const u64 x = xw[w];
                            if (x == 0ull) continue;   // (wave-uniform: no free channel of that level in this word)
                            const int cc = 64 * w + lane;
                            const bool fr = ((x >> lane) & 1ull) && cc < p.C;
                            int sdot = nv_dot(nr.c, nv_get(gnv, cc, p.C)) - nr.cq;
                            if (nr.nchord) sdot -= nv_chords(occ, nr, cc, W);
                            const int kk = ((nr.wsum - 2 * sdot + 1024) << 9) | (511 - cc);   // |metric| <= sum of the weights < 1024
                            if (fr && kk > key) key = kk;
                        }
                        if (ballot(key > kthr) != 0ull) {
                            key = wave_max_i32(key);
                            l0 = 0; c0 = 511 - (key & 511); m0 = (double)((key >> 9) - 1024);
                        }
                    } else {
                        int lv[W];
                        double mtr[W];
                        uint32_t cols[W];
                        uint4 dv0[W];
#pragma unroll
                        for (int w = 0; w < W; ++w) dv0[w] = make_uint4(0u, 0u, 0u, 0u);
                        u64 acc1 = 0ull;   // the candidate's free words as phy_row_metrics takes them: word w on lane w
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            if (lane == w) acc1 = xw[w];
                        const uint8_t *mrow = p.mod_t + (size_t)__builtin_amdgcn_readlane((int)rv, l8 + 7) * p.cpad;   // (levels: not looked at, flat)
                        phy_columns<W>(occ, tb, p, lane, rss ? 1 : 0, cols, r0w);
                        phy_row_metrics<W>(occ, tb, p, acc1, 0, gid, mrow, lane, rss ? 1 : 0, true, lv, mtr, cols, r0w, dv0);
                        phy_row_best<W>(lv, mtr, lane, l0, m0, c0);  // sorted(key=(-metric, channel))[0]
                    }
                }
                if (l0 >= 0 && -1.0 * m0 < diff) {
                    // _move (:662-697): the service's channel list is read now -- the moved entry goes to its end
                    const uint32_t d3 = (uint32_t)uni((int)reinterpret_cast<const uint32_t *>(r)[3]);   // gid | nch << 16 | flags << 24
                    const int nch = (int)((d3 >> 16) & 0xffu), rflags = (int)(d3 >> 24);
                    const int mych = lane < nch ? (int)r->ch[lane] : 0xffff;
                    const u64 jm = ballot(lane < nch && (mych & 0x1ff) == ch && !(mych & (1 << 14)));
                    if (jm) {
                        const int jpos = ctz64(jm);
                        mc_before(occ, mc, c0, lane);
                        mc_before(occ, mc, ch, lane);
                        if (lane < rec->hops) {
                            u64 *rowp = occ + (int)rec->link[lane] * W;
                            rowp[c0 >> 6] &= ~(1ull << (c0 & 63));
                            rowp[ch >> 6] |= 1ull << (ch & 63);
                        }
                        wave_sync();
                        mc_after(occ, mc, c0, lane);
                        mc_after(occ, mc, ch, lane);
                        if (gnv) {
                            const uint4 cv4 = p.nvrec[2 * gid];
                            if (lane < 2) nv_update(gnv, cv4, lane == 0 ? c0 : ch, lane != 0);
                        }
                        const int nxtc = __shfl_down(mych, 1);
                        int nv2 = mych;
                        if (lane >= jpos && lane + 1 < nch) nv2 = nxtc;
                        if (lane == nch - 1) nv2 = c0 | (readlane64((u64)(uint32_t)mych, jpos) & 0xfe00u);
                        if (lane < nch) grec[idx].ch[lane] = (uint16_t)nv2;
                        {
                            const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane(nv2, 0), h1 = (uint32_t)__builtin_amdgcn_readlane(nv2, 1);
                            if (lane == 0) {
                                grec[idx].seq = (uint32_t)next_seq;
                                gsum[idx] = svc_summary(gid, rflags, nch, h0, nch > 1 ? h1 : 0u);
                                gseq[idx] = (uint32_t)next_seq;
                            }
                        }
                        next_seq += 1;
                        cmoves += 1;
                        moved_in_group = true;
                        wave_sync();
                    }
                }
                if (cmoves + gmoves > p.number_moves || moved_in_group) { c += 1; break; }
            }
            if (cmoves + gmoves > p.number_moves) break;
            q0 += c;                 // (the candidates behind a move see the new occupancy: their group is read again)
            if (moved_in_group) fresh = true;
        }
        cycles = cmoves != 0 ? 1 : 0;
    }
    if (lane == 0) {
        ws->counted_moves_groom = gmoves;
        ws->counted_moves += cmoves;
        ws->counted_defrag_cycles += cycles;
        if (overflow) ws->q_overflow |= 2;
    }
    wave_sync();
}
