// orlg_usage.h -- most-used spectrum assignment and the route that takes the best window over all candidate paths (DESIGN 2.25;
// include/orlg.h orlg_step_window, orlg_slot_usage, orlg_path_most_used).  With A, n and WINDOW as orlg_assign.h has them:
//     U[t]        = the number of links of the topology (all E) on which slot t is occupied, t in 0 .. S - 1;  0 .. E, E <= 255
//     usage(p, s) = U[s] + .. + U[s + n - 1] for a window start s of path p;  0 .. 255 * 512, 17 bits
// The rule MOST_USED takes the window with the largest usage, ties to the lowest start; the route BEST_WINDOW lets every path that
// has a window propose its rule window and takes the proposal that ranks best by the rule's own order, ties to the lowest path
// (FIRST_FULL: lower start; LAST: higher start; BEST: shorter block, lower start; EXACT: a block of exactly n first, lower start;
// MOST_USED: higher usage, lower start).  Not in the reference; integer-exact; U is recomputed from the occupancy a step meets.
//
// The usage pass (usage_prefix): slot-per-lane extraction, four slots to a lane.  A row of 16 lanes takes one word of the bitmaps
// at a time, lane gl its slots 4 gl .. 4 gl + 3; per link the lanes of a row read the SAME word (an LDS broadcast), cut their
// nibble out and spread it into the four bytes of one register (a multiply), so ONE add counts four slots and E <= 255 keeps a
// byte from overflowing.  Then a DPP prefix scan along the row, the words' totals carried on, and the inclusive prefix sums
// I[t] = U[0] + .. + U[t] go to LDS as int32 (64 W of them per environment, 16 bytes a lane and word):
//     usage(p, s) = I[s + n - 1] - (s ? I[s - 1] : 0).
// The group kernel's row is its environment (ROWS = 1); the wave kernel and the query kernel give an environment all four rows
// (ROWS = 4, word r + 4 i on row r).  Bit-sliced counters on the (path, word) lanes -- eight 64-bit planes, a ripple carry per
// link, as cut_word_key counts hops -- were the other shape: 48 VALU operations per link and word against 5 here, and the counts
// would still have to be taken out of the planes slot by slot for the sums.
//
// The rule (usage_word_key), on the (path, word) lanes of orlg_assign.h: the lane walks the window starts of its own word and keeps
// the largest key usage << 10 | (1023 - start) -- 27 bits, never 0; ONE maximum over the path's lanes decides, as for every rule.
// The whole wave takes part: DPP moves and ballots stand outside conditions, words past an end are read at a valid address.
#pragma once
#include "../../include/orlg.h"
#include "orlg_assign.h"
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

DEV int usage_row_add(int v) { v += dpp_xor1(v); v += dpp_xor2(v); v += dpp_half_mirror(v); v += dpp_row_mirror(v); return v; }

// I[0 .. 64 W) of one environment from its occupancy (LDS; bit set = free, slots at and beyond S stored as not free) into `incl`
// (LDS, 16-byte aligned).  ROWS = 1: every row of the wave works on its own environment (occ, incl: the row's); ROWS = 4: the
// wave's four rows share one.  The caller synchronises the wave before it reads incl.
template <int W, int ROWS>
DEV void usage_prefix(const u64 *occ, int32_t *incl, int E, int S, int lane) {
    static_assert(ROWS == 1 || ROWS == 4, "one environment per row or per wave");
    const int gl = lane & 15, r = ROWS == 1 ? 0 : lane >> 4;
    int carry = 0;   // U summed over the words before this pass
#pragma unroll
    for (int i = 0; i < (W + ROWS - 1) / ROWS; ++i) {
        const int j = r + ROWS * i;
        const bool on = j < W;
        const int jc = on ? j : W - 1;   // (a row past the last word reads it and stores nothing)
        uint32_t freec = 0u;            // four byte counters: the links on which slots 64 j + 4 gl + 0 .. 3 are free
#pragma unroll 4
        for (int e = 0; e < E; ++e) {
            const uint32_t nib = (uint32_t)(occ[e * W + jc] >> (4 * gl)) & 15u;
            freec += (nib * 0x00204081u) & 0x01010101u;   // bit b of the nibble -> bit 8 b
        }
        const int t0 = 64 * j + 4 * gl;
        int c[4], run = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            run += t0 + b < S ? E - (int)((freec >> (8 * b)) & 0xffu) : 0;
            c[b] = run;
        }
        // inclusive scan of the lanes' totals along the row, then the row's own total
        int v = run;
        v += lane_back_i32<1>(v);
        v += lane_back_i32<2>(v);
        v += lane_back_i32<4>(v);
        v += lane_back_i32<8>(v);
        const int tot = usage_row_add(run);
        int off = carry;
        if (ROWS == 1) {
            carry += tot;
        } else {
            const int q0 = __builtin_amdgcn_readlane(tot, 0), q1 = __builtin_amdgcn_readlane(tot, 16);
            const int q2 = __builtin_amdgcn_readlane(tot, 32), q3 = __builtin_amdgcn_readlane(tot, 48);
            off += (r > 0 ? q0 : 0) + (r > 1 ? q1 : 0) + (r > 2 ? q2 : 0);
            carry += q0 + q1 + q2 + q3;
        }
        const int before = off + v - run;
        if (on) *reinterpret_cast<int4 *>(incl + t0) = make_int4(before + c[0], before + c[1], before + c[2], before + c[3]);
    }
}

// The MOST_USED key of THIS lane's word of a path: usage << 10 | (1023 - start) of the lane's best window, 0 = the word holds no
// window start -- a maximum over the path's lanes is the path's MOST_USED window.  x: the lane's word of the path-wide bitmap
// (slots at and beyond S not free, 0 on an inactive lane); n: slots of the request on this path.
template <int W>
DEV uint32_t usage_word_key(const int32_t *incl, u64 x, int n, int w) {
    u64 c = run_starts<W>(x, n, w);
    uint32_t best = 0u;
    while (ballot(c != 0ull) != 0ull) {
        if (c != 0ull) {
            const int s = 64 * w + ctz64(c);
            c &= c - 1ull;
            const int hi = incl[s + n - 1], lo = incl[s > 0 ? s - 1 : 0];
            const uint32_t key = (uint32_t)(hi - (s > 0 ? lo : 0)) << 10 | (uint32_t)(1023 - s);
            best = key > best ? key : best;
        }
    }
    return best;
}
DEV int usage_key_slot(uint32_t key) { return 1023 - (int)(key & 1023u); }
DEV int usage_key_usage(uint32_t key) { return (int)(key >> 10); }

// a rule of orlg_step_window: the four of orlg_assign.h, or MOST_USED (rule: wave-uniform)
template <int W>
DEV uint32_t window_word_key(const int32_t *incl, u64 x, int n, int w, int rule) {
    if (rule == ORLG_ASSIGN_MOST_USED) return usage_word_key<W>(incl, x, n, w);
    return assign_word_key<W>(x, n, w, rule);
}
DEV int window_key_slot(uint32_t key, int rule) { return rule == ORLG_ASSIGN_MOST_USED ? usage_key_slot(key) : assign_key_slot(key, rule); }

// wave_assign (orlg_assign.h) for orlg_step_window: (path << 10) | slot of the request under route `route` (ORLG_POLICY_SP / SAP /
// LLP / PATH_EXT as there, or ORLG_POLICY_BEST_WINDOW: of all K paths the one whose rule window ranks best, ties to the lowest
// path) and rule `rule`, or -1 = no path of the route has a window.  A key is larger for the better window under every rule, and
// across paths it orders the proposals as the rule orders them, so the ranked routes take the maximum of a rank --
// llp's free slots, or the key itself, 27 bits: too wide to share a register with the group's number -- and then the lowest group
// that holds it.  Across passes the comparison is strict, so the earlier pass wins a tie.  incl: the environment's prefix sums,
// filled here when the rule asks for them.  Wave-uniform result.
template <int W>
DEV int wave_window_assign(const u64 *occ, int32_t *incl, const Tab &tb, int base, int K, int E, int S, int br, int lane, int route, int rule,
                           int given) {
    const int g8 = lane >> 3, w = lane & 7;
    int path0 = 0, kmax = route == ORLG_POLICY_SP ? 1 : K;
    if (route == ORLG_POLICY_PATH_EXT) {
        if (given < 0 || given >= K) return -1;
        path0 = given;
        kmax = 1;
    }
    if (rule == ORLG_ASSIGN_MOST_USED) {
        usage_prefix<W, 4>(occ, incl, E, S, lane);
        wave_sync();
    }
    const bool llp = route == ORLG_POLICY_LLP, ranked = llp || route == ORLG_POLICY_BEST_WINDOW;
    int found = -1, top = 0;
    for (int p0 = 0; p0 < kmax; p0 += 8) {
        const int idp = p0 + g8;
        const bool on = idp < kmax && w < W;
        int se_l, hops_l;
        const u64 x = path_word_rec<W>(occ, tb.recs, base + path0 + idp, w, on, se_l, hops_l) & valid_mask(S, w);
        int n = 1;
        if (on) n = tb.nslots[br * ORLG_NSLOT_STRIDE + se_l];
        const int key = group8_max((int)window_word_key<W>(incl, x, n, w, rule));   // the path's key on every lane of its group
        if (ranked) {
            const int fs = group8_add(popc64(x));
            const int rank = key ? (llp ? fs : key) : 0;
            const int m = wave_max_i32(rank);
            if (m > top) {
                const int g = ctz64(ballot(rank == m && w == 0)) >> 3;   // the lowest path of the pass that holds the maximum
                top = m;
                found = ((p0 + g) << 10) | window_key_slot((uint32_t)__builtin_amdgcn_readlane(key, g << 3), rule);
            }
        } else {
            const u64 m = ballot(key != 0 && w == 0);
            if (m) {
                const int g = ctz64(m) >> 3;
                found = ((path0 + p0 + g) << 10) | window_key_slot((uint32_t)__builtin_amdgcn_readlane(key, g << 3), rule);
                break;
            }
        }
    }
    return found;
}

// orlg_slot_usage and orlg_path_most_used (include/orlg.h): U [B][S] uint8; the MOST_USED window of every candidate path of every
// pending request -- usage [B][K] int32 (-1 = the path has no window), slots [B][K] int16 (S there); a null array is not written.
// The shape of orlg_min_cuts_kernel: tables staged once per workgroup, one wave per environment at a time, the grid striding over
// the batch, the occupancy row copied to LDS, the prefix sums behind it.  Reads state and writes only its outputs.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_usage_kernel(const OrlgParams p, uint8_t *slot_usage, int32_t *usage,
                                                                                        int16_t *slots) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int occ_bytes = (p.NW * 8 + 15) & ~15;
    unsigned char *wb = smem + p.l_shared_bytes + (size_t)wib * (occ_bytes + ORLG_USAGE_BYTES(W));
    u64 *occ = reinterpret_cast<u64 *>(wb);
    int32_t *incl = reinterpret_cast<int32_t *>(wb + occ_bytes);
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const bool wide = (p.NW & 1) == 0;
    const int g8 = lane >> 3, w = lane & 7;
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = sc->req_src, dst = sc->req_dst, br = sc->req_br;
        if (wide) copy_words(occ, p.occ + (size_t)env * p.NW, p.NW * 8, lane);
        else {
            const u64 *g = p.occ + (size_t)env * p.NW;
            for (int i = lane; i < p.NW; i += 64) occ[i] = g[i];
        }
        wave_sync();
        usage_prefix<W, 4>(occ, incl, p.E, p.S, lane);
        wave_sync();
        if (slot_usage)
            for (int t = lane; t < p.S; t += 64) slot_usage[(size_t)env * p.S + t] = (uint8_t)(incl[t] - (t > 0 ? incl[t - 1] : 0));
        if (usage || slots) {
            const int base = tb.pair_base[src * p.N + dst];
            for (int p0 = 0; p0 < p.K; p0 += 8) {
                const int idp = p0 + g8;
                const bool on = idp < p.K && w < W;
                int se_l, hops_l;
                const u64 x = path_word_rec<W>(occ, tb.recs, base + idp, w, on, se_l, hops_l) & valid_mask(p.S, w);
                int n = 1;
                if (on) n = tb.nslots[br * ORLG_NSLOT_STRIDE + se_l];
                const uint32_t key = (uint32_t)group8_max((int)usage_word_key<W>(incl, x, n, w));
                if (on && w == 0) {
                    const size_t o = (size_t)env * p.K + idp;
                    if (usage) usage[o] = key ? usage_key_usage(key) : -1;
                    if (slots) slots[o] = (int16_t)(key ? usage_key_slot(key) : p.S);
                }
            }
        }
        wave_sync();
    }
}
