// orlg_query_kernels.hip -- kernels that read the RMSA / DeepRMSA state and write only the caller's buffers:
// orlg_path_masks_kernel (one environment's path-wide free bitmaps and slot counts) and orlg_deeprmsa_obs_kernel (the DeepRMSA
// observation, and its action mask, for the whole batch).  The whole-batch valid-action masks are orlg_mask_kernels.hip.
//
// Reference: optical_rl_gym/envs/rmsa_env.py get_number_slots :708-719, get_available_slots :745-756, get_available_blocks
// :774-804; deeprmsa_env.py step :48-58, observation :60-121.
#pragma once
#include "orlg_rmsa_layout.h"
#include "orlg_spectrum.h"

// For env `env_index`: the k path-wide free bitmaps of its pending request and get_number_slots per path
// (rmsa_env.py:708-719, 745-756).  One wave.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE) void orlg_path_masks_kernel(const OrlgParams p, int env, int gid0, int count,
                                                                    u64 *masks, int32_t *nslots) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    u64 *occ = reinterpret_cast<u64 *>(smem + p.l_shared_bytes);
    const u64 *g = p.occ + (size_t)env * p.NW;
    for (int i = lane; i < p.NW; i += 64) occ[i] = g[i];
    wave_sync();
    const OrlgEnvScalars *sc = p.scal + env;
    // gid0 < 0: the k candidate paths of the pending request; otherwise `count` records starting at gid0
    const int base = gid0 < 0 ? tb.pair_base[sc->req_src * p.N + sc->req_dst] : gid0;
    const int cnt = gid0 < 0 ? p.K : count;
    const int pp = lane / W, pw = lane - pp * W;
    {
        u64 m = path_word<W>(occ, tb.recs, base + pp, pw, pp < cnt);
        if (pp < cnt) masks[pp * W + pw] = m;
    }
    if (lane < cnt) nslots[lane] = tb.nslots[sc->req_br * ORLG_NSLOT_STRIDE + tb.recs[base + lane].se];
}

// DeepRMSAEnv.observation() (deeprmsa_env.py:60-121) for every env.  One wave per env at a time: the grid is sized to the
// device and strides over the environments (the topology tables are staged once per workgroup).  The per-path integers
// (block starts / lengths, slots needed, free slots, free runs) are found with wave-uniform scans and parked in LDS; then
// lane i evaluates element i of the vector -- one fp64 division sequence for all elements -- and the row leaves coalesced.
// mask != nullptr: the DeepRMSA action mask [B][mask_dim] leaves the same launch -- action a < K * J is valid iff block a % J of
// path a / J exists, i.e. the path has more than a % J free runs of at least get_number_slots slots (deeprmsa_env.py:48-58,
// rmsa_env.py:774-804), which is what the block scan has just parked: a start >= 0; the column beyond K * J (the explicit
// rejection) is always valid.  mask == nullptr: the kernel writes what it wrote before the mask existed.  p.o_obs == nullptr
// (only with a mask): the mask alone.
template <int W>
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_deeprmsa_obs_kernel(const OrlgParams p, uint8_t *mask,
                                                                                                int mask_dim) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int occ_bytes = (p.NW * 8 + 15) & ~15, obs_bytes = (p.obs_dim * 8 + 15) & ~15;
    unsigned char *wb = smem + p.l_shared_bytes + (size_t)wib * (occ_bytes + obs_bytes);
    u64 *occ = reinterpret_cast<u64 *>(wb);
    int *opa = reinterpret_cast<int *>(wb + occ_bytes);   // [obs_dim] integer operand of element i
    int *opb = opa + p.obs_dim;                            // [obs_dim] second operand (free runs) where needed
    const int N = p.N, K = p.K, S = p.S, J = p.j;
    const int PW = 2 * J + 3, head = 1 + 2 * N;
    const uint32_t pw_inv = (65536u + (uint32_t)PW - 1u) / (uint32_t)PW;
    const uint32_t j_inv = (65536u + (uint32_t)J - 1u) / (uint32_t)J;   // (a / J as r / PW below: a < K * J <= 64 * J, J <= 16)
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const bool wide = (p.NW & 1) == 0;
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        const OrlgEnvScalars *sc = p.scal + env;
        const int src = sc->req_src, dst = sc->req_dst, br = sc->req_br;
        if (wide) copy_words(occ, p.occ + (size_t)env * p.NW, p.NW * 8, lane);
        else {
            const u64 *g = p.occ + (size_t)env * p.NW;
            for (int i = lane; i < p.NW; i += 64) occ[i] = g[i];
        }
        wave_sync();
        const int mn = src < dst ? src : dst, mx = src < dst ? dst : src;
        const int base = tb.pair_base[src * N + dst];
        if (K <= 8) {
            // every candidate path at once: path g on the 8-lane group g (two groups per DPP row), one word per lane
            const int g8 = lane >> 3, w = lane & 7;
            const bool on = g8 < K && w < W;
            int se_l, hops_l;
            const u64 x = path_word_rec<W>(occ, tb.recs, base + g8, w, on, se_l, hops_l);
            int n = 1;
            if (on) n = tb.nslots[br * ORLG_NSLOT_STRIDE + se_l];
            const u64 xprev = lane_prev_u64(x);
            const u64 starts = x & ~((x << 1) | (w > 0 ? xprev >> 63 : 0ull));   // first slots of the free runs
            const u64 bs = starts & run_starts<W>(x, n, w);                        // ... of those with >= n slots: the blocks
            // free slots continuing a run that reaches this word's end (as in link_stats_update)
            const int lead = x == ~0ull ? 64 : ctz64(~x);
            const int nlead_raw = lane_next_i32(lead);
            const int nlead = w < W - 1 ? nlead_raw : 0;
            int e = nlead;
#pragma unroll
            for (int i = 0; i < W - 2; ++i) {
                const int ne_raw = lane_next_i32(e);
                const int ne = w < W - 1 ? ne_raw : 0;
                e = nlead == 64 ? 64 + ne : nlead;
            }
            // blocks in the words before this one (prefix sum over the group's lanes)
            const int cnt = popc64(bs);
            int incl = cnt, o;
            o = lane_back_i32<1>(incl); if (w >= 1) incl += o;
            o = lane_back_i32<2>(incl); if (w >= 2) incl += o;
            o = lane_back_i32<4>(incl); if (w >= 4) incl += o;
            const int n_blocks = group8_add(cnt), total = group8_add(popc64(x)), runs = group8_add(popc64(starts));
            int *row = opa + head + g8 * PW;
            for (int b = 0; b < J; ++b) {
                const int kth = b - (incl - cnt);   // which block of this word
                u64 m = bs;
                for (int q = 0; q < J; ++q)
                    if (q < kth) m &= m - 1;
                if (on && kth >= 0 && kth < cnt) {
                    const int sb = ctz64(m);
                    row[2 * b] = 64 * w + sb;
                    row[2 * b + 1] = free_run_length((~x) >> sb, 64 - sb + e);
                }
                if (on && w == 0 && b >= n_blocks) { row[2 * b] = -1; row[2 * b + 1] = -1; }
            }
            if (on && w == 0) {
                row[2 * J] = n; row[2 * J + 1] = total; row[2 * J + 2] = total;
                opb[head + g8 * PW + 2 * J + 2] = runs;
            }
        } else {
            const int pp = lane / W, pw = lane - pp * W;
            u64 acc = 0ull;
            acc = path_word<W>(occ, tb.recs, base + pp, pw, pp < K);
            int my_se = 0;
            if (lane < K) my_se = tb.recs[base + lane].se;
            int my_n = tb.nslots[br * ORLG_NSLOT_STRIDE + my_se];
            for (int idp = 0; idp < K; ++idp) {
                u64 x[W];
    #pragma unroll
                for (int w = 0; w < W; ++w) x[w] = readlane64(acc, idp * W + w);
                const int n = __builtin_amdgcn_readlane(my_n, idp);
                int *row = opa + head + idp * PW;
                for (int b = 0; b < J; ++b) {
                    int len = 0;
                    int s0 = find_block<W>(x, n, b, lane, &len);
                    if (lane == 0) { row[2 * b] = s0; row[2 * b + 1] = s0 >= 0 ? len : -1; }
                }
                int total = 0, runs = 0;
    #pragma unroll
                for (int w = 0; w < W; ++w) {
                    u64 carry = w > 0 ? (x[w > 0 ? w - 1 : 0] >> 63) : 0ull;
                    total += popc64(x[w]);
                    runs += popc64(x[w] & ~((x[w] << 1) | carry));
                }
                if (lane == 0) {
                    row[2 * J] = n; row[2 * J + 1] = total; row[2 * J + 2] = total;
                    opb[head + idp * PW + 2 * J + 2] = runs;
                }
            }
        }
        wave_sync();
        if (mask) {   // lane a = action a: one row of bytes per environment
            uint8_t *mrow = mask + (size_t)env * mask_dim;
            for (int a = lane; a < mask_dim; a += 64) {
                const int route = (int)(((uint32_t)a * j_inv) >> 16), block = a - route * J;
                mrow[a] = (uint8_t)(route >= K || opa[head + route * PW + 2 * block] >= 0 ? 1 : 0);
            }
        }
        double *gout = p.o_obs + (size_t)env * p.obs_dim;
        float *gout32 = reinterpret_cast<float *>(p.o_obs) + (size_t)env * p.obs_dim;   // (obs_f32: the same vector rounded once)
        const int br_val = tb.bit_rates[br];
        for (int i = p.o_obs ? lane : p.obs_dim; i < p.obs_dim; i += 64) {
            // element i = num / den (one division for every kind of element), optionally followed by (q - 4) / 4
            double num = 0.0, den = 1.0, res;
            bool fixed = false, tail = false;
            double fixed_val = 0.0;
            if (i == 0) {
                num = (double)br_val; den = 100.0;                                   // bit_rate / 100
            } else if (i < head) {
                fixed = true; fixed_val = (i - 1 == mn || i - 1 == N + mx) ? 1.0 : 0.0;   // one-hot endpoints
            } else {
                // (r / PW by multiply-shift: exact for every r < 64 * PW, PW <= 35, checked exhaustively; r < K * PW with K <= 64 -- an integer division by a run-time value is ~30 instructions)
                const int r = i - head, c = r - (int)(((uint32_t)r * pw_inv) >> 16) * PW;
                const int v = opa[i];
                if (c < 2 * J) {
                    if (v < 0) { fixed = true; fixed_val = -1.0; }
                    else if ((c & 1) == 0) { num = 2 * ((double)v - 0.5 * S); den = (double)S; }   // 2 * (start - S/2) / S
                    else { num = (double)v - 8; den = 8.0; }                                        // (length - 8) / 8
                } else if (c == 2 * J) {
                    num = (double)v - 5.5; den = 3.5;                                               // (slots - 5.5) / 3.5
                } else if (c == 2 * J + 1) {
                    num = 2 * ((double)v - 0.5 * S); den = (double)S;                               // 2 * (free - S/2) / S
                } else {
                    const int runs = opb[i];
                    if (runs > 0) { num = (double)v; den = (double)runs; tail = true; }              // (free / runs - 4) / 4
                    else { fixed = true; fixed_val = -1.0; }
                }
            }
            res = num / den;
            if (tail) res = (res - 4) * 0.25;   // (x / 4 is x * 0.25 exactly)
            const double val = fixed ? fixed_val : res;
            if (p.obs_f32) gout32[i] = (float)val; else gout[i] = val;
        }
        wave_sync();
    }
}
