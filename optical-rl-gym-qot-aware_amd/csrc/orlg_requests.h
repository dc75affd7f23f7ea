// orlg_requests.h -- the arrival ring's producers, shared by the three step kernels (orlg_kernels.hip, orlg_group_kernels.hip,
// orlg_phy_kernels.hip).
//
// Every step kernel takes a service's arrival from a ring of ORLG_RING pre-generated requests (three rows: inter-arrival time,
// holding time, src | dst << 8 | bit-rate index << 16) and refills the ring when it runs dry, from one of three producers:
//     refill_requests         MT19937, discrete bit rates
//     refill_requests_cont    MT19937, bit_rate_selection="continuous"
//     refill_requests_trace   a caller's trace
// The wave-per-environment kernel keeps the generator in its own LDS region; the other two stage an environment's generator from
// HBM through a workgroup buffer behind a lock, call the producer, and then wait for the ring entries (ring_visible).  That
// staging sequence stays written out in both.  As one inline function (refill_staged) it changed VGPRs, scratch or spilled VGPRs
// of 99 of the library's 742 kernels against the parent commit: 92 of the 480 orlg_phy_kernel instantiations (76 with more scratch
// or spills, 19 with less; the worst, <1,false,false,3,true,false>: scratch 32 -> 128 B per lane, spilled VGPRs 7 -> 12) and 7
// of the 147 orlg_rmsa_group_kernel ones (6 up, 1 down; the worst, <3,2,false,false,true>: spilled VGPRs 47 -> 49).  The headline's
// orlg_rmsa_group_kernel<5,2,false,true> kept 168 VGPRs, 352 B scratch and 94 spilled VGPRs either way.
//
// orlg_env_rates: the arrival process of one environment of a handle with per-environment traffic.
#pragma once
#include "orlg_wave.h"   // DEV, wave_sync, recip_refine, div_by

// The producers are out of line, so their pointers carry their address space in the signature: through generic pointers every
// access of the MT19937 state and the tables in LDS was a flat instruction.
typedef __attribute__((address_space(3))) uint32_t orlg_lds_u32;
typedef __attribute__((address_space(3))) double orlg_lds_f64;
typedef __attribute__((address_space(3))) const double orlg_lds_cf64;
typedef __attribute__((address_space(1))) uint32_t orlg_glb_u32;
typedef __attribute__((address_space(1))) double orlg_glb_f64;
typedef __attribute__((address_space(1))) const double orlg_glb_cf64;
typedef __attribute__((address_space(1))) const uint32_t orlg_glb_cu32;

// ---------------------------------------------------------------------------------------- MT19937
// Regenerate all 624 words in place (CPython _randommodule.c genrand_uint32).  Sub-round r handles
// kk = 64r + lane; mt[kk+1] is still old (same or later sub-round), mt[kk+397] is old for kk < 227 and
// mt[kk-227] is already new for kk >= 227, exactly as in the sequential loop.
template <typename MT /* pointer to the 624 state words: generic or LDS-qualified */>
DEV void mt_regenerate(MT mt, int lane) {
    for (int r = 0; r < 10; ++r) {
        int kk = 64 * r + lane;
        uint32_t v = 0;
        if (kk < ORLG_MT_N) {
            int k1 = kk + 1 == ORLG_MT_N ? 0 : kk + 1;
            int ks = kk < ORLG_MT_N - ORLG_MT_M ? kk + ORLG_MT_M : kk - (ORLG_MT_N - ORLG_MT_M);
            uint32_t y = (mt[kk] & 0x80000000u) | (mt[k1] & 0x7fffffffu);
            v = mt[ks] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        wave_sync();
        if (kk < ORLG_MT_N) mt[kk] = v;
        wave_sync();
    }
}
DEV uint32_t mt_temper(uint32_t y) {
    y ^= (y >> 11); y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= (y >> 18);
    return y;
}
// random.random() from two consecutive tempered words
DEV double mt_random(uint32_t a, uint32_t b) { return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0); }

// ---------------------------------------------------------------------------------------- a request from its uniform variates
// the two expovariate() draws (rmsa_env.py:646-650): inter-arrival and holding time
DEV void request_times(double u0, double u1, double lam_arrival, double lam_holding, double &iat, double &ht) {
    const double ylam_arrival = recip_refine(lam_arrival), ylam_holding = recip_refine(lam_holding);
    iat = div_by(-orlg_log(1.0 - u0), lam_arrival, ylam_arrival);
    ht = div_by(-orlg_log(1.0 - u1), lam_holding, ylam_holding);
}
// (The two random.choices() counts for source and destination stay written out in both generators: as one function from
// (u2, u3, src_cum, dst_cum, N) to (src, dst) they changed the generators' code -- the same instructions in another order with
// other registers -- and with it, through the registers a caller keeps across the call, the figures of their callers: 33 kernels
// more than without it differed from the parent's, among them 10 of the wave units' (7 with more scratch or spills, 3 with less;
// orlg_rmsa_kernel_ff<2,2,false>: scratch 144 -> 176 B per lane, orlg_rmsa_reset_kernel<4,0>: 32 -> 48 B, spilled VGPRs 7 -> 9).)

// ---------------------------------------------------------------------------------------- per-environment traffic
// (arrival_lambda, holding_lambda) of environment `env` (wave-uniform) of a handle with per-environment traffic; a handle without
// (rates == nullptr) keeps the two scalars the caller passes in.  The table is written before the handle's first launch and never
// after, so it is read through the constant address space: the pair arrives by the scalar cache in four SGPRs at the place that
// uses it -- no vector register, nothing kept across the step
DEV void orlg_env_rates(const OrlgRates *rates, int env, double &arrival_lambda, double &holding_lambda) {
    if (rates) {
        typedef const OrlgRates __attribute__((address_space(4))) *ConstRates;
        ConstRates r = (ConstRates)(uintptr_t)rates + __builtin_amdgcn_readfirstlane(env);
        arrival_lambda = r->arrival_lambda;
        holding_lambda = r->holding_lambda;
    }
}
// ---------------------------------------------------------------------------------------- the ring
// Lane j's entry into slot j of the ring's three rows.  RING_LDS: the ring lives in LDS (wave-per-environment kernel) or in HBM
// (the other two).  A refill of n requests passes zeros in the lanes past n: those entries are dead, and a snapshot of the state
// must not depend on what the ring held before.
template <bool RING_LDS>
DEV void ring_store(void *ring_iat_v, void *ring_ht_v, void *ring_req_v, int lane, double iat, double ht, uint32_t rq) {
    if (RING_LDS) {
        ((orlg_lds_f64 *)ring_iat_v)[lane] = iat; ((orlg_lds_f64 *)ring_ht_v)[lane] = ht; ((orlg_lds_u32 *)ring_req_v)[lane] = rq;
    } else {
        ((orlg_glb_f64 *)ring_iat_v)[lane] = iat; ((orlg_glb_f64 *)ring_ht_v)[lane] = ht; ((orlg_glb_u32 *)ring_req_v)[lane] = rq;
    }
    wave_sync();
}
// After a refill of a ring in HBM: the entries other lanes wrote are read back by this wave, so the stores have to be complete
// (same CU: the vector cache is write-through and coherent for its own CU's stores, no L2 write-back / invalidate needed).
DEV void ring_visible() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    wave_sync();
}

// ---------------------------------------------------------------------------------------- producers
// Pre-generate arrivals, one per lane (_next_service's five random() draws each: inter-arrival, holding time, source,
// destination, bit rate -- rmsa_env.py:646-659, optical_network_env.py:197-206).  The arrival process does not depend
// on the network state, so lane j produces request j of the RNG stream: words [idx + 10 j, idx + 10 j + 10).  At most
// one MT19937 regeneration happens inside a refill (n is capped accordingly), exactly where the sequential
// generator would do it.  Returns count | new index << 8.
template <bool RING_LDS>
__device__ __noinline__ int refill_requests_as(orlg_lds_u32 *mt, void *ring_iat_v, void *ring_ht_v, void *ring_req_v,
                                               orlg_lds_cf64 *src_cum, orlg_lds_cf64 *dst_cum, orlg_lds_cf64 *br_cum, int idx,
                                               int N, int NBR, double lam_arrival, double lam_holding, int env) {
    // out of line on purpose: it runs once per ~62 steps and must not add register pressure to the step loop
    const int lane = threadIdx.x & 63;
    int n = (2 * ORLG_MT_N - idx) / 10;
    n = n > ORLG_RING ? ORLG_RING : n;
    // A freshly seeded generator (idx == 624: every environment's first refill) hands out 62 - env % 56 requests instead of 62.
    // The request stream is the same whatever a refill's size; what changes is WHEN the environments run dry: batches stepped
    // one launch per step (agent-driven) otherwise refill all at once every 62nd launch, one after the other behind the
    // workgroup's staging-buffer lock.
#ifndef ORLG_EXP_NO_STAGGER   // (experiment: every environment refills in the same launch, the other 61 of 62 launches none)
    if (idx == ORLG_MT_N) { const int cap = 62 - env % 56; n = n > cap ? cap : n; }
#endif
    uint32_t w[10];
    const int g0 = idx + 10 * lane;
#pragma unroll
    for (int k = 0; k < 10; ++k) w[k] = (lane < n && g0 + k < ORLG_MT_N) ? mt[g0 + k] : 0u;
    if (idx + 10 * n > ORLG_MT_N) {
        mt_regenerate(mt, lane);
#pragma unroll
        for (int k = 0; k < 10; ++k)
            if (lane < n && g0 + k >= ORLG_MT_N) w[k] = mt[g0 + k - ORLG_MT_N];
        idx = idx + 10 * n - ORLG_MT_N;
    } else {
        idx += 10 * n;
    }
    double u[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) u[q] = mt_random(mt_temper(w[2 * q]), mt_temper(w[2 * q + 1]));
    double iat, ht;
    request_times(u[0], u[1], lam_arrival, lam_holding, iat, ht);
    // random.choices: bisect_right(cum, u * total, 0, n - 1) = #{i < n - 1 : cum[i] <= x}
    int src = 0, dst = 0, bri = 0;
    {
        const double x = u[2] * (src_cum[N - 1] + 0.0);
        for (int i = 0; i < N - 1; ++i) src += src_cum[i] <= x ? 1 : 0;
    }
    {
        orlg_lds_cf64 *row = dst_cum + src * N;
        const double x = u[3] * (row[N - 1] + 0.0);
        for (int i = 0; i < N - 1; ++i) dst += row[i] <= x ? 1 : 0;
    }
    {
        const double x = u[4] * (br_cum[NBR - 1] + 0.0);
        for (int i = 0; i < NBR - 1; ++i) bri += br_cum[i] <= x ? 1 : 0;
    }
    // entries past n are dead; they are zeroed so that a snapshot of the state does not depend on what the ring held before
    const double o_iat = lane < n ? iat : 0.0, o_ht = lane < n ? ht : 0.0;
    const uint32_t o_rq = lane < n ? ((uint32_t)src | ((uint32_t)dst << 8) | ((uint32_t)bri << 16)) : 0u;
    ring_store<RING_LDS>(ring_iat_v, ring_ht_v, ring_req_v, lane, o_iat, o_ht, o_rq);
    return n | (idx << 8);
}
// the callers' form: generic pointers in, the new MT19937 index through idx_io, returns the number of requests written
template <bool RING_LDS>
DEV int refill_requests(uint32_t *mt, double *ring_iat, double *ring_ht, uint32_t *ring_req, const double *src_cum,
                        const double *dst_cum, const double *br_cum, int *idx_io, int N, int NBR, double lam_arrival,
                        double lam_holding, int env) {
    const int r = refill_requests_as<RING_LDS>((orlg_lds_u32 *)mt, ring_iat, ring_ht, ring_req, (orlg_lds_cf64 *)src_cum,
                                               (orlg_lds_cf64 *)dst_cum, (orlg_lds_cf64 *)br_cum, *idx_io, N, NBR, lam_arrival,
                                               lam_holding, env);
    *idx_io = r >> 8;
    return r & 0xff;
}

// bit_rate_selection="continuous" (rmsa_env.py:95-101, 655-659): the bit rate is rng.randint(lower, higher) = lower +
// _randbelow(width), CPython's _randbelow_with_getrandbits: k = width.bit_length(); r = getrandbits(k) -- one MT19937 word
// shifted right by 32 - k -- until r < width.  A request then consumes eight words for its four random() values and a
// VARIABLE number for the bit rate, so request j no longer starts at a known word.  Two phases: (1) one walk over the word
// stream, wave-uniform, that only looks at the bit-rate words -- where every request starts and which r it accepts (~25
// instructions per request); (2) lane j computes request j from its eight words like the discrete generator.  A refill
// stays inside the state's current 624 words; the request that straddles a regeneration is generated alone, word by word.
// The ring entry holds r (the index into the table of the width bit rates lower .. higher).  Returns count | new index << 8.
template <bool RING_LDS>
__device__ __noinline__ int refill_requests_cont_as(orlg_lds_u32 *mt, void *ring_iat_v, void *ring_ht_v, void *ring_req_v,
                                                    orlg_lds_cf64 *src_cum, orlg_lds_cf64 *dst_cum, int idx, int N, int width,
                                                    double lam_arrival, double lam_holding) {
    const int lane = threadIdx.x & 63;
    const int sh = 32 - (32 - __builtin_clz((unsigned)width));   // 32 - k, k = width.bit_length()
    if (idx >= ORLG_MT_N) { mt_regenerate(mt, lane); idx = 0; }
    // phase 1: the requests that lie inside [idx, 624)
    int n = 0, my_off = 0, my_r = 0, off = idx;
    for (; n < ORLG_RING; ++n) {
        int w = off + 8;
        if (w >= ORLG_MT_N) break;
        int r = 0;
        bool got = false;
        while (w < ORLG_MT_N) {
            r = (int)(mt_temper(mt[w]) >> sh);
            w += 1;
            if (r < width) { got = true; break; }
        }
        if (!got) break;          // its bit-rate draws run past the state's end
        if (lane == n) { my_off = off; my_r = r; }
        off = w;
    }
    double u[4];
    if (n == 0) {
        // the straddler: word by word through the regeneration, every lane the same values
        uint32_t wq[8];
        int r = 0;
        for (int k = 0;; ++k) {
            if (off >= ORLG_MT_N) { mt_regenerate(mt, lane); off = 0; }
            const uint32_t y = mt_temper(mt[off]);
            off += 1;
            if (k < 8) { wq[k] = y; continue; }
            r = (int)(y >> sh);
            if (r < width) break;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = mt_random(wq[2 * q], wq[2 * q + 1]);
        my_r = r;
        n = 1;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t a = lane < n ? mt_temper(mt[my_off + 2 * q]) : 0u, b = lane < n ? mt_temper(mt[my_off + 2 * q + 1]) : 0u;
            u[q] = mt_random(a, b);
        }
    }
    idx = off;
    double iat, ht;
    request_times(u[0], u[1], lam_arrival, lam_holding, iat, ht);
    int src = 0, dst = 0;
    {
        const double x = u[2] * (src_cum[N - 1] + 0.0);
        for (int i = 0; i < N - 1; ++i) src += src_cum[i] <= x ? 1 : 0;
    }
    {
        orlg_lds_cf64 *row = dst_cum + src * N;
        const double x = u[3] * (row[N - 1] + 0.0);
        for (int i = 0; i < N - 1; ++i) dst += row[i] <= x ? 1 : 0;
    }
    const double o_iat = lane < n ? iat : 0.0, o_ht = lane < n ? ht : 0.0;
    const uint32_t o_rq = lane < n ? ((uint32_t)src | ((uint32_t)dst << 8) | ((uint32_t)my_r << 16)) : 0u;
    ring_store<RING_LDS>(ring_iat_v, ring_ht_v, ring_req_v, lane, o_iat, o_ht, o_rq);
    return n | (idx << 8);
}
template <bool RING_LDS>
DEV int refill_requests_cont(uint32_t *mt, double *ring_iat, double *ring_ht, uint32_t *ring_req, const double *src_cum,
                             const double *dst_cum, int *idx_io, int N, int width, double lam_arrival, double lam_holding) {
    const int r = refill_requests_cont_as<RING_LDS>((orlg_lds_u32 *)mt, ring_iat, ring_ht, ring_req, (orlg_lds_cf64 *)src_cum,
                                                    (orlg_lds_cf64 *)dst_cum, *idx_io, N, width, lam_arrival, lam_holding);
    *idx_io = r >> 8;
    return r & 0xff;
}

// A request trace as the ring's third producer (include/orlg.h orlg_create_trace): lane j copies request cursor + j of the
// environment from the device trace into ring slot j -- three coalesced loads, no MT19937 state, no logarithm.  The ring's first
// array then holds ABSOLUTE arrival times (the step takes them as they are: a recorded time comes back with its own bits).
// cursor = requests of the environment copied so far (kept where a generated handle keeps the MT19937 position).  The first
// refill keeps the stagger of refill_requests_as.  A cursor outside the trace copies nothing (the host refuses a launch that
// would draw past the end; a state from elsewhere must not make the loads leave the arrays).  Returns the count.
template <bool RING_LDS>
__device__ __noinline__ int refill_requests_trace_as(orlg_glb_cf64 *tr_arrival, orlg_glb_cf64 *tr_holding, orlg_glb_cu32 *tr_req,
                                                     void *ring_iat_v, void *ring_ht_v, void *ring_req_v, int cursor, int length,
                                                     int env) {
    const int lane = threadIdx.x & 63;
    int n = length - cursor;
    n = n > ORLG_RING ? ORLG_RING : n;
    if (cursor == 0) { const int cap = 62 - env % 56; n = n > cap ? cap : n; }
    if (cursor < 0 || n < 0) n = 0;
    const size_t at = (size_t)env * (size_t)length + (size_t)(cursor > 0 ? cursor : 0) + (size_t)lane;
    double o_at = 0.0, o_ht = 0.0;
    uint32_t o_rq = 0u;
    if (lane < n) { o_at = tr_arrival[at]; o_ht = tr_holding[at]; o_rq = tr_req[at]; }
    ring_store<RING_LDS>(ring_iat_v, ring_ht_v, ring_req_v, lane, o_at, o_ht, o_rq);
    return n;
}
// the callers' form: generic pointers in, the cursor advanced through cursor_io
template <bool RING_LDS>
DEV int refill_requests_trace(const double *tr_arrival, const double *tr_holding, const uint32_t *tr_req, double *ring_iat,
                              double *ring_ht, uint32_t *ring_req, int *cursor_io, int length, int env) {
    const int n = refill_requests_trace_as<RING_LDS>((orlg_glb_cf64 *)tr_arrival, (orlg_glb_cf64 *)tr_holding, (orlg_glb_cu32 *)tr_req,
                                                     ring_iat, ring_ht, ring_req, *cursor_io, length, env);
    *cursor_io += n;
    return n;
}
