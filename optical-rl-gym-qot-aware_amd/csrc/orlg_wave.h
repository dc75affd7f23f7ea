// orlg_wave.h -- the device library every kernel of the project stands on: what a wavefront (gfx950, wave64) does with its own
// lanes and registers.  Nothing here knows a data layout.
//
// The names (u64, DEV, ORLG_INF_BITS, ORLG_GPTR); the wave helpers (wave_sync, uni, readlane64, readlane_d, ballot, ctz64, clz64,
// popc64); the two slot-bit masks (valid_mask, window_mask); the fp64 division as the hardware expands it, with the
// denominator-only part hoisted (recip_refine, div_by); the DPP lane moves (dpp_*, lane_*), the reductions over a link's 8-lane
// group (group8_*) and over the whole wave (wave_*_i32, wave_*_f64).  Users: the three step kernels, the query and mask kernels,
// the OSNR kernel (orlg_osnr.hip), the arrival producers (orlg_requests.h) and the helper kernels of the two host APIs.
//
// Reference: the arithmetic these reproduce is cited where it is used; here only the slot range of a link's bitmap
// (rmsa_env.py:721-734: slots [s, s + n) of num_spectrum_resources).
#pragma once
#include <hip/hip_runtime.h>

#include "orlg_device.h"
#include "orlg_math.h"

typedef uint64_t u64;

#define DEV __device__ __forceinline__
#define ORLG_INF_BITS 0x7ff0000000000000ull

// Per-step output arrays: their addresses are kept in LDS (Tab::outs), and a pointer read from memory is a generic pointer --
// every store through it would be a flat instruction, which waits on both memory counters.  They are global memory.
typedef int orlg_v4i __attribute__((ext_vector_type(4)));
#define ORLG_GPTR(T, v) ((T __attribute__((address_space(1))) *)(v))   // an output array: global memory, not a generic pointer
// ---------------------------------------------------------------------------------------- wave helpers
DEV void wave_sync() {
    // LDS hand-off between lanes of ONE wave: hardware executes a wave's LDS operations in order, the
    // fences only stop the compiler from caching or reordering across the hand-off.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// An explicit `s_waitcnt vmcnt(0)` (gfx9 encoding: expcnt and lgkmcnt left at their maxima): the wave waits here for its
// outstanding loads, stores and atomics without return -- one in-order counter.  It orders nothing and nothing depends on it;
// it is a statement about WHERE the wave waits.  The compiler's wait-count pass reads the builtin (inline assembly it does not
// read) and then knows the counter is zero on the paths that pass here, so it places no wait of its own for them further on.
DEV void vm_drain() { __builtin_amdgcn_s_waitcnt(0x0F70); }
DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
DEV u64 readlane64(u64 v, int l) {
    uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}
DEV double readlane_d(double v, int l) { return __longlong_as_double((long long)readlane64((u64)__double_as_longlong(v), l)); }
DEV u64 ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
DEV int ctz64(u64 v) { return __builtin_ctzll(v); }
DEV int clz64(u64 v) { return __builtin_clzll(v); }
DEV int popc64(u64 v) { return __builtin_popcountll(v); }

// valid slot bits of word w of a link's bitmap (slots >= S do not exist and are stored as 0 = not free)
DEV u64 valid_mask(int S, int w) {
    int nv = S - 64 * w;
    return nv >= 64 ? ~0ull : (nv <= 0 ? 0ull : ((1ull << nv) - 1ull));
}

// bits of the slot window [s, s+n) that fall in word w
DEV u64 window_mask(int s, int n, int w) {
    int lo = s - 64 * w, hi = s + n - 64 * w;
    lo = lo < 0 ? 0 : lo;
    hi = hi > 64 ? 64 : hi;
    if (hi <= lo) return 0ull;
    int len = hi - lo;
    u64 m = len >= 64 ? ~0ull : ((1ull << len) - 1ull);
    return m << lo;
}

// ---------------------------------------------------------------------------------------- fp64 division
// x / b for several numerators over ONE denominator.  This is the gfx9 fdiv-f64 expansion itself
// (v_rcp_f64, two Newton steps, quotient, residual, final fma) with the denominator-only part hoisted;
// v_div_scale / v_div_fixup are identities for the operand ranges here (simulation clock in
// (0, 1e12), numerators below 1e18), so every quotient is the correctly rounded IEEE quotient the
// reference computes.  Checked bit for bit against the oracle in tests/test_gpu_rmsa.py.
DEV double recip_refine(double b) {
    double y = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-b, y, 1.0);
    return __builtin_fma(y, e, y);
}
DEV double div_by(double a, double b, double y) {
    double q = a * y;
    double r = __builtin_fma(-b, q, a);
    return __builtin_fma(r, y, q);
}

// ---------------------------------------------------------------------------------------- DPP moves and reductions
// reductions over the 8 lanes of a link group (lane = link slot * 8 + word) with DPP lane permutations: xor 1 and xor 2
// inside a quad, then the mirrored half row brings in the other quad's total -- every lane ends with the group's result
DEV int dpp_xor1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false); }   // quad_perm [1,0,3,2]
DEV int dpp_xor2(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false); }   // quad_perm [2,3,0,1]
DEV int dpp_half_mirror(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false); }
// neighbours inside a row of 16 lanes: the previous lane (row_shr:1), the next lane (row_shl:1), K lanes ahead (row_shl:K);
// 0 where the row ends
DEV int lane_prev_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true); }
DEV int lane_next_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x101, 0xf, 0xf, true); }
template <int K>
DEV int lane_ahead_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x100 + K, 0xf, 0xf, true); }
template <int K>
DEV int lane_back_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x110 + K, 0xf, 0xf, true); }   // K lanes back (row_shr:K)
DEV u64 lane_prev_u64(u64 v) {
    const uint32_t lo = (uint32_t)lane_prev_i32((int)(uint32_t)v), hi = (uint32_t)lane_prev_i32((int)(uint32_t)(v >> 32));
    return ((u64)hi << 32) | lo;
}
DEV int group8_add(int v) { v += dpp_xor1(v); v += dpp_xor2(v); v += dpp_half_mirror(v); return v; }
DEV int group8_min(int v) {
    int o = dpp_xor1(v); v = o < v ? o : v;
    o = dpp_xor2(v); v = o < v ? o : v;
    o = dpp_half_mirror(v); return o < v ? o : v;
}
DEV int group8_max(int v) {
    int o = dpp_xor1(v); v = o > v ? o : v;
    o = dpp_xor2(v); v = o > v ? o : v;
    o = dpp_half_mirror(v); return o > v ? o : v;
}

// whole-wave reductions without LDS crossbar round trips: full-mask DPP permutations inside a row of 16 lanes (quad, half row,
// row: every lane of a row ends with the row's result), then the four row results are read with v_readlane and combined as
// wave-uniform values.  (The row-broadcast DPP modes with a partial row mask are avoided on purpose: whether the masked-off
// lanes keep the right value depends on how the compiler folds the move into the ALU op.)
DEV int dpp_row_mirror(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false); }
DEV int wave_max_i32(int v) {
    int o = dpp_xor1(v); v = o > v ? o : v;
    o = dpp_xor2(v); v = o > v ? o : v;
    o = dpp_half_mirror(v); v = o > v ? o : v;
    o = dpp_row_mirror(v); v = o > v ? o : v;
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    const int a = r0 > r1 ? r0 : r1, b = r2 > r3 ? r2 : r3;
    return a > b ? a : b;
}
DEV int wave_add_i32(int v) {
    v += dpp_xor1(v); v += dpp_xor2(v); v += dpp_half_mirror(v); v += dpp_row_mirror(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}
#define ORLG_DPP_F64(fn, x) __hiloint2double(fn(__double2hiint(x)), fn(__double2loint(x)))
DEV double wave_max_f64(double v) {
    double o = ORLG_DPP_F64(dpp_xor1, v); v = o > v ? o : v;
    o = ORLG_DPP_F64(dpp_xor2, v); v = o > v ? o : v;
    o = ORLG_DPP_F64(dpp_half_mirror, v); v = o > v ? o : v;
    o = ORLG_DPP_F64(dpp_row_mirror, v); v = o > v ? o : v;
    const double r0 = readlane_d(v, 0), r1 = readlane_d(v, 16), r2 = readlane_d(v, 32), r3 = readlane_d(v, 48);
    const double a = r0 > r1 ? r0 : r1, b = r2 > r3 ? r2 : r3;
    return a > b ? a : b;
}
DEV double wave_add_f64(double v) {   // the association order differs from a sequential sum: only for tolerance-based results
    v += ORLG_DPP_F64(dpp_xor1, v); v += ORLG_DPP_F64(dpp_xor2, v);
    v += ORLG_DPP_F64(dpp_half_mirror, v); v += ORLG_DPP_F64(dpp_row_mirror, v);
    return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}

DEV int wave_min_i32(int v) {
    int o = dpp_xor1(v); v = o < v ? o : v;
    o = dpp_xor2(v); v = o < v ? o : v;
    o = dpp_half_mirror(v); v = o < v ? o : v;
    o = dpp_row_mirror(v); v = o < v ? o : v;
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    const int a = r0 < r1 ? r0 : r1, b = r2 < r3 ? r2 : r3;
    return a < b ? a : b;
}
