// orlg_graph_log.h -- the graph statistics of the group kernel's lean body, logged per accepted provision and worked off in batches.
//
// _update_network_stats (rmsa_env.py:537-560) runs once per accepted provision:
//     comp = _get_network_compactness();  if now > 0: g_x = (g_x * g_lu + cur_x * (now - g_lu)) / now  for x = throughput, compactness;  g_lu = now
// Nothing of a launch without per-step outputs reads the three doubles before the state leaves, and of the work only
// g <- (g * g_lu + c) / now is a chain: the compactness (two float64 divisions), the reciprocal of `now`, the time difference and the
// two products c = cur * time_diff depend on the entry and its predecessor's time alone.  The lean body therefore LOGS what the
// update consumes -- the time, the running bit-rate sum and the three integer sums behind the compactness: OrlgGraphEntry, five
// registers -- with entry k of a row's environment on lane k of the row, and group_graph_replay (orlg_group_kernels.hip) works a
// row's log off: orlg_glog_eval once on every lane (lane = entry), then orlg_glog_chain entry by entry.
//
// The arithmetic is group_link_stats' GRAPH tail, operation for operation and in its order per environment, written once here
// for the device and the host (tests/graph_log_check.cc feeds random logs at the field limits through the packing and the batched
// evaluation and through a plain sequential restatement).  On the host the division is IEEE's, of which the device's expansion
// is the correctly rounded equal (orlg_math.h, orlg_wave.h).  Compile with FP contraction off.
#pragma once
#if defined(__HIPCC__)
#include "orlg_wave.h"   // recip_refine, div_by: the device's division (a host compiler reads orlg_math.h alone)
#endif
#include "orlg_math.h"

#define ORLG_GLOG_FN ORLG_HD __attribute__((always_inline))
#define ORLG_GLOG_CAP 16                     // entries per environment between two replays: one per lane of its row
// what the packed fields hold -- the library's limits: E <= 255 links (a link is a byte of a path record) of S <= 512
// slots (8 words), a release queue of at most 4 096 services (orlg_create) of an int32 bit rate each
#define ORLG_GLOG_MAX_ES (255 * 512)           // sum_span, sum_slots_hops <= E S; sum_gaps <= E S / 2
#define ORLG_GLOG_MAX_Q 4096
#define ORLG_GLOG_SUM_BITS 17
#define ORLG_GLOG_BR_BITS 45
static_assert(ORLG_GLOG_MAX_ES < (1 << ORLG_GLOG_SUM_BITS), "an E S sum must fit its field");
static_assert((long long)ORLG_GLOG_MAX_Q * 0x7fffffffLL < (1LL << ORLG_GLOG_BR_BITS), "the bit rates of a full queue must fit their field");
static_assert(3 * ORLG_GLOG_SUM_BITS + ORLG_GLOG_BR_BITS == 96, "three registers");

// one logged update: the simulation time of the provision and, in three words, sum_span (17 bits) | sum_slots_hops (17) |
// sum_gaps (17) | sum_bitrate_running (45), all as they stand after the provision's statistics pass
struct OrlgGraphEntry {
    double now;
    uint32_t w0, w1, w2;
};

ORLG_GLOG_FN void orlg_glog_pack(OrlgGraphEntry &e, double now, long long sum_bitrate_running, int sum_span, int sum_sh, int sum_gaps) {
    const uint64_t br = (uint64_t)sum_bitrate_running;
    e.now = now;
    e.w0 = (uint32_t)sum_span | ((uint32_t)sum_sh << 17);                                      // (the low 15 bits of sum_sh)
    e.w1 = ((uint32_t)sum_sh >> 15) | ((uint32_t)sum_gaps << 2) | ((uint32_t)(br >> 32) << 19);  // (its high 2; the high 13 of the rate)
    e.w2 = (uint32_t)br;
}

// the parallel part of one update: what the chain consumes
struct OrlgGraphTerm {
    double now, ynow;       // the time and (device) its refined reciprocal; the update does nothing but g_lu = now unless now > 0
    double c_thr, c_comp;   // cur * time_diff of the throughput and of the compactness
};

// entry `e`, whose predecessor's time (g_last_update for a log's first entry) is `prev`: _get_network_compactness (rmsa_env.py:844-851),
// time_diff and the two products
ORLG_GLOG_FN OrlgGraphTerm orlg_glog_eval(const OrlgGraphEntry &e, double prev, int E) {
    const int sum_span = (int)(e.w0 & 0x1ffffu), sum_sh = (int)((e.w0 >> 17) | ((e.w1 & 3u) << 15)), sum_gaps = (int)((e.w1 >> 2) & 0x1ffffu);
    const long long br = (long long)(((uint64_t)(e.w1 >> 19) << 32) | e.w2);
    OrlgGraphTerm t;
    t.now = e.now;
    t.ynow = 0.0;
    t.c_thr = 0.0;
    t.c_comp = 0.0;
    double comp = 1.0;
    if (sum_gaps > 0) comp = ORLG_FDIV((double)sum_span, (double)sum_sh) * ORLG_FDIV((double)E, (double)sum_gaps);
    if (e.now > 0) {
#if defined(__HIP_DEVICE_COMPILE__)
        t.ynow = recip_refine(e.now);
#endif
        const double time_diff = e.now - prev;
        t.c_thr = (double)br * time_diff;
        t.c_comp = comp * time_diff;
    }
    return t;
}

// one link of the chain: g <- (g * g_lu + c) / now, where g_lu is the predecessor's time
ORLG_GLOG_FN double orlg_glog_chain(double g, double g_lu, double c, double now, double ynow) {
    const double num = (g * g_lu) + c;
#if defined(__HIP_DEVICE_COMPILE__)
    return div_by(num, now, ynow);
#else
    (void)ynow;
    return num / now;
#endif
}
