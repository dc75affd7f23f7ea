// orlg_device.h -- device-side data layout shared by the kernels (through orlg_wave.h) and the host API
// (orlg_host.h, the RMSA API's units orlg_api*.hip behind orlg_rmsa_host.h).  Names follow the reference's domain: links, slots, paths, services, release queue.
#pragma once
#include <hip/hip_vector_types.h>   // uint4
#include <stdint.h>

#define ORLG_WAVE 64
#define ORLG_MAX_WAVES_PER_BLOCK 8
#define ORLG_MT_N 624
#define ORLG_MT_M 397
#define ORLG_MAX_W 8          // 64-bit words per link: S <= 512
#define ORLG_MAX_HOPS 14
#define ORLG_NSLOT_STRIDE 8   // nslots table: [bit-rate index][spectral efficiency 0..7]
#define ORLG_NUM_OUTS 12
#define ORLG_RING 64           // arrivals generated per refill (one per lane)
#ifndef ORLG_GROUP_WAVES
#define ORLG_GROUP_WAVES 12    // four-environments-per-wave kernel: waves per workgroup at most (LDS decides how many fit): up to 3 per SIMD
#endif
#define ORLG_DIRECT_STEPS 4    // launches of at most this many steps read their ring entries straight from HBM
#define ORLG_LLOG_CAP 64      // logged updates per (environment, link) between two replays (6-bit count): sizes OrlgParams::llog

// One k-shortest-path record (16 B): Path.hops, Path.best_modulation.spectral_efficiency and the link
// "index" of every hop (utils.py:27-36, rmsa_env.py:479-483).
// Padding: link[h] for h >= hops repeats link[0] (orlg_path_records, orlg_host.hip, fills it so).  A byte past the path's end
// thus names a link of the path itself, and a reader that ANDs the occupancy words of all ORLG_MAX_HOPS bytes gets the path's
// word (group_path_word_rec, orlg_group_kernels.hip).  Every other reader stops at `hops` and must not depend on the padding.
struct __attribute__((aligned(16))) OrlgPathRec {
    uint8_t hops, se;
    uint8_t link[ORLG_MAX_HOPS];
};

// Per-environment scalars kept in HBM between launches (one record per env, 192 B).
struct __attribute__((aligned(16))) OrlgEnvScalars {
    double current_time;                                   // optical_network_env.py:33
    double req_arrival, req_holding;                       // current_service.arrival_time / holding_time
    double g_throughput, g_compactness, g_last_update;     // topology.graph[...] rmsa_env.py:537-560
    int64_t c[8];                                          // orlg_counters order
    int64_t sum_bitrate_running;                           // sum of bit_rate over running services
    int64_t episodes_done;
    int32_t sum_slots_hops;                                // sum of number_slots * hops over running services
    int32_t n_running;
    int32_t req_src, req_dst, req_br, req_sid;             // pending request (br = bit-rate INDEX)
    int32_t mt_idx;                                        // MT19937 position (0..624)
    int32_t new_service;                                   // self._new_service
    int32_t q_overflow;                                    // release queue overflowed (error)
    int32_t ring_pos, ring_cnt;                            // pre-generated arrivals: next entry, entries left
    int32_t sum_span, sum_gaps;                            // sums over the per-link (span, gaps) cache (_get_network_compactness)
    int32_t q_head;                                        // release queue: slot of the earliest entry (time-sorted ring, see OrlgParams::qtime)
};
static_assert(sizeof(OrlgEnvScalars) == 192, "OrlgEnvScalars layout");

// Wave scalars that live in LDS during a launch (rarely touched counters; lane 0 updates them).
struct OrlgWaveScalars {
    int64_t c[8];
    int64_t sum_bitrate_running;
    int64_t episodes_done;
    double g_thr, g_comp, g_lu;        // topology.graph["throughput" | "compactness" | "last_update"]
    double req_arrival, req_holding;   // pending request times
    int32_t n_running, q_overflow;
};
static_assert(sizeof(OrlgWaveScalars) == 128, "OrlgWaveScalars layout");

// the arrival process of one environment of a handle with per-environment traffic (include/orlg.h orlg_traffic)
struct __attribute__((aligned(16))) OrlgRates {
    double arrival_lambda, holding_lambda;
};

enum { ORLG_MODE_STEP = 0, ORLG_MODE_INIT = 1, ORLG_MODE_EPISODE_RESET = 2 };
// device-side policy ids (== include/orlg.h ORLG_POLICY_*)
enum { ORLG_POLICY_EXT = -1, ORLG_POLICY_SP = 0, ORLG_POLICY_SAP = 1, ORLG_POLICY_LLP = 2, ORLG_POLICY_DEEP_SP = 3,
       ORLG_POLICY_DEEP_SAP = 4, ORLG_POLICY_DEEP_EXT = 5, ORLG_POLICY_PATH_EXT = 6, ORLG_POLICY_SAP_GN = 7 };
// device-side only (orlg_step_min_cut, orlg_cut.h; no public policy or rule has these values): the route "fewest cuts" -- of all k
// paths the one whose MIN_CUT window has the fewest cuts (include/orlg.h ORLG_ROUTE_FEWEST_CUTS is mapped to it) -- and the rule
// MIN_CUT as a value of OrlgParams::assign, behind the public ORLG_ASSIGN_* (ORLG_NUM_ASSIGN_RULES stays what it is)
enum { ORLG_POLICY_MIN_CUT = 8 };
enum { ORLG_ASSIGN_MIN_CUT = 5 };
// device-side only (orlg_step_window, orlg_usage.h): the route "best window" -- of all k paths the one whose rule window ranks best
// by the rule's own order (include/orlg.h ORLG_ROUTE_BEST_WINDOW is mapped to it) -- and the rule MOST_USED as a value of
// OrlgParams::assign (include/orlg.h ORLG_RULE_MOST_USED is mapped to it); a launch with either runs the USAGE instantiations
enum { ORLG_POLICY_BEST_WINDOW = 9 };
enum { ORLG_ASSIGN_MOST_USED = 6 };
// LDS an environment's prefix sums of the slot usage take in such a launch: 64 W int32 (orlg_usage.h usage_prefix)
#define ORLG_USAGE_BYTES(W) (256 * (W))
// per-step output slots (OrlgParams::outs)
enum { ORLG_OUT_PATH = 0, ORLG_OUT_SLOT, ORLG_OUT_ACCEPTED, ORLG_OUT_DONE, ORLG_OUT_REWARD, ORLG_OUT_REQUEST,
       ORLG_OUT_ARRIVAL, ORLG_OUT_HOLDING, ORLG_OUT_COMPACT, ORLG_OUT_COMPACT_DIFF, ORLG_OUT_AVG_LINK_COMPACT,
       ORLG_OUT_AVG_LINK_UTIL };

// Kernel parameters (passed by value).
struct OrlgParams {
    // sizes
    int32_t B, N, E, S, K, NBR, Q, NW;       // NW = E*W words of occupancy per env
    int32_t episode_length, n_steps, policy, auto_reset, mode, reward_mode, stats_level, j;
    int32_t obs_dim, out_mask;               // out_mask: bit i set <=> outs[i] != nullptr
    double arrival_lambda, holding_lambda;
    // per-env state in HBM
    uint64_t *occ;            // [B][NW]   free-slot bitmap, word (link*W + w)
    // release queue (the reference's heapq of (release time, service), optical_network_env.py:178-189): a time-sorted ring.  The
    // n_running entries sit at slots (q_head + rank) % Q in ascending release time; every other slot holds (+inf, 0).  A
    // release pops the head, an insert moves the later entries up by one slot.
    double *qtime;            // [B][Q]    release time, +inf = empty slot
    uint32_t *qdesc;          // [B][Q]    path gid | start << 14 | bit-rate index << 24
    uint32_t *mt;             // [B][624]
    OrlgEnvScalars *scal;     // [B]
    int32_t *hist;            // [B][4][NBR] requested, provisioned, episode requested, episode provisioned
    double *lstat;            // [B][4][E] utilization, external_fragmentation, compactness, last_update
    int32_t *lint;            // [B][lint_stride] per-link span | gaps << 16 (the cache behind _get_network_compactness)
    int32_t lint_stride;
    int32_t obs_f32;          // orlg_deeprmsa_obs_kernel writes float32 (o_obs then points to floats)
    uint4 *llog;              // [B][E][ORLG_LLOG_CAP] logged link-statistics updates (orlg_rmsa_group_kernel<.., DEFER>), scratch
    int32_t br_width;         // bit_rate_selection="continuous": number of bit rates lower .. higher (the table bit_rates holds them), 0 = discrete
    int32_t g_lean;           // orlg_rmsa_group_kernel<.., DEFER>: this launch takes the lean body (launch_rmsa_group decides)
    double *ring_iat, *ring_ht;   // [B][64] pre-generated inter-arrival / holding times (in RNG stream order)
    uint32_t *ring_req;           // [B][64] src | dst << 8 | bit-rate index << 16
    // read-only tables: ONE blob in HBM that every workgroup stages into LDS (byte offsets t_*, 16-B aligned)
    const unsigned char *tables;
    int32_t tab_bytes;
    int32_t t_pair;           // int32  [N*N]        first path record of pair (src, dst)
    int32_t t_recs;           // PathRec[num_paths]
    int32_t t_nslots;         // uint16 [NBR][8]     get_number_slots per (bit rate, spectral efficiency)
    int32_t t_bitrates;       // int32  [NBR]
    int32_t t_brcum;          // double [NBR]
    int32_t t_srccum;         // double [N]
    int32_t t_dstcum;         // double [N*N]
    int32_t t_divs;           // double [S+1]        k / S   (link utilization: exact IEEE quotients, built on the host)
    int32_t t_inv;            // double [S/2+2]      1 / k   (link compactness)
    // per-call IO
    const int32_t *actions;
    void *outs[ORLG_NUM_OUTS];
    double *o_obs;
    int32_t *err_flag;        // the handle's sticky error word (mapped host memory): 1 = a release queue overflowed
    // work queue: every wave draws environments from *ticket until the launch's B are taken (ticket - ticket_base
    // is the environment index; the host advances ticket_base by B + launched waves per launch, no memset needed)
    uint32_t *ticket;
    uint32_t ticket_base;
    uint32_t ticket_stride;   // 1: static striding (env = wave, wave + waves, ...) instead of tickets: short launches
    // long launches of the four-environments-per-wave kernel, tickets in CHUNKS of steps (n_chunks > 1): ticket t = chunk t / quads
    // of quad t % quads -- a quad's launch is cut into n_chunks pieces that different waves may run, so the last round of
    // tickets is short; progress[quad] = chunks of the quad completed in this launch (the hand-off between the waves)
    int32_t n_chunks, chunk_steps;
    uint32_t *progress;
    // per-wave LDS layout (byte offsets from the wave's base) and size
    int32_t l_occ, l_qtime, l_qdesc, l_mt, l_lstat, l_hist, l_lint, l_scratch, l_wsc, l_ring, l_wave_bytes;
    int32_t l_shared_bytes;   // tables + output pointer block, in front of the per-wave regions
    int32_t l_outs;           // byte offset of the staged outs[] array
    // four-environments-per-wave kernel (orlg_group_kernels.hip): byte offsets inside one environment's LDS region, the region's
    // size (a wave's region = 4 environments), and g_mt = size of the workgroup's MT19937 staging buffer, which sits with its
    // lock word between the tables and the waves' regions
    int32_t g_occ, g_qtime, g_qdesc, g_lstat, g_hist, g_lint, g_env_bytes, g_mt, g_wave_bytes;
    // per-environment traffic (orlg_create_traffic): [B] pairs (arrival_lambda, holding_lambda) that take the place of the two
    // scalars above, nullptr = every environment has the scalars.  Read where a refill needs it (orlg_env_rates), never kept
    const OrlgRates *rates;
    // request trace (orlg_create_trace): [B][tr_len] each, 20 bytes per request -- absolute arrival time, holding time,
    // src | dst << 8 | bit-rate index << 16 (the ring's own layout); nullptr = the environments generate their traffic.  A trace
    // handle has no generator: OrlgEnvScalars::mt_idx is the index of the next request a refill copies into the ring, and the
    // ring's first array holds absolute arrival times (refill_requests_trace_as)
    const double *tr_arrival, *tr_holding;
    const uint32_t *tr_req;
    int32_t tr_len;
    // the gate chooses the modulation from the GSNR (orlg_set_gn_modulation): M = the gate's num_thresholds, 0 = every
    // service runs at its path's own spectral efficiency.  Set: the descriptors of qdesc carry a level (orlg_qdesc.h).  (It took the
    // place of a padding word: every other field lies in the kernarg segment where it lay)
    int32_t gn_adaptive;
    // GN-model admission check of the wave-per-environment kernel (orlg_set_gn_gate, orlg_rmsa_gn.h): the gate's table in HBM
    // (ORLG_GN_* below), nullptr = no gate; o_gsnr: the per-step output gn_gsnr_db [n_steps][B] of orlg_step_gn, nullptr = not asked for
    const double *gn;
    double *o_gsnr;
    // blocking cause (include/orlg.h orlg_step_diag; orlg_block_cause.h), written by the CAUSE instantiations of the two step kernels
    // only: o_cause [n_steps][B] ORLG_CAUSE_* per step, o_cause_counts [B][8] steps of this launch per cause (zeroed on the stream
    // before the launch); nullptr = not asked for.  A launch that asks for either has ORLG_OUT_CAUSE_BIT in out_mask.  (At the
    // struct's end: every other field lies in the kernarg segment where it lay)
    uint8_t *o_cause;
    int32_t *o_cause_counts;
    // spectrum-assignment rule (include/orlg.h ORLG_ASSIGN_*, orlg_step_assign; orlg_assign.h), read by the ASSIGN instantiations of
    // the two step kernels only: `policy` is then the route.  0 = the reference's first fit; a launch with another rule has
    // ORLG_OUT_ASSIGN_BIT in out_mask; ORLG_ASSIGN_MIN_CUT (above): the fewest-cuts window, orlg_cut.h, the CUT instantiations.
    // (At the struct's end, as the cause pointers)
    int32_t assign;
    // the neighbour margin of a protecting handle (orlg_set_gn_protect, orlg_rmsa_gn_protect.h): the per-step output
    // gn_neighbour_margin_db [n_steps][B] of orlg_step_gn_protect, written by the PROTECT instantiations only; nullptr = not asked
    // for.  (At the struct's end, as the fields above)
    double *o_margin;
};
// what a launch of orlg_rmsa_mm_kernel (orlg_step_max_margin, orlg_gn_max_margin.h) gets beside OrlgParams -- a kernel argument of its
// own: OrlgParams, and with it the kernarg segment of every other kernel, stays what it is
struct OrlgMmArgs {
    double *o_window_margin;   // [n_steps][B] the w of the proposed window, NaN for a fallback or a rejection; nullptr = not asked for
    int32_t protect;           // the handle protects its running lightpaths (wave-uniform)
    int32_t pad;
};
// device-side only (orlg_step_modulation, orlg_rmsa_gn_am.h; the AM instantiations alone read them): the policies that walk the levels
// of a path -- path 0 / the paths in order / the agent's path -- and the agent's (path, slot, level)
enum { ORLG_POLICY_SP_AM = 10, ORLG_POLICY_SAP_AM = 11, ORLG_POLICY_PATH_AM_EXT = 12, ORLG_POLICY_EXT_AM = 13 };
// what a launch of orlg_rmsa_am_kernel gets beside OrlgParams -- a kernel argument of its own, as OrlgMmArgs
struct OrlgAmArgs {
    uint8_t *o_se;   // [n_steps][B] gn_se: the level of the candidate the step shows, 0 = no check ran; nullptr = not asked for
};
// out_mask of a launch that asks for a cause output: not one of outs[], but a per-step output like them -- what looks at
// out_mask to choose a kernel (the deferred link statistics, the group kernel's HBMQ kind and lean body) keeps such a launch on
// the plain instantiations, the only ones that exist with the classifier
enum { ORLG_OUT_CAUSE_BIT = 1 << 30 };
// out_mask of a launch under an assignment rule other than the reference's first fit (OrlgParams::assign): no output at all, the
// same device -- the ASSIGN instantiations exist of the plain kind only, and what looks at out_mask keeps the launch on them
enum { ORLG_OUT_ASSIGN_BIT = 1 << 29, ORLG_OUT_PLAIN_BITS = ORLG_OUT_CAUSE_BIT | ORLG_OUT_ASSIGN_BIT };
// OrlgParams::gn, in doubles: the gate's scalars, the thresholds by spectral efficiency - 1 from ORLG_GN_THR0, then four per link
// from ORLG_GN_LINK0 -- effective length of a span, its ratio to the span's length, exp(2 att len) - 1, number of spans
enum { ORLG_GN_DENSITY = 0, ORLG_GN_F0, ORLG_GN_SLOT, ORLG_GN_ATT, ORLG_GN_NF, ORLG_GN_LEFF_A, ORLG_GN_THR0 = 8, ORLG_GN_LINK0 = 16 };

// A kernel's parameter struct T in the kernarg segment: fields are fetched through the scalar cache where they are used
template <typename T>
__device__ __forceinline__ const T __attribute__((address_space(4))) *kernarg_as() {
    return (const T __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
}
