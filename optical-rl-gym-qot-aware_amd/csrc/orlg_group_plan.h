// orlg_group_plan.h -- what the host decides about a launch of the four-environments-per-wave step kernel (orlg_group_kernels.hip):
// the LDS layout of a wave's region for each of the kernel's three kinds of instantiation, and from them the kind, the workgroup, the
// grid and the tickets of one launch.  Arithmetic only -- no HIP call, no environment variable, no handle -- so all of it runs
// without a device (orlg_debug_group_plan); rmsa_create (orlg_api.hip) and launch_rmsa_group (orlg_api_step.hip) do what it says.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/orlg.h"   // ORLG_STATS_FULL
#include "orlg_device.h"
#include "orlg_lds.h"

// the plain instantiation, the one that leaves the release queue in HBM, the one that defers the link statistics
enum OrlgGroupKind { ORLG_GROUP_PLAIN, ORLG_GROUP_HBMQ, ORLG_GROUP_DEFER };
// A wave's LDS region = four environments' regions (no MT19937 state, no arrival ring, scalars in registers).
// A wave's region is array-major: the four environments' occupancy bitmaps behind each other, then their link statistics,
// span caches, release times, descriptors -- exactly as four consecutive environments lie in the HBM arrays, so a quad's
// occupancy / statistics / span cache move as ONE linear copy by all 64 lanes (uniform base + lane offset); occ .. qdesc = offset of
// the array in the wave's region, row g's slice starts g * (slice bytes) further.  DEFER: lstat = where the links' summaries go (8
// bytes per link, group_release_links).  wpb_max: the most waves per workgroup the LDS holds (0: none fit); shared_bytes: the
// tables and the output pointer block, in front of the waves' regions
struct OrlgGroupLayout { int occ, lstat, lint, qtime, qdesc, wave_bytes, wpb_max, shared_bytes; };
// the workgroup's MT19937 staging buffer (then its lock word), in front of the waves' regions
enum { ORLG_GROUP_MT_BYTES = (ORLG_MT_N * 4 + 15) & ~15 };
static inline size_t orlg_group_lds(size_t shared_bytes, int wpb, int wave_bytes) { return shared_bytes + ORLG_GROUP_MT_BYTES + 16 + (size_t)wpb * wave_bytes; }
static inline OrlgGroupLayout orlg_group_layout(OrlgGroupKind kind, int NW, int E, int Q, int lint_stride, int stats_level, int shared_bytes) {
    auto up16 = [](int v) { return (v + 15) & ~15; };
    OrlgGroupLayout l = {};
    int go = up16(4 * NW * 8);
    // the instantiation that defers the link statistics keeps them in HBM: the same arrays without their slices
    l.lstat = go; if (kind != ORLG_GROUP_DEFER && stats_level >= ORLG_STATS_FULL) go = up16(go + 4 * 4 * E * 8);
    l.lint = go; go = up16(go + 4 * lint_stride * 4);
    l.qtime = go; go = up16(go + 4 * Q * 8);
    l.qdesc = go; go = up16(go + 4 * Q * 4);
    if (kind == ORLG_GROUP_DEFER) { l.lstat = go; go = up16(go + 4 * E * 8); }
    l.wave_bytes = kind == ORLG_GROUP_HBMQ ? l.qtime : go;   // the region ends where the ring's slices would begin (they are the last arrays)
    l.shared_bytes = shared_bytes;
    for (int cand = ORLG_GROUP_WAVES; cand >= 1 && !l.wpb_max; cand--)
        if (orlg_group_lds(shared_bytes, cand, l.wave_bytes) <= ORLG_LDS_BYTES) l.wpb_max = cand;
    return l;
}

// A USAGE launch (orlg_step_window under the rule MOST_USED or the route BEST_WINDOW; orlg_usage.h) keeps the four environments'
// prefix sums of the slot usage behind the workgroup's wave regions, 4 * ORLG_USAGE_BYTES(W) per wave on top of the layout: the most
// waves per workgroup, at most `wpb`, that the LDS then holds; 0 = not even one (the launch is refused, or goes to the wave kernel)
static inline int orlg_group_usage_wpb(const OrlgGroupLayout &l, int wpb, int W) {
    while (wpb >= 1 && orlg_group_lds(l.shared_bytes, wpb, l.wave_bytes + 4 * ORLG_USAGE_BYTES(W)) > ORLG_LDS_BYTES) --wpb;
    return wpb;
}

// the lean body keeps its bit-rate histograms on the sixteen lanes of an environment's row, two bit rates per lane (orlg_group_body.h, LANE_HIST)
enum { ORLG_LEAN_MAX_BIT_RATES = 32 };
// (n_bit_rates: the handle's; 0 = not said, which orlg_debug_group_plan's callers rely on.  min_slots: the smallest window the
// handle's slots table holds, 1 = not said: the lean body's pass at a provision takes the links' statistics from their summaries
// (group_link_stats, FROMSUM), which holds for a window of at least one slot -- the table's 0 for a negative bit rate is none)
struct OrlgGroupLaunch { int B, n_steps, stats_level, policy, out_mask, br_width, n_bit_rates = 0, min_slots = 1; };
// the tooling environment: ORLG_NO_DEFER, ORLG_NO_CHUNKS, ORLG_NO_LEAN set; ORLG_GROUP_WPB, ORLG_GROUP_CHUNKS (0 = not set)
struct OrlgGroupOverrides { bool no_defer, no_chunks, no_lean; int wpb, chunks; };
struct OrlgGroupChoice { OrlgGroupKind kind; int wpb; size_t lds_bytes; bool lean; uint32_t ticket_stride; bool long_rounds; };
struct OrlgGroupTickets { int n_quads, nblocks, n_chunks, chunk_steps; uint32_t ticket_advance; };

// long launches with full statistics whose outputs do not read the link statistics step by step: the instantiation that
// logs the links' updates and works them off one link per lane (group_link_replay; link_replay of the wave-per-environment kernel)
static inline bool orlg_defer_link_stats(int stats_level, int n_steps, int out_mask, const OrlgGroupOverrides &ov) {
    return stats_level >= 2 && n_steps >= 16 && !ov.no_defer &&
           !(out_mask & ((1 << ORLG_OUT_AVG_LINK_COMPACT) | (1 << ORLG_OUT_AVG_LINK_UTIL) | ORLG_OUT_PLAIN_BITS));
}

static inline OrlgGroupChoice orlg_group_choose(const OrlgGroupLayout *layouts, const OrlgGroupLaunch &a, const OrlgGroupOverrides &ov, int num_cu) {
    OrlgGroupChoice c = {};
    // launches of very few steps leave the release queue in HBM (the kernel's HBMQ instantiation): without the queue's slices an
    // environment takes half the LDS, and such a launch is bound by the waves a CU keeps resident
    // (a launch that asks for a blocking cause, ORLG_OUT_CAUSE_BIT, or runs an assignment rule, ORLG_OUT_ASSIGN_BIT: the plain kind
    // whatever its length -- the only instantiations with the classifier and with the rules)
    const bool hq = a.n_steps <= ORLG_DIRECT_STEPS && layouts[ORLG_GROUP_HBMQ].wpb_max > layouts[ORLG_GROUP_PLAIN].wpb_max &&
                    !(a.out_mask & ORLG_OUT_PLAIN_BITS);
    const bool df = !hq && orlg_defer_link_stats(a.stats_level, a.n_steps, a.out_mask, ov) && layouts[ORLG_GROUP_DEFER].wpb_max >= 1;
    c.kind = hq ? ORLG_GROUP_HBMQ : df ? ORLG_GROUP_DEFER : ORLG_GROUP_PLAIN;
    const int wpb_max = layouts[c.kind].wpb_max, n_quads = (a.B + 3) / 4;
    // Waves per workgroup: as many as the LDS holds when the batch keeps every CU busy for several rounds (more resident waves
    // per SIMD hide more latency); fewer when that would leave CUs idle or the last round mostly empty.  A round of w waves per
    // CU costs about w + 1.5 (measured: 10 waves per CU step 3 % more environments per second than 8); few rounds count whole.
    c.wpb = wpb_max;
    // (long launches of batches beyond one round of the full workgroup keep it: their rounds are evened out by tickets in chunks
    // of steps, below -- the model here would trade resident waves for whole rounds)
    c.long_rounds = a.n_steps >= 256 && !hq && n_quads >= wpb_max * num_cu && !ov.no_chunks;
    if (!c.long_rounds) {
        double best = 1e300;
        for (int w = wpb_max; w >= 1; --w) {
            const double rounds = (double)n_quads / ((double)num_cu * w);
            // (short launches stride statically over the quads: whole rounds; long ones draw tickets: the last round is partial)
            const double cost = ((rounds < 3.0 || a.n_steps <= 16) ? std::ceil(rounds) : rounds + 0.5) * (w + 1.5);
            if (cost < best - 1e-9) { best = cost; c.wpb = w; }
        }
    }
    if (ov.wpb >= 1 && ov.wpb <= wpb_max) c.wpb = ov.wpb;   // tooling override: waves per workgroup
    c.lds_bytes = orlg_group_lds(layouts[c.kind].shared_bytes, c.wpb, layouts[c.kind].wave_bytes);
    // the lean body of the DEFER instantiations (orlg_rmsa_group_body): first fit over the first path or all of them, no per-step
    // output at all, discrete bit rates, no more of them than a row's lanes count -- what a heuristic's evaluation or a load sweep launches
    c.lean = df && (a.policy == ORLG_POLICY_SP || a.policy == ORLG_POLICY_SAP) && a.out_mask == 0 && a.br_width == 0 && !ov.no_lean &&
             a.n_bit_rates <= ORLG_LEAN_MAX_BIT_RATES && a.min_slots >= 1;
    c.ticket_stride = a.n_steps <= 16 ? 1u : 0u;
    return c;
}

// resident: the workgroups of the chosen kernel and shape the device holds at a time (orlg_handle_resident)
static inline OrlgGroupTickets orlg_group_tickets(const OrlgGroupChoice &c, int B, int n_steps, int resident, const OrlgGroupOverrides &ov) {
    OrlgGroupTickets t = {};
    t.n_quads = (B + 3) / 4;
    t.nblocks = (t.n_quads + c.wpb - 1) / c.wpb;
    if (t.nblocks > resident) t.nblocks = resident;
    // Tickets in chunks of steps (orlg_rmsa_group_kernel, work queue): when the batch is not a multiple of the resident waves, a
    // launch's last round of whole-launch tickets runs at a fraction of the occupancy for a whole launch's time (B = 65 536 on 3072
    // wave slots: 5.33 rounds, the last one 1/3 full and nearly as long as a full one).  With k chunks per quad the tail is one
    // chunk long; a hand-off between waves costs a few microseconds (agent-scope release + acquire) against milliseconds of steps.
    const int slots = t.nblocks * c.wpb;
    int k = 1;
    if (c.long_rounds && !c.ticket_stride && t.n_quads > slots) {   // (exactly one round: 1 116 with chunks against 1 131-1 140 M)
        // Measured (NSFNET-320, 1000-step launches, M env-steps/s by chunks k = 1 / 2 / 3 / 4; r = quads / slots rounds):
        //   B = 16 384 (r = 1.33):   853 / 1 090 / 1 131 / 1 178      B = 49 152 (r = 4):    1 151 / 1 250 / 1 212 / 1 240
        //   B = 24 576 (r = 2):    1 139 / 1 136 / 1 234 / 1 234      B = 65 536 (r = 5.33): 1 206 / 1 259 / 1 249 / 1 235
        //   B = 131 072 (r = 10.7): 1 282 with k = 1, 1 257 with k = 3: after many rounds the waves' finishing times have
        //   spread and the last round is short by itself.
        // A chunk boundary costs a quad ~0.55 % of a 1000-step launch (state store + load, release + acquire); whole rounds
        // (r = 2, 4) gain as well: waves that start together stay in step -- all in the same refill at the same time -- and
        // chunks of different quads break that up.  About eight rounds of tickets are enough:
        k = (int)std::floor(8.0 * slots / t.n_quads + 0.5);
        k = k < 1 ? 1 : (k > 4 ? 4 : k);
        while (k > 1 && n_steps / k < 128) --k;   // (a boundary costs the same whatever the chunk's length)
    }
    // tooling / tests: force the number of chunks (any batch)
    if (ov.chunks >= 1 && ov.chunks <= 64 && !c.ticket_stride && c.kind != ORLG_GROUP_HBMQ) k = ov.chunks < n_steps ? ov.chunks : n_steps;
    t.chunk_steps = (n_steps + k - 1) / k;
    t.n_chunks = (n_steps + t.chunk_steps - 1) / t.chunk_steps;
    // one draw per ticket a wave takes on (the next one is drawn when a ticket is taken up); with chunks every wave draws its first
    // ticket as well
    if (!c.ticket_stride) t.ticket_advance = (uint32_t)t.n_quads * (uint32_t)t.n_chunks + (t.n_chunks > 1 ? (uint32_t)slots : 0u);
    return t;
}
