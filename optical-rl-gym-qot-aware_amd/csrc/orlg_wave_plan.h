// orlg_wave_plan.h -- what the host decides about a launch of the wave-per-environment step kernels (orlg_kernels.hip): which kernel
// family and which key of it (orlg_variants.h) serve the launch, the workgroup of a launch that keeps something behind the wave regions
// in LDS, the grid and the tickets.  Arithmetic only -- no HIP call, no environment variable, no handle -- so all of it runs without
// a device (orlg_debug_wave_plan); launch_rmsa and launch_wave (orlg_api_step.hip) do what it says.  A new variant of the kernel is
// one row of orlg_wave_choose and one entry of a key list.
#pragma once
#include <cstddef>
#include <cstdint>

#include "orlg_group_plan.h"   // orlg_defer_link_stats
#include "orlg_variants.h"

// ---------------------------------------------------------------------------------------- which kernel
// orlg_rmsa_kernel / _ff / reset (OrlgWaveKey), orlg_rmsa_mm_kernel (OrlgMmKey), orlg_rmsa_am_kernel (OrlgAmKey)
enum OrlgWaveFamily { ORLG_WAVE_PLAIN, ORLG_WAVE_MM, ORLG_WAVE_AM };
// the launch: OrlgParams' mode, policy, K, stats_level, n_steps, out_mask and assign; the handle has a gate, the gate chooses the
// modulation, the gate protects the running lightpaths; the call is orlg_step_max_margin's; ORLG_NO_DEFER is set
struct OrlgWaveAsk { int mode, policy, K, stats_level, n_steps, out_mask, assign; bool gated, adaptive, protect, max_margin, no_defer; };
struct OrlgWaveChoice { OrlgWaveFamily family; OrlgWaveKey key; OrlgMmKey mm; OrlgAmKey am; };

static inline OrlgWaveChoice orlg_wave_choose(const OrlgWaveAsk &a) {
    const bool step = a.mode == ORLG_MODE_STEP;
    OrlgWaveChoice c = {ORLG_WAVE_PLAIN, {ORLG_WAVE_KERNEL(orlg_rmsa_reset_kernel), a.stats_level, false}, {a.stats_level}, {a.stats_level}};
    // a launch that asks for the blocking cause: the CAUSE instantiation, with or without the check
    const bool cause = step && (a.out_mask & ORLG_OUT_CAUSE_BIT) != 0;
    // orlg_step_max_margin (a step behind a gate: orlg_step_mm_call): its own kernel, without and with the classifier
    if (a.max_margin) {
        c.family = ORLG_WAVE_MM;
        c.mm.CAUSE = cause;
        return c;
    }
    // a step of a handle whose gate chooses the modulation: its own kernel whatever the policy -- its decode knows the levels
    if (step && a.gated && a.adaptive) {
        c.family = ORLG_WAVE_AM;
        return c;
    }
    if (!step) return c;   // the initial and the episode reset: the reset kernel, which has no DEFER
    // a step of a handle with a GN-model admission check: the general kernel's GN instantiation, whatever the policy and the length
    const bool gn = a.gated;
    // a launch under an assignment rule other than the reference's first fit: the ASSIGN instantiation (behind a gate:
    // orlg_step_rule_gn alone, every other entry refuses); with it the fewest-cuts window (CUT) or MOST_USED / BEST_WINDOW (USAGE)
    const bool assign = (a.out_mask & ORLG_OUT_ASSIGN_BIT) != 0;
    const bool usage = assign && (a.assign == ORLG_ASSIGN_MOST_USED || a.policy == ORLG_POLICY_BEST_WINDOW);
    // the first-fit kernel: the first-fit policies over at most eight paths, and none of the above
    const bool ff = !gn && !cause && !assign && a.K <= 8 && (a.policy == ORLG_POLICY_SP || a.policy == ORLG_POLICY_SAP);
    // the links' float64 statistics deferred: as the group kernel's launches, and never behind a gate
    const bool df = !gn && orlg_defer_link_stats(a.stats_level, a.n_steps, a.out_mask, {a.no_defer, false, false, 0, 0});
    c.key = {ff ? ORLG_WAVE_KERNEL(orlg_rmsa_kernel_ff) : ORLG_WAVE_KERNEL(orlg_rmsa_kernel), a.stats_level, df, gn, cause, assign,
             assign && a.assign == ORLG_ASSIGN_MIN_CUT, usage, gn && a.protect};
    return c;
}

// ---------------------------------------------------------------------------------------- the workgroup
// A launch that keeps `extra_per_wave` bytes behind each wave region (a USAGE launch: ORLG_USAGE_BYTES(W), the wave's prefix sums of
// the slot usage; orlg_rmsa_mm_kernel: up16(4 Q), the compacted services of the path under evaluation): the most waves per workgroup,
// at most `wpb`, that the LDS then holds, and the workgroup's LDS bytes.  wpu = 0 where one wave does not fit (lds: what it would take)
struct OrlgWaveShape { int wpu; size_t lds; };
static inline OrlgWaveShape orlg_wave_extra_lds(size_t shared_bytes, size_t wave_bytes, size_t extra_per_wave, int wpb) {
    const size_t per_wave = wave_bytes + extra_per_wave;
    int wpu = wpb;
    while (wpu > 1 && shared_bytes + wpu * per_wave > ORLG_LDS_BYTES) --wpu;
    const size_t lds = shared_bytes + wpu * per_wave;
    return {lds > ORLG_LDS_BYTES ? 0 : wpu, lds};
}

// ---------------------------------------------------------------------------------------- the grid and the tickets
// resident: the workgroups the device holds at a time (orlg_handle_resident).  A launch of at most 16 steps, and the two resets,
// stride statically over the environments (ticket_stride 1); a longer one draws tickets: waves * 1 static environment + (B - waves)
// tickets + one failing draw per wave move the handle's ticket_base by B.  (The MM and AM kernels are launched in step mode only.)
struct OrlgWaveGrid { int nblocks; uint32_t ticket_stride, ticket_advance; };
static inline OrlgWaveGrid orlg_wave_grid(int B, int wpu, int resident, int mode, int n_steps) {
    OrlgWaveGrid g = {(B + wpu - 1) / wpu, (mode != ORLG_MODE_STEP || n_steps <= 16) ? 1u : 0u, 0u};
    if (g.nblocks > resident) g.nblocks = resident;
    if (!g.ticket_stride) g.ticket_advance = (uint32_t)B;
    return g;
}
