// orlg_run_schedule.h -- the shift schedule of run_starts' doubling loop (orlg_spectrum.h), said once for the device and the host.
//
// run_starts keeps r_m = AND of x >> 0 .. x >> (m - 1) and doubles it: r_{m+k} = r_m & (r_m >> k) for any k <= m, with k <= 31 so
// that a shift is two 32-bit funnel shifts.  A lane that wants windows of n slots starts at m = 1 and takes, round for round,
//     k = min(n - m, m, 31),  m += k                                   (orlg_run_k_ref: the per-lane form, the reference of the test)
// until k = 0.  The lanes of a wave want different n, and the loop runs until the last has finished.
//
// Invariant.  m starts at 1 on every lane, and a lane that has slots to go AFTER a round took k = min(m, 31) in it -- the n - m
// term did not bind, or the lane would be done.  So as long as a lane is not done its m is the same number as every other such
// lane's: one value for the wave, have_u, which advances by ku = min(have_u, 31) a round whatever the lanes do.  A lane needs only
// its remainder:
//     rem = n - 1;   per round  k = min(rem, ku),  rem -= k            (orlg_run_rem0, orlg_run_ku, orlg_run_k)
// While rem > ku the lane's m is have_u and k = ku = min(m, 31) <= n - m; in the round rem <= ku the lane takes k = rem = n - m
// <= min(m, 31) and is done; from then on rem = 0 and k = 0, which is what the per-lane form gives with m = n.  The k are the same
// numbers on every lane, round for round, and so are the round count and the result.  On the device have_u and ku live in scalar
// registers; rem is the only per-lane state (tests/run_schedule_check.cc holds the two forms together for every n and for waves
// of mixed n, and a restatement of run_starts on this schedule against a bit-by-bit search).
//
// Precondition: n >= 1.  Every caller takes n from the slots table (get_number_slots = ceil(bit rate / (SE width)) + 1, at least 1
// for a bit rate >= 0) or passes 1 on a lane that does not look.  The create call does not refuse a negative bit rate, for which
// the table holds 0: orlg_run_rem0 clamps the remainder at 0, so that such a lane shifts by 0 like a lane with n = 1 (the
// per-lane form would have shifted by n - 1 mod 32).
#pragma once
#include "orlg_math.h"   // ORLG_HD

#define ORLG_RUN_FN ORLG_HD __attribute__((always_inline))
#define ORLG_RUN_MAX_SHIFT 31   // one v_alignbit_b32 shifts by 0..31

// slots a lane has to go beyond the one it starts with
ORLG_RUN_FN int orlg_run_rem0(int n) { return n > 1 ? n - 1 : 0; }
// the wave's step of a round: have_u += orlg_run_ku(have_u) after it, from have_u = 1
ORLG_RUN_FN int orlg_run_ku(int have_u) { return have_u < ORLG_RUN_MAX_SHIFT ? have_u : ORLG_RUN_MAX_SHIFT; }
// the lane's shift of a round: rem -= k after it
ORLG_RUN_FN int orlg_run_k(int rem, int ku) { return rem < ku ? rem : ku; }

// the per-lane form: the lane's shift with `have` slots covered, have += k after it, from have = 1 (n >= 1)
ORLG_RUN_FN int orlg_run_k_ref(int n, int have) {
    int k = n - have;
    k = k < have ? k : have;
    return k < ORLG_RUN_MAX_SHIFT ? k : ORLG_RUN_MAX_SHIFT;
}
