// orlg_gn_max_margin.h -- the max-margin policy section of the gated wave-per-environment step kernel (orlg_kernels.hip,
// rmsa_body<.., MM>; include/orlg.h orlg_step_max_margin): the window the step proposes is the admitted window whose worst
// margin w = min(GSNR - threshold, neighbour margin) is the largest, found by running the admission check of orlg_gn_slots_path.h over
// every free start of the paths in the route's scope -- the query's code on the step's own LDS: the occupancy row and the release
// ring where the step keeps them, walked in rank order from the ring's head.
//     route SAP          the first path in order that has an admitted window, at its best_slot; later paths are not evaluated
//     route BEST_WINDOW  the path with the largest best_margin (strictly greater: ties go to the lowest index), at its best_slot
//     route PATH_EXT     the path the agent named, at its best_slot; a path out of range proposes nothing
//     fallback           some path in scope has a free window but none is admitted: the lowest free start (S - n included) of the first
//                        such path -- a proposal the step's check refuses (the band of orlg_gn_slots_path.h makes the two agree)
// The section only proposes: the step's own check then runs on the one window like on any proposal.  Not in the reference.
#pragma once
#include "orlg_gn_slots_path.h"

// (path << 10) | slot of the proposal, -1 = no path in scope has a free window; w: the worst margin of an admitted proposal, NaN for a
// fallback.  cidx: Q words of the wave's LDS.  Wave-uniform.
template <int W>
DEV int wave_max_margin(const Wave &wv, const Tab &tb, OrlgGnTable gn, int E, int Q, int q_head, int q_n, uint32_t *cidx, int base, int K, int S,
                        int br, int route, int given, int protect, double &w) {
    const int lane = wv.lane;
    const double nan = __longlong_as_double(0x7ff8000000000000ll), ninf = __longlong_as_double((long long)0xfff0000000000000ull);
    const OrlgGnSlotsConst gk = gn_slots_const(gn);
    int lo = 0, hi = K;
    if (route == ORLG_POLICY_PATH_EXT) {
        lo = given;
        hi = given >= 0 && given < K ? given + 1 : given;
    }
    int got = -1, fallback = -1;
    double top = ninf;
    u64 fit_l = 0ull;
    for (int idp = lo; idp < hi; ++idp) {
        if ((idp & 7) == 0 || idp == lo) fit_l = gn_slots_fit8<W>(wv.occ, tb, base, idp & ~7, K, br, lane);
        const int fl0 = (idp & 7) << 3;
        int first_free = S;   // the lowest free start of the path
#pragma unroll
        for (int c = W - 1; c >= 0; --c) {
            const u64 xc = readlane64(fit_l, fl0 + c);
            first_free = xc ? 64 * c + ctz64(xc) : first_free;
        }
        if (first_free >= S) continue;
        const OrlgPathRec *rec = tb.recs + (base + idp);
        const int se = uni((int)rec->se);
        const int n = uni((int)tb.nslots[br * ORLG_NSLOT_STRIDE + se]);
        OrlgGnSlotsRows<W> r;
        gn_slots_path<W, true>(wv, tb, gn, gk, E, Q, q_head, q_n, cidx, rec, n, fit_l, fl0, protect, r);
        int b_slot;
        double b_w;
        gn_slots_finish<W>(r, gn[ORLG_GN_THR0 + se - 1], S, lane, nullptr, nullptr, nullptr, true, b_slot, b_w);
        wave_sync();   // (the next path compacts into the same offsets)
        if (b_slot < S) {
            if (route != ORLG_POLICY_BEST_WINDOW) {
                got = (idp << 10) | b_slot;
                top = b_w;
                break;
            }
            if (b_w > top) { got = (idp << 10) | b_slot; top = b_w; }
        } else if (fallback < 0) {
            fallback = (idp << 10) | first_free;
        }
    }
    w = got >= 0 ? top : nan;
    return got >= 0 ? got : fallback;
}
