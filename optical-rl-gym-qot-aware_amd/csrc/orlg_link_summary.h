// orlg_link_summary.h -- a link's summary of the group kernel's DEFER instantiations, said once for the device and the host.
//
// The summary (LDS only, 8 bytes per link) holds every integer _update_link_stats consumes, 10 bits each: free slots, free runs,
// used runs, first used slot (lmin), end of the last used run (lmax: one past its last slot), longest free run (ml), and two bits:
// slot 0 free, slot S - 1 free.  With no used slot lmin / lmax are group_link_stats' 0x7fff / 0 and lmin keeps only its low 10
// bits (0x3ff): a reader that wants a slot asks U first.
//
// Provision.  A window [s, e), e = s + n, that was WHOLLY FREE is taken out of one free run.  With
//     a = s > 0 and slot s - 1 free,   b = e < S and slot e free
// (slots at and beyond S are stored as not free and are no used slots; with e < S tested first nothing else is needed for them)
//     free slots   freec - n
//     free runs    F - 1 + a + b            the run is gone, and a piece of it stays on either side that is free
//     used runs    U + 1 - [s > 0 and not a] - [e < S and not b]     the window joins the used run it touches on either side
//     first used   U == 0 ? s : min(lmin, s)      (U == 0: the stored lmin is no slot)
//     last end     U == 0 ? e : max(lmax, e)
//     slot 0 free  ff and s != 0,   slot S - 1 free  lf and e != S
// The longest free run does not follow from these: it is the one field the caller brings (orlg_lsum_provision's ml), from a scan
// of the link's words.  tests/link_summary_check.cc holds all of it to a bit-by-bit recount for every wholly free window of
// bitmaps of 64 .. 400 slots.
#pragma once
#include "orlg_math.h"   // ORLG_HD

#define ORLG_LSUM_FN ORLG_HD __attribute__((always_inline))

struct OrlgLinkSummary {
    int freec, F, U;   // free slots, free runs, used runs
    int lmin, lmax;    // first used slot, end of the last used run (U == 0: 0x3ff as stored / 0x7fff as computed, and 0)
    int ml;            // longest free run
    bool ff, lf;       // slot 0 free, slot S - 1 free
};

ORLG_LSUM_FN uint64_t lsum_pack(int freec, int F, int U, int lmin, int lmax, int ml, bool ff, bool lf) {
    return (uint64_t)((uint32_t)freec | ((uint32_t)F << 10) | ((uint32_t)U << 20)) |
           ((uint64_t)((uint32_t)(lmin & 0x3ff) | ((uint32_t)lmax << 10) | ((uint32_t)ml << 20) | ((uint32_t)ff << 30) | ((uint32_t)lf << 31)) << 32);
}

ORLG_LSUM_FN OrlgLinkSummary lsum_unpack(uint64_t sm) {
    const uint32_t lo = (uint32_t)sm, hi = (uint32_t)(sm >> 32);
    OrlgLinkSummary r;
    r.freec = (int)(lo & 0x3ffu);
    r.F = (int)((lo >> 10) & 0x3ffu);
    r.U = (int)((lo >> 20) & 0x3ffu);
    r.lmin = (int)(hi & 0x3ffu);
    r.lmax = (int)((hi >> 10) & 0x3ffu);
    r.ml = (int)((hi >> 20) & 0x3ffu);
    r.ff = ((hi >> 30) & 1u) != 0u;
    r.lf = (hi >> 31) != 0u;
    return r;
}

// The window's two neighbours in a link's words (bit = free; slots at and beyond S are stored as 0): the word that holds slot
// s - 1 / slot e -- word 0 where there is no such slot -- and the bit in it.  The index is a word of the link for EVERY s and e,
// also those of a lane that provisions nothing (a first fit that found no window leaves -1): one unsigned comparison says
// 0 <= slot < S, so that the read stands outside every condition.  The window itself does not reach either slot: the words may
// be read before or after it is cleared.
ORLG_LSUM_FN bool orlg_lsum_is_slot(int S, int i) { return (uint32_t)i < (uint32_t)S; }
ORLG_LSUM_FN int orlg_lsum_word_below(int S, int s) { return orlg_lsum_is_slot(S, s - 1) ? (s - 1) >> 6 : 0; }
ORLG_LSUM_FN int orlg_lsum_word_above(int S, int e) { return orlg_lsum_is_slot(S, e) ? e >> 6 : 0; }
ORLG_LSUM_FN bool orlg_lsum_free_below(uint64_t x, int S, int s) { return orlg_lsum_is_slot(S, s - 1) && ((x >> ((s - 1) & 63)) & 1ull) != 0ull; }
ORLG_LSUM_FN bool orlg_lsum_free_above(uint64_t x, int S, int e) { return orlg_lsum_is_slot(S, e) && ((x >> (e & 63)) & 1ull) != 0ull; }

// The summary after the wholly free window [s, s + n) was provisioned, from the one before: a, b as above, ml the link's
// longest free run after it (the caller's scan).  With no used slot before, lmin is the window's own start, whatever was stored.
ORLG_LSUM_FN OrlgLinkSummary orlg_lsum_provision(OrlgLinkSummary o, int S, int s, int n, bool a, bool b, int ml) {
    const int e = s + n;
    OrlgLinkSummary r;
    r.freec = o.freec - n;
    r.F = o.F - 1 + (a ? 1 : 0) + (b ? 1 : 0);
    r.U = o.U + 1 - ((s > 0 && !a) ? 1 : 0) - ((e < S && !b) ? 1 : 0);
    const int lo = o.lmin < s ? o.lmin : s, hi = o.lmax > e ? o.lmax : e;
    r.lmin = o.U == 0 ? s : lo;
    r.lmax = o.U == 0 ? e : hi;
    r.ml = ml;
    r.ff = o.ff && s != 0;
    r.lf = o.lf && e != S;
    return r;
}
