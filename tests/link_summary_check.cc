// link_summary_check.cc -- host check of the link summary's arithmetic at a provision (csrc/orlg_link_summary.h), a program of
// its own.
//
// For S = 64, 100, 128, 320 and 400 slots (one to eight words per link: seven words of slots run on the eight-word layout, so at
// S = 400 slot S - 1 is not in the last word): bitmaps at several densities -- the empty link, links with one free run (at the
// start, in the middle, at the end), used runs drawn at random with long and short free runs between them, single random bits --
// and on each EVERY wholly free window [s, e) of every length, s = 0, e = S, s and e on word boundaries and windows over three
// words among them.  The summary of the bitmap before (packed and unpacked, as the device holds it), the window and the two
// neighbouring bits -- read from the link's words the way the device reads them, slots at and beyond S stored as not free -- give
// the seven fields after (orlg_lsum_provision); they are compared with a plain bit-loop recount of the cleared bitmap, written
// here.  The longest free run is the caller's: the recount's own goes in and has to come out.  Pack and unpack round-trip on
// every summary met and at the fields' limits.
// Build: c++ -std=c++17 -O1 -fsanitize=address,undefined -I optical-rl-gym-qot-aware_amd/csrc tests/link_summary_check.cc
// (tests/test_link_summary.py does).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "orlg_link_summary.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int words_of(int S) {
    const int w = (S + 63) / 64;
    return w == 7 ? 8 : w;
}

struct Link {
    int S;
    std::vector<uint64_t> x;   // bit = free; slots at and beyond S are 0
    bool free_at(int i) const { return (x[i >> 6] >> (i & 63)) & 1ull; }
    void set_free(int i, bool f) {
        if (f) x[i >> 6] |= 1ull << (i & 63);
        else x[i >> 6] &= ~(1ull << (i & 63));
    }
};

// the plain recount: one loop over the slots 0 .. S - 1, nothing shared with the header
static OrlgLinkSummary recount(const Link &l) {
    OrlgLinkSummary r = {0, 0, 0, 0x7fff, 0, 0, false, false};
    int run = 0;
    for (int i = 0; i < l.S; ++i) {
        const bool f = l.free_at(i), before = i > 0 && l.free_at(i - 1);
        if (f) {
            r.freec += 1;
            if (i == 0 || !before) { r.F += 1; run = 0; }
            run += 1;
            if (run > r.ml) r.ml = run;
        } else {
            if (i == 0 || before) r.U += 1;
            if (r.lmin == 0x7fff) r.lmin = i;
            r.lmax = i + 1;
        }
    }
    r.ff = l.free_at(0);
    r.lf = l.free_at(l.S - 1);
    return r;
}

static long long failures = 0;
static void fail(const char *what, int S, int s, int e, long long got, long long want) {
    if (failures < 20) std::printf("MISMATCH %s S=%d window [%d, %d): got %lld, want %lld\n", what, S, s, e, got, want);
    failures += 1;
}

static bool same_fields(const OrlgLinkSummary &a, const OrlgLinkSummary &b) {
    return a.freec == b.freec && a.F == b.F && a.U == b.U && a.lmin == b.lmin && a.lmax == b.lmax && a.ml == b.ml && a.ff == b.ff && a.lf == b.lf;
}

static void round_trip(const OrlgLinkSummary &v, int S) {
    OrlgLinkSummary want = v;
    want.lmin &= 0x3ff;   // (the stored lmin of a link without a used slot)
    const OrlgLinkSummary got = lsum_unpack(lsum_pack(v.freec, v.F, v.U, v.lmin, v.lmax, v.ml, v.ff, v.lf));
    if (!same_fields(got, want)) fail("round trip", S, v.lmin, v.lmax, got.freec, want.freec);
}

// what the windows of all bitmaps reached
static long long n_windows, n_u0, n_ab[3], n_s0, n_eS, n_s_word, n_e_word, n_three_words, n_runs_vanish, n_joins_two;

static void every_window(const Link &l) {
    const int S = l.S;
    const OrlgLinkSummary before = recount(l);
    round_trip(before, S);
    const OrlgLinkSummary held = lsum_unpack(lsum_pack(before.freec, before.F, before.U, before.lmin, before.lmax, before.ml, before.ff, before.lf));
    for (int s = 0; s < S; ++s) {
        Link c = l;
        for (int e = s + 1; e <= S && l.free_at(e - 1); ++e) {
            c.set_free(e - 1, false);   // c: l with [s, e) cleared
            const OrlgLinkSummary want = recount(c);
            // the neighbours as the device reads them: from the words, the index clamped
            const uint64_t xa = l.x[orlg_lsum_word_below(S, s)], xb = c.x[orlg_lsum_word_above(S, e)];
            const bool a = orlg_lsum_free_below(xa, S, s), b = orlg_lsum_free_above(xb, S, e);
            const OrlgLinkSummary got = orlg_lsum_provision(held, S, s, e - s, a, b, want.ml);
            if (got.freec != want.freec) fail("free slots", S, s, e, got.freec, want.freec);
            if (got.F != want.F) fail("free runs", S, s, e, got.F, want.F);
            if (got.U != want.U) fail("used runs", S, s, e, got.U, want.U);
            if (got.lmin != want.lmin) fail("first used slot", S, s, e, got.lmin, want.lmin);
            if (got.lmax != want.lmax) fail("end of the last used run", S, s, e, got.lmax, want.lmax);
            if (got.ml != want.ml) fail("longest free run", S, s, e, got.ml, want.ml);
            if (got.ff != want.ff) fail("slot 0 free", S, s, e, got.ff, want.ff);
            if (got.lf != want.lf) fail("slot S - 1 free", S, s, e, got.lf, want.lf);
            round_trip(got, S);
            n_windows += 1;
            n_u0 += before.U == 0;
            n_ab[(a ? 1 : 0) + (b ? 1 : 0)] += 1;
            n_s0 += s == 0;
            n_eS += e == S;
            n_s_word += s > 0 && (s & 63) == 0;
            n_e_word += e < S && (e & 63) == 0;
            n_three_words += ((e - 1) >> 6) - (s >> 6) >= 2;
            n_runs_vanish += want.F == before.F - 1;
            n_joins_two += want.U == before.U - 1;
        }
    }
}

static Link all_used(int S) { return Link{S, std::vector<uint64_t>(words_of(S), 0ull)}; }

static Link one_free_run(int S, int from, int to) {
    Link l = all_used(S);
    for (int i = from; i < to; ++i) l.set_free(i, true);
    return l;
}

// used and free runs in turn, their lengths uniform in 1 .. max_used / 1 .. max_free
static Link random_runs(int S, int max_used, int max_free) {
    Link l = all_used(S);
    bool f = rnd() & 1;
    for (int i = 0; i < S;) {
        const int len = 1 + (int)(rnd() % (uint64_t)(f ? max_free : max_used));
        for (int j = 0; j < len && i < S; ++j, ++i) l.set_free(i, f);
        f = !f;
    }
    return l;
}

static Link random_bits(int S, int free_percent) {
    Link l = all_used(S);
    for (int i = 0; i < S; ++i) l.set_free(i, (int)(rnd() % 100) < free_percent);
    return l;
}

int main() {
    const int sizes[] = {64, 100, 128, 320, 400};
    for (int S : sizes) {
        every_window(one_free_run(S, 0, S));           // the empty link
        every_window(one_free_run(S, 0, S / 2));       // one free run: at the start,
        every_window(one_free_run(S, S / 3, S - 5));   // in the middle (over a word boundary from S = 100 on),
        every_window(one_free_run(S, S - 40, S));      // at the end
        every_window(one_free_run(S, 1, S - 1));       // and between slot 0 and slot S - 1 in use
        every_window(all_used(S));                     // (no window: the summary alone)
        for (int rep = 0; rep < 6; ++rep) {
            every_window(random_runs(S, 4, 200));      // mostly free, long free runs (windows over three words)
            every_window(random_runs(S, 12, 70));
            every_window(random_runs(S, 12, 12));
            every_window(random_runs(S, 60, 6));       // mostly used
            every_window(random_bits(S, 50));
            every_window(random_bits(S, 90));
        }
    }
    // a lane that provisions nothing reads a word of the link all the same, whatever its window says
    for (int S : sizes)
        for (int i = -70; i <= S + 70; ++i) {
            const int wa = orlg_lsum_word_below(S, i), wb = orlg_lsum_word_above(S, i);
            if (wa < 0 || wa >= words_of(S) || wb < 0 || wb >= words_of(S)) fail("word index", S, i, i, wa, wb);
            if ((i < 1 || i > S) && (wa != 0 || orlg_lsum_free_below(~0ull, S, i))) fail("no slot below", S, i, i, wa, 0);
            if ((i < 0 || i >= S) && (wb != 0 || orlg_lsum_free_above(~0ull, S, i))) fail("no slot above", S, i, i, wb, 0);
        }
    // the fields' limits
    round_trip(OrlgLinkSummary{1023, 1023, 1023, 1023, 1023, 1023, true, true}, 0);
    round_trip(OrlgLinkSummary{0, 0, 0, 0x7fff, 0, 0, false, false}, 0);
    round_trip(OrlgLinkSummary{1023, 0, 0, 0, 1023, 0, false, true}, 0);
    round_trip(OrlgLinkSummary{0, 1023, 0, 1023, 0, 1023, true, false}, 0);
    std::printf("windows %lld: empty link %lld, a + b = 0 / 1 / 2: %lld / %lld / %lld, s = 0 %lld, e = S %lld, s on a word boundary %lld, "
                "e on a word boundary %lld, over three words %lld, a free run vanishes %lld, two used runs join %lld\n",
                n_windows, n_u0, n_ab[0], n_ab[1], n_ab[2], n_s0, n_eS, n_s_word, n_e_word, n_three_words, n_runs_vanish, n_joins_two);
    const long long reached[] = {n_u0, n_ab[0], n_ab[1], n_ab[2], n_s0, n_eS, n_s_word, n_e_word, n_three_words, n_runs_vanish, n_joins_two};
    for (long long r : reached)
        if (r == 0) { std::printf("a case was not reached\n"); return 1; }
    if (failures) { std::printf("%lld mismatches\n", failures); return 1; }
    std::printf("summary and recount agree on every window\n");
    return 0;
}
