// run_schedule_check.cc -- host check of run_starts' shift schedule (csrc/orlg_run_schedule.h), a program of its own.
//
// (a) Schedule.  For every n of 1..1023 the wave-uniform form (orlg_run_rem0, orlg_run_ku, orlg_run_k: one have_u for all, a
//     remainder per lane) gives the shifts of the per-lane form (orlg_run_k_ref) round for round and ends in the same round; in
//     a "wave" of 64 lanes with different n, where have_u advances for all until the last lane is done, every lane sees its own
//     per-lane sequence followed by zeros.  n = 0 (a slots table entry of a negative bit rate) shifts by 0 throughout.
// (b) Bitmaps.  run_starts restated in plain C++ on that schedule -- a path's W words on W consecutive lanes, the next word's low
//     half where the device reads it by DPP, two 32-bit funnel shifts per word, several paths of different n in one wave -- against
//     a bit-by-bit search: bit b of word w is set exactly when slots 64 w + b .. 64 w + b + n - 1 are all free.  W = 1, 2, 3, 5, 6, 8
//     with S = 64 W, and S = 100, 130, 320, 400; 2 000 random occupancies each at several fill levels (and the all-free and
//     all-used bitmaps); every n of 1..130, then 191, 192, 193 and S.
// Build: c++ -std=c++17 -O1 -fsanitize=address,undefined -I optical-rl-gym-qot-aware_amd/csrc tests/run_schedule_check.cc
// (tests/test_run_schedule.py does).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "orlg_run_schedule.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// ---------------------------------------------------------------------------------------- (a) the schedule
// the per-lane form's shifts for n, until the first 0
static std::vector<int> ref_sequence(int n) {
    std::vector<int> ks;
    for (int have = 1;;) {
        const int k = orlg_run_k_ref(n, have);
        if (k <= 0) break;
        ks.push_back(k);
        have += k;
    }
    return ks;
}

static bool check_single(int n) {
    const std::vector<int> ref = ref_sequence(n);
    int rem = orlg_run_rem0(n), have_u = 1, covered = 1;
    size_t round = 0;
    for (;; ++round) {
        const int ku = orlg_run_ku(have_u), k = orlg_run_k(rem, ku);
        if (k <= 0) break;
        if (round >= ref.size() || ref[round] != k) {
            std::printf("MISMATCH schedule n %d round %zu: k %d, per-lane form %d\n", n, round, k, round < ref.size() ? ref[round] : 0);
            return false;
        }
        if (k > covered || k > ORLG_RUN_MAX_SHIFT) {   // r_{m+k} = r_m & (r_m >> k) needs k <= m
            std::printf("MISMATCH schedule n %d round %zu: k %d with %d slots covered\n", n, round, k, covered);
            return false;
        }
        covered += k;
        rem -= k;
        have_u += ku;
    }
    if (round != ref.size() || covered != n || rem != 0) {
        std::printf("MISMATCH schedule n %d: %zu rounds (per-lane form %zu), %d slots covered, %d left\n", n, round, ref.size(), covered, rem);
        return false;
    }
    return true;
}

static bool check_wave(const int (&n)[64]) {
    std::vector<int> ref[64];
    int rem[64];
    size_t longest = 0;
    for (int l = 0; l < 64; ++l) {
        ref[l] = ref_sequence(n[l]);
        rem[l] = orlg_run_rem0(n[l]);
        longest = ref[l].size() > longest ? ref[l].size() : longest;
    }
    size_t round = 0;
    for (int have_u = 1;; ++round) {
        const int ku = orlg_run_ku(have_u);
        bool any = false;
        int k[64];
        for (int l = 0; l < 64; ++l) {
            k[l] = orlg_run_k(rem[l], ku);
            any = any || k[l] > 0;
        }
        if (!any) break;   // the ballot
        for (int l = 0; l < 64; ++l) {
            const int want = round < ref[l].size() ? ref[l][round] : 0;
            if (k[l] != want) {
                std::printf("MISMATCH wave lane %d (n %d) round %zu: k %d, per-lane form %d\n", l, n[l], round, k[l], want);
                return false;
            }
            rem[l] -= k[l];
        }
        have_u += ku;
    }
    if (round != longest) {
        std::printf("MISMATCH wave: %zu rounds, the longest lane needs %zu\n", round, longest);
        return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------- (b) the bitmaps
static uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t k) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (k & 31u)); }   // v_alignbit_b32

// run_starts<W> on a "wave" of `paths` paths, path q's word w on lane q W + w, n[q] slots each; x is replaced by the result
static void run_starts_wave(std::vector<uint64_t> &x, const std::vector<int> &n, int W) {
    const int paths = (int)n.size(), lanes = paths * W;
    std::vector<uint32_t> lo(lanes), hi(lanes), keep(lanes), nlo(lanes);
    std::vector<int> rem(lanes), k(lanes);
    for (int l = 0; l < lanes; ++l) {
        lo[l] = (uint32_t)x[l];
        hi[l] = (uint32_t)(x[l] >> 32);
        keep[l] = (l % W) == W - 1 ? 0u : ~0u;
        rem[l] = orlg_run_rem0(n[l / W]);
    }
    for (int have_u = 1;;) {
        const int ku = orlg_run_ku(have_u);
        bool any = false;
        for (int l = 0; l < lanes; ++l) {
            k[l] = orlg_run_k(rem[l], ku);
            any = any || k[l] > 0;
        }
        if (!any) break;
        for (int l = 0; l < lanes; ++l) nlo[l] = (l + 1 < lanes ? lo[l + 1] : 0u) & keep[l];   // the next lane's, 0 past the row's end
        for (int l = 0; l < lanes; ++l) {
            const uint32_t slo = alignbit(hi[l], lo[l], (uint32_t)k[l]), shi = alignbit(nlo[l], hi[l], (uint32_t)k[l]);
            lo[l] &= slo;
            hi[l] &= shi;
            rem[l] -= k[l];
        }
        have_u += ku;
    }
    for (int l = 0; l < lanes; ++l) x[l] = ((uint64_t)hi[l] << 32) | lo[l];
}

// one occupancy of S slots (free[s]), checked for every n of `ns`: the paths of a wave are the same bitmap with different n
static bool check_bitmap(const std::vector<uint8_t> &free_, int W, int S, const std::vector<int> &ns, const char *what, long long &checked) {
    std::vector<int> run(64 * W + 1, 0);   // run[s]: free slots from s on
    for (int s = 64 * W - 1; s >= 0; --s) run[s] = (s < S && free_[s]) ? run[s + 1] + 1 : 0;
    std::vector<uint64_t> words(W, 0ull);
    for (int s = 0; s < S; ++s)
        if (free_[s]) words[s >> 6] |= 1ull << (s & 63);   // (slots at and beyond S: stored as not free)
    const int per_wave = 64 / W;
    for (size_t i0 = 0; i0 < ns.size(); i0 += per_wave) {
        std::vector<int> n(ns.begin() + i0, ns.begin() + (i0 + per_wave < ns.size() ? i0 + per_wave : ns.size()));
        std::vector<uint64_t> x;
        for (size_t q = 0; q < n.size(); ++q) x.insert(x.end(), words.begin(), words.end());
        run_starts_wave(x, n, W);
        for (size_t q = 0; q < n.size(); ++q)
            for (int w = 0; w < W; ++w) {
                uint64_t want = 0ull;
                for (int b = 0; b < 64; ++b)
                    if (run[64 * w + b] >= n[q]) want |= 1ull << b;
                if (x[q * W + w] != want) {
                    std::printf("MISMATCH bitmap (%s) W %d S %d n %d word %d: %016llx, bit by bit %016llx\n", what, W, S, n[q], w,
                                (unsigned long long)x[q * W + w], (unsigned long long)want);
                    return false;
                }
                checked += 1;
            }
    }
    return true;
}

int main() {
    // (a)
    for (int n = 1; n <= 1023; ++n)
        if (!check_single(n)) return 1;
    {
        int rem = orlg_run_rem0(0);
        for (int have_u = 1; have_u < 200; have_u += orlg_run_ku(have_u))
            if (rem != 0 || orlg_run_k(rem, orlg_run_ku(have_u)) != 0) {
                std::printf("MISMATCH schedule n 0 shifts\n");
                return 1;
            }
    }
    long long waves = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        int n[64];
        const int top = trial % 4 == 0 ? 1023 : (trial % 4 == 1 ? 130 : (trial % 4 == 2 ? 40 : 8));
        for (int l = 0; l < 64; ++l) n[l] = (rnd() % 3 == 0) ? 1 : 1 + (int)(rnd() % (uint64_t)top);   // (1: a lane that does not look)
        if (trial % 7 == 0)
            for (int l = 0; l < 64; ++l) n[l] = 1;
        if (trial % 11 == 0) n[rnd() % 64] = 31 + (int)(rnd() % 3);
        if (trial % 13 == 0) n[rnd() % 64] = 62 + (int)(rnd() % 4);
        if (trial % 17 == 0) n[rnd() % 64] = 94 + (int)(rnd() % 2);
        if (!check_wave(n)) return 1;
        waves += 1;
    }

    // (b)
    static const int shapes[][2] = {{1, 64}, {2, 128}, {3, 192}, {5, 320}, {6, 384}, {8, 512}, {2, 100}, {3, 130}, {8, 400}};
    long long words = 0, bitmaps = 0;
    for (const auto &sh : shapes) {
        const int W = sh[0], S = sh[1];
        std::vector<int> ns;
        for (int n = 1; n <= 130; ++n) ns.push_back(n);
        for (int n : {191, 192, 193, S}) ns.push_back(n);
        std::vector<uint8_t> f(S, 1);
        if (!check_bitmap(f, W, S, ns, "all free", words)) return 1;
        f.assign(S, 0);
        if (!check_bitmap(f, W, S, ns, "all used", words)) return 1;
        for (int trial = 0; trial < 2000; ++trial) {
            const int level = trial % 5;
            if (level < 4) {
                // every slot used with probability 1/64, 1/16, 1/4, 1/2
                const uint64_t den = level == 0 ? 64 : (level == 1 ? 16 : (level == 2 ? 4 : 2));
                for (int s = 0; s < S; ++s) f[s] = rnd() % den != 0;
            } else {
                // free runs of the lengths at which the schedule changes its step, a few used slots between them
                static const int lens[] = {1, 2, 3, 7, 8, 15, 16, 17, 30, 31, 32, 33, 34, 61, 62, 63, 64, 65, 66, 93, 94, 95, 96, 127, 128, 129, 130, 131};
                int s = (int)(rnd() % 4);
                f.assign(S, 0);
                while (s < S) {
                    const int len = lens[rnd() % (sizeof lens / sizeof lens[0])];
                    for (int i = 0; i < len && s < S; ++i) f[s++] = 1;
                    s += 1 + (int)(rnd() % 3);
                }
            }
            if (!check_bitmap(f, W, S, ns, "random", words)) return 1;
            bitmaps += 1;
        }
    }
    std::printf("run schedule: n = 1..1023 and %lld waves of mixed n agree with the per-lane schedule; %lld bitmaps, %lld words agree bit by bit\n",
                waves, bitmaps, words);
    return 0;
}
