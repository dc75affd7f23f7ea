// graph_log_check.cc -- host check of the lean body's graph log (csrc/orlg_graph_log.h), a program of its own.
//
// Random sequences of accepted provisions, with every packed field at its limits, go through two routes:
//   batched     the device's: orlg_glog_pack into a row of ORLG_GLOG_CAP lanes, a replay whenever the row is full or at a random
//               earlier point (a ticket's end), and the replay as group_graph_replay does it -- orlg_glog_eval on every lane with the
//               previous lane's time, then orlg_glog_chain down the row, lane k in iteration k, as long as the wave's longest row;
//   sequential  _update_network_stats (rmsa_env.py:537-560) restated plainly on the unpacked values, one update after the other.
// The three doubles must agree bit for bit after every replay.  Build: c++ -std=c++17 -O1 -ffp-contract=off
// -fsanitize=address,undefined -I optical-rl-gym-qot-aware_amd/csrc tests/graph_log_check.cc (tests/test_graph_log.py does).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "orlg_graph_log.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static double unit() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }

// a value of [0, limit]: the ends and their neighbours as often as the middle
static long long field(long long limit) {
    switch (rnd() % 8) {
        case 0: return 0;
        case 1: return 1;
        case 2: return limit;
        case 3: return limit - 1;
        default: return (long long)(rnd() % (uint64_t)(limit + 1));
    }
}

struct Update {
    double now;
    long long br;
    int span, sh, gaps;
};

struct Stats {
    double thr, comp, lu;
};

static void sequential(Stats &g, const Update &u, int E) {
    double comp = 1.0;
    if (u.gaps > 0) comp = ((double)u.span / (double)u.sh) * ((double)E / (double)u.gaps);
    if (u.now > 0) {
        const double time_diff = u.now - g.lu;
        g.thr = ((g.thr * g.lu) + ((double)u.br * time_diff)) / u.now;
        g.comp = ((g.comp * g.lu) + (comp * time_diff)) / u.now;
    }
    g.lu = u.now;
}

// group_graph_replay on one row: lg[k] = lane k's entry, cnt entries; nmax >= cnt: the longest row of the wave
static void replay(Stats &g, const OrlgGraphEntry *lg, int cnt, int nmax, int E) {
    OrlgGraphTerm t[ORLG_GLOG_CAP];
    double lu[ORLG_GLOG_CAP], x_thr[ORLG_GLOG_CAP] = {g.thr}, x_comp[ORLG_GLOG_CAP] = {g.comp}, o_thr[ORLG_GLOG_CAP], o_comp[ORLG_GLOG_CAP];
    for (int gl = 0; gl < ORLG_GLOG_CAP; ++gl) {
        lu[gl] = gl == 0 ? g.lu : lg[gl - 1].now;
        t[gl] = orlg_glog_eval(lg[gl], lu[gl], E);
    }
    for (int k = 0; k < nmax; ++k) {
        for (int gl = 0; gl < ORLG_GLOG_CAP; ++gl) {
            const bool upd = gl < cnt && t[gl].now > 0;
            o_thr[gl] = upd ? orlg_glog_chain(x_thr[gl], lu[gl], t[gl].c_thr, t[gl].now, t[gl].ynow) : x_thr[gl];
            o_comp[gl] = upd ? orlg_glog_chain(x_comp[gl], lu[gl], t[gl].c_comp, t[gl].now, t[gl].ynow) : x_comp[gl];
        }
        for (int gl = ORLG_GLOG_CAP - 1; gl > 0; --gl) { x_thr[gl] = o_thr[gl - 1]; x_comp[gl] = o_comp[gl - 1]; }   // row_shr:1
        x_thr[0] = x_comp[0] = 0.0;                                                                                  // (0 at the row's start)
    }
    g.thr = o_thr[nmax - 1];
    g.comp = o_comp[nmax - 1];
    g.lu = lg[cnt - 1].now;
}

static bool same(const Stats &a, const Stats &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    long long updates = 0, replays = 0, full = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        const int E = 1 + (int)(rnd() % 255);
        Stats a = {0.0, 0.0, 0.0}, b = a;
        if (trial % 3) {   // a state that has run before
            a.lu = unit() * 1e6;
            a.thr = unit() * (double)ORLG_GLOG_MAX_Q * 2147483647.0;
            a.comp = unit() * 300.0;
            b = a;
        }
        OrlgGraphEntry lg[ORLG_GLOG_CAP];
        std::memset(lg, 0, sizeof lg);
        int cnt = 0;
        double now = a.lu;
        const int n = 1 + (int)(rnd() % 70);
        for (int i = 0; i < n; ++i) {
            Update u;
            // the clock: mostly forward, sometimes standing still (two arrivals of one time), 0 at a fresh state's first step
            if (!(trial % 3 == 0 && i == 0 && rnd() % 2)) now += (rnd() % 5) ? unit() * 10.0 : 0.0;
            u.now = now;
            u.br = field((long long)ORLG_GLOG_MAX_Q * 0x7fffffffLL);
            u.span = (int)field(ORLG_GLOG_MAX_ES);
            u.sh = (int)field(ORLG_GLOG_MAX_ES);
            u.gaps = (int)field(ORLG_GLOG_MAX_ES / 2);
            if (u.gaps > 0 && u.sh == 0) u.sh = 1;   // (gaps lie between used runs: some slot is in use)
            sequential(b, u, E);
            orlg_glog_pack(lg[cnt], u.now, u.br, u.span, u.sh, u.gaps);
            cnt += 1;
            updates += 1;
            const bool is_full = cnt == ORLG_GLOG_CAP;
            if (is_full || i == n - 1 || rnd() % 23 == 0) {   // the log is full / the launch ends / a ticket ends
                replay(a, lg, cnt, cnt + (int)(rnd() % (uint64_t)(ORLG_GLOG_CAP - cnt + 1)), E);
                cnt = 0;   // (the entries stay where they are: stale lanes, as on the device)
                replays += 1;
                full += is_full;
                if (!same(a, b)) {
                    std::printf("MISMATCH trial %d update %d: batched (%a %a %a) sequential (%a %a %a)\n", trial, i, a.thr, a.comp, a.lu, b.thr,
                                b.comp, b.lu);
                    return 1;
                }
            }
        }
    }
    std::printf("graph log: %lld updates in %lld replays (%lld of a full log) agree bit for bit\n", updates, replays, full);
    return 0;
}
