// variant_names.cpp -- the host program of tests/host_programs.py, linked against liborlg.so.  Walks every key of every list of
// csrc/orlg_variants.h -- the wave family unit by unit, the max-margin and adaptive-modulation keys, the group kernel's lists, the
// QoT-aware list -- and every single-kernel lookup (ORLG_WAVE_QUERIES, the two audit kernels) at every word count the library was
// built for, and requires, per key: orlg_pick returns a kernel; the symbol at the returned address, demangled, spaces and trailing
// default arguments left out, IS the name the host reports for that key (orlg_kernel_name), with the kernel's parameter list; no two
// keys of a family share a kernel; the unit that holds the key's list answers it with the same kernel, and every other unit with
// null.  Keys outside the lists return null, and the names the older launches report stay spelled as they were.  Launches nothing
// and calls no HIP function.  Prints "list <name> <keys walked>" per list and "checked N", and exits 0 when all of that holds.
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "orlg_variants.h"

static int checked = 0, failures = 0;
#define FAIL(...) do { printf("FAIL " __VA_ARGS__); printf("\n"); ++failures; } while (0)

// "void orlg_phy_kernel<5, false, true, -1, false, false>(OrlgPhyParams)" -> "orlg_phy_kernel<5,false,true,-1>(OrlgPhyParams)": every
// defaulted template parameter of the kernels is a bool whose default is false, and the parameter before the first of them is an int
static std::string symbol_name(const void *kernel) {
    Dl_info info;
    if (!dladdr(kernel, &info) || !info.dli_sname || info.dli_saddr != kernel) return "(no symbol at this address)";
    int status = 0;
    char *dem = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
    if (status != 0 || !dem) return std::string("(not demangled: ") + info.dli_sname + ")";
    std::string s(dem);
    free(dem);
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    const size_t close = s.rfind(">(");
    if (close == std::string::npos) return s;   // (no template: the audit's kernels)
    const std::string params = s.substr(close + 1);
    s.erase(close);
    std::string out;
    for (char c : s)
        if (c != ' ') out += c;
    const std::string def = ",false";
    while (out.size() > def.size() && out.compare(out.size() - def.size(), def.size(), def) == 0) out.erase(out.size() - def.size());
    return out + ">" + params;
}

static bool ends_with(const std::string &s, const char *tail) { return s.size() >= strlen(tail) && s.compare(s.size() - strlen(tail), strlen(tail), tail) == 0; }

// one kernel behind a lookup: there is one, its symbol is `want` and its parameter list begins with `params` (the whole list for the
// step kernels), and no other key of the family has it
static void check(const void *kernel, const std::string &want, const char *params, std::set<const void *> *seen) {
    ++checked;
    if (!kernel) { FAIL("%s: the lookup returned null", want.c_str()); return; }
    const std::string got = symbol_name(kernel);
    const std::string head = want + params;
    if (got.compare(0, head.size(), head) != 0) FAIL("%s%s: the lookup returned %s", want.c_str(), params, got.c_str());
    if (!seen->insert(kernel).second) FAIL("%s: another key of the family returned the same kernel", want.c_str());
}

// a list: every key through orlg_pick; `tail`: what the names of the list end with (the flags the list turns on)
template <typename Key, size_t N>
static void walk(const char *list, int W, const Key (&keys)[N], const char *params, const char *tail, std::set<const void *> *seen, int *count) {
    char want[112];
    for (const Key &key : keys) {
        orlg_kernel_name(want, sizeof(want), W, key);
        check(reinterpret_cast<const void *>(orlg_pick(W, key)), want, params, seen);
        if (!ends_with(want, tail)) FAIL("%s: not a name of %s (%s)", want, list, tail);
        ++*count;
    }
}
template <typename Key>
static void absent(int W, const Key &key, const char *what) {
    if (orlg_pick(W, key)) FAIL("W=%d: %s is in no list and has a kernel", W, what);
}
template <typename Key>
static void named(const Key &key, const char *want) {
    char got[112];
    orlg_kernel_name(got, sizeof(got), 5, key);
    if (strcmp(got, want) != 0) FAIL("the name %s is now %s", want, got);
}

// the units of the wave family: their exported lookup at a word count (null: not built) and their keys
typedef orlg_rmsa_kernel_t (*wave_unit_t)(OrlgWaveKey);
struct WaveUnit { const char *name; wave_unit_t (*at)(int W); const OrlgWaveKey *keys; size_t n; };
#define UNIT_CASE(n, lookup) case n: return lookup##n;
#define UNIT(lookup, KEYS)                                                                                          \
    static const OrlgWaveKey lookup##_keys[] = {KEYS(ORLG_WAVE_KEY_ENTRY)};                                         \
    static wave_unit_t lookup##_at(int W) { switch (W) { ORLG_FOR_EACH_W(UNIT_CASE, lookup) default: return nullptr; } }
ORLG_WAVE_UNITS(UNIT)
#undef UNIT
#define UNIT(lookup, KEYS) {#lookup, lookup##_at, lookup##_keys, sizeof(lookup##_keys) / sizeof(OrlgWaveKey)},
static const WaveUnit UNITS[] = {ORLG_WAVE_UNITS(UNIT)};
#undef UNIT

// every key of the family against every unit: the owner answers with orlg_pick's kernel, the others with null
static void units_answer_their_own(int W) {
    for (const OrlgWaveKey &key : ORLG_WAVE_ALL_KEY_LIST)
        for (const WaveUnit &u : UNITS) {
            bool own = false;
            for (size_t i = 0; i < u.n; i++) own = own || u.keys[i] == key;
            wave_unit_t at = u.at(W);
            if (!at) { FAIL("W=%d: the library has the wave kernels and not %s", W, u.name); continue; }
            if (at(key) != (own ? orlg_pick(W, key) : nullptr)) FAIL("W=%d: %s answers a key %s", W, u.name, own ? "of its own lists not as orlg_pick does" : "of another unit");
        }
}

#define K(name) ORLG_WAVE_KERNEL(orlg_rmsa_##name)
static void wave_absent(int W) {
    const bool t = true, f = false;
    const struct { OrlgWaveKey key; const char *what; } probes[] = {
        {{K(kernel), 1, t}, "DEFER with STATS=1"}, {{K(reset_kernel), 2, t}, "reset with DEFER"}, {{K(kernel), 3, f}, "STATS=3"},
        {{K(kernel), 2, t, t}, "GN with DEFER"}, {{K(kernel_ff), 2, f, t}, "GN _ff"}, {{K(reset_kernel), 2, f, t}, "GN reset"},
        {{K(kernel), 2, t, f, t}, "CAUSE with DEFER"}, {{K(kernel_ff), 2, f, f, t}, "CAUSE _ff"}, {{K(reset_kernel), 2, f, f, t}, "CAUSE reset"},
        {{K(kernel), 2, t, f, f, t}, "ASSIGN with DEFER"}, {{K(kernel_ff), 2, f, f, f, t}, "ASSIGN _ff"}, {{K(reset_kernel), 2, f, f, f, t}, "ASSIGN reset"},
        {{K(kernel), 2, f, f, f, f, t}, "CUT without ASSIGN"}, {{K(kernel), 2, t, f, f, t, t}, "CUT with DEFER"}, {{K(kernel_ff), 2, f, f, f, t, t}, "CUT _ff"},
        {{K(reset_kernel), 2, f, f, f, t, t}, "CUT reset"},
        {{K(kernel), 2, f, f, f, f, f, t}, "USAGE without ASSIGN"}, {{K(kernel), 2, t, f, f, t, f, t}, "USAGE with DEFER"}, {{K(kernel), 2, f, t, f, t, f, t}, "USAGE with GN"},
        {{K(kernel_ff), 2, f, f, f, t, f, t}, "USAGE _ff"}, {{K(kernel), 2, f, f, f, t, t, t}, "USAGE with CUT"},
        {{K(kernel), 2, f, t, f, f, t}, "GN and CUT without ASSIGN"}, {{K(kernel), 2, t, t, f, t}, "GN x ASSIGN with DEFER"}, {{K(kernel_ff), 2, f, t, f, t}, "GN x ASSIGN _ff"},
        {{K(reset_kernel), 2, f, t, f, t}, "GN x ASSIGN reset"},
        {{K(kernel), 2, f, f, f, f, f, f, t}, "PROTECT without GN"}, {{K(kernel), 2, f, t, f, t, f, f, t}, "PROTECT with ASSIGN"}, {{K(kernel), 2, t, t, f, f, f, f, t}, "PROTECT with DEFER"},
        {{K(kernel_ff), 2, f, t, f, f, f, f, t}, "PROTECT _ff"}, {{K(reset_kernel), 2, f, t, f, f, f, f, t}, "PROTECT reset"}};
    for (const auto &p : probes) {
        absent(W, p.key, p.what);
        for (const WaveUnit &u : UNITS)
            if (u.at(W) && u.at(W)(p.key)) FAIL("W=%d: %s has a kernel in %s", W, p.what, u.name);
    }
    const struct { OrlgGroupKey key; const char *what; } group[] = {
        {{2, t, t, f, f}, "HBMQ with DEFER"}, {{1, f, t, f, f}, "DEFER with STATS=1"}, {{0, f, f, t, t}, "TRAFFIC with TRACE"},
        {{2, t, f, f, f, t}, "CAUSE with HBMQ"}, {{2, f, t, f, f, t}, "group CAUSE with DEFER"},
        {{2, t, f, f, f, f, t}, "ASSIGN with HBMQ"}, {{2, f, t, f, f, f, t}, "group ASSIGN with DEFER"},
        {{2, f, f, f, f, f, f, t}, "group CUT without ASSIGN"}, {{2, t, f, f, f, f, t, t}, "CUT with HBMQ"}, {{2, f, t, f, f, f, t, t}, "group CUT with DEFER"},
        {{2, f, f, f, f, f, f, f, t}, "group USAGE without ASSIGN"}, {{2, t, f, f, f, f, t, f, t}, "USAGE with HBMQ"}, {{2, f, t, f, f, f, t, f, t}, "group USAGE with DEFER"}};
    for (const auto &p : group) absent(W, p.key, p.what);
    absent(W, OrlgMmKey{3, false}, "orlg_rmsa_mm_kernel with STATS=3");
    absent(W, OrlgAmKey{3}, "orlg_rmsa_am_kernel with STATS=3");
}

int main() {
    char want[112];
    int wave[10] = {}, mm = 0, am = 0, group[5] = {}, phy = 0, queries = 0;
#define QUERY(pick, type, lookup, kernel)                                 \
    snprintf(want, sizeof(want), #kernel "<%d>", W);                      \
    check(reinterpret_cast<const void *>(pick(W)), want, "(OrlgParams", &one);       \
    if (pick(7)) FAIL(#pick ": W=7 has a kernel");                        \
    ++queries;
#define WALK_W(n, ...)                                                                                                         \
    if (orlg_wave_kernel_W##n) {                                                                                               \
        const int W = n;                                                                                                       \
        std::set<const void *> w, g, one;   /* the wave kernels of all three key types are one family: rmsa_body */          \
        const char *P = "(OrlgParams)";                                                                                        \
        walk("ORLG_WAVE_KEYS", W, ORLG_WAVE_KEY_LIST, P, "", &w, &wave[0]);                                                    \
        walk("ORLG_WAVE_GN_KEYS", W, ORLG_WAVE_GN_KEY_LIST, P, ",false,true>", &w, &wave[1]);                                  \
        walk("ORLG_WAVE_CAUSE_KEYS", W, ORLG_WAVE_CAUSE_KEY_LIST, P, ",true>", &w, &wave[2]);                                  \
        walk("ORLG_WAVE_ASSIGN_KEYS", W, ORLG_WAVE_ASSIGN_KEY_LIST, P, ",true>", &w, &wave[3]);                                \
        walk("ORLG_WAVE_CUT_KEYS", W, ORLG_WAVE_CUT_KEY_LIST, P, ",true,true>", &w, &wave[4]);                                 \
        walk("ORLG_WAVE_USAGE_KEYS", W, ORLG_WAVE_USAGE_KEY_LIST, P, ",true,false,true>", &w, &wave[5]);                       \
        walk("ORLG_WAVE_GN_ASSIGN_KEYS", W, ORLG_WAVE_GN_ASSIGN_KEY_LIST, P, ",true>", &w, &wave[6]);                          \
        walk("ORLG_WAVE_GN_CUT_KEYS", W, ORLG_WAVE_GN_CUT_KEY_LIST, P, ",true,true>", &w, &wave[7]);                           \
        walk("ORLG_WAVE_GN_PROTECT_KEYS", W, ORLG_WAVE_GN_PROTECT_KEY_LIST, P, ",false,true,false,false,false,false,true>", &w, &wave[8]); \
        walk("ORLG_WAVE_GN_PROTECT_CAUSE_KEYS", W, ORLG_WAVE_GN_PROTECT_CAUSE_KEY_LIST, P, ",false,true,true,false,false,false,true>", &w, &wave[9]); \
        walk("ORLG_WAVE_GN_MM_KEYS", W, ORLG_WAVE_GN_MM_KEY_LIST, "(OrlgParams, OrlgMmArgs)", "", &w, &mm);                    \
        walk("ORLG_WAVE_GN_AM_KEYS", W, ORLG_WAVE_GN_AM_KEY_LIST, "(OrlgParams, OrlgAmArgs)", "", &w, &am);                    \
        for (const OrlgMmKey &key : ORLG_WAVE_GN_MM_KEY_LIST)                                                                  \
            if (!orlg_gnmm_kernel_W##n || orlg_gnmm_kernel_W##n(key) != orlg_pick(W, key)) FAIL("W=%d: orlg_pick and the max-margin unit differ", W); \
        for (const OrlgAmKey &key : ORLG_WAVE_GN_AM_KEY_LIST)                                                                  \
            if (!orlg_gnam_kernel_W##n || orlg_gnam_kernel_W##n(key) != orlg_pick(W, key)) FAIL("W=%d: orlg_pick and the adaptive unit differ", W); \
        orlg_kernel_name(want, sizeof(want), W, ORLG_WAVE_GN_MM_KEY_LIST[5]);   /* (the lists' order: their last keys) */       \
        printf("W=%d %s", W, want);                                                                                            \
        orlg_kernel_name(want, sizeof(want), W, ORLG_WAVE_GN_AM_KEY_LIST[2]);                                                  \
        printf(" %s\n", want);                                                                                                 \
        units_answer_their_own(W);                                                                                             \
        walk("ORLG_GROUP_KEYS", W, ORLG_GROUP_KEY_LIST, P, "", &g, &group[0]);                                                 \
        walk("ORLG_GROUP_CAUSE_KEYS", W, ORLG_GROUP_CAUSE_KEY_LIST, P, ",true>", &g, &group[1]);                               \
        walk("ORLG_GROUP_ASSIGN_KEYS", W, ORLG_GROUP_ASSIGN_KEY_LIST, P, ",true>", &g, &group[2]);                             \
        walk("ORLG_GROUP_CUT_KEYS", W, ORLG_GROUP_CUT_KEY_LIST, P, ",true,true>", &g, &group[3]);                              \
        walk("ORLG_GROUP_USAGE_KEYS", W, ORLG_GROUP_USAGE_KEY_LIST, P, ",true,false,true>", &g, &group[4]);                    \
        for (const OrlgGroupKey &key : ORLG_GROUP_ALL_KEY_LIST)                                                                \
            if (orlg_group_kernel_W##n(key) != orlg_pick(W, key)) FAIL("W=%d: orlg_pick and the group unit differ", W);        \
        ORLG_WAVE_QUERIES(QUERY)                                                                                               \
        wave_absent(W);                                                                                                        \
    }
    ORLG_FOR_EACH_W(WALK_W, )
#define WALK_PHY_W(n, ...)                                                                                                     \
    if (orlg_phy_kernel_W##n) {                                                                                                \
        std::set<const void *> p;                                                                                              \
        walk("ORLG_PHY_KEYS", n, ORLG_PHY_KEY_LIST, "(OrlgPhyParams)", "", &p, &phy);                                          \
        for (int trace = 0; trace < 2; trace++) {                                                                              \
            absent(n, OrlgPhyKey{true, false, ORLG_PHY_POLICY_BMFA_CUT, true, trace != 0}, "CONT with DF");                    \
            absent(n, OrlgPhyKey{false, false, 7, false, trace != 0}, "POL=7");                                                \
            absent(n, OrlgPhyKey{false, false, -2, false, trace != 0}, "POL=-2");                                              \
        }                                                                                                                      \
    }
    ORLG_FOR_EACH_PHY_W(WALK_PHY_W, )
    // the audit's two kernels know no word count
    std::set<const void *> audit;
    for (const void *k : {reinterpret_cast<const void *>(orlg_gn_audit_kernel_lookup()), reinterpret_cast<const void *>(orlg_running_services_kernel_lookup())}) {
        ++checked; ++queries;
        const std::string got = k ? symbol_name(k) : "null";
        const char *name = audit.empty() ? "orlg_gn_audit_kernel(" : "orlg_running_services_kernel(";
        if (!k || got.compare(0, strlen(name), name) != 0 || !audit.insert(k).second) FAIL("%s...): the lookup returned %s", name, got.c_str());
    }
    // a word count the library does not hold
    absent(7, ORLG_WAVE_KEY_LIST[0], "W=7");
    for (const OrlgWaveKey &key : ORLG_WAVE_ALL_KEY_LIST) absent(7, key, "W=7");
    absent(7, ORLG_GROUP_KEY_LIST[0], "W=7");
    absent(7, ORLG_WAVE_GN_MM_KEY_LIST[0], "W=7");
    absent(7, ORLG_WAVE_GN_AM_KEY_LIST[0], "W=7");
    absent(6, ORLG_PHY_KEY_LIST[0], "W=6");
    // the names the launches have always reported: a flag at its default does not show, whatever flags came after it
    const bool t = true, f = false;
    named(OrlgWaveKey{K(kernel), 2, f}, "orlg_rmsa_kernel<5,2>");
    named(OrlgWaveKey{K(kernel), 2, t}, "orlg_rmsa_kernel<5,2,true>");
    named(OrlgWaveKey{K(kernel), 2, f, t}, "orlg_rmsa_kernel<5,2,false,true>");
    named(OrlgWaveKey{K(kernel), 2, f, f, t}, "orlg_rmsa_kernel<5,2,false,false,true>");
    named(OrlgWaveKey{K(kernel), 0, f, f, f, t}, "orlg_rmsa_kernel<5,0,false,false,false,true>");
    named(OrlgWaveKey{K(kernel), 0, f, f, t, t, t}, "orlg_rmsa_kernel<5,0,false,false,true,true,true>");
    named(OrlgWaveKey{K(kernel), 0, f, f, t, t, f, t}, "orlg_rmsa_kernel<5,0,false,false,true,true,false,true>");
    named(OrlgWaveKey{K(kernel), 2, f, t, f, t}, "orlg_rmsa_kernel<5,2,false,true,false,true>");
    named(OrlgWaveKey{K(kernel), 0, f, t, t, t, t}, "orlg_rmsa_kernel<5,0,false,true,true,true,true>");
    named(OrlgWaveKey{K(kernel), 2, f, t, f, f, f, f, t}, "orlg_rmsa_kernel<5,2,false,true,false,false,false,false,true>");
    named(OrlgMmKey{0, t}, "orlg_rmsa_mm_kernel<5,0,true>");
    named(OrlgAmKey{1}, "orlg_rmsa_am_kernel<5,1>");
    named(OrlgGroupKey{2, f, t, f, f}, "orlg_rmsa_group_kernel<5,2,false,true>");
    named(OrlgGroupKey{1, f, f, t, f, t}, "orlg_rmsa_group_kernel<5,1,false,false,true,false,true>");
    named(OrlgGroupKey{1, f, f, f, t, f, t}, "orlg_rmsa_group_kernel<5,1,false,false,false,true,false,true>");
    named(OrlgGroupKey{1, f, f, f, t, f, t, t}, "orlg_rmsa_group_kernel<5,1,false,false,false,true,false,true,true>");
    named(OrlgGroupKey{1, f, f, f, t, f, t, f, t}, "orlg_rmsa_group_kernel<5,1,false,false,false,true,false,true,false,true>");

    const char *const wave_lists[10] = {"ORLG_WAVE_KEYS", "ORLG_WAVE_GN_KEYS", "ORLG_WAVE_CAUSE_KEYS", "ORLG_WAVE_ASSIGN_KEYS", "ORLG_WAVE_CUT_KEYS",
                                        "ORLG_WAVE_USAGE_KEYS", "ORLG_WAVE_GN_ASSIGN_KEYS", "ORLG_WAVE_GN_CUT_KEYS", "ORLG_WAVE_GN_PROTECT_KEYS",
                                        "ORLG_WAVE_GN_PROTECT_CAUSE_KEYS"};
    const char *const group_lists[5] = {"ORLG_GROUP_KEYS", "ORLG_GROUP_CAUSE_KEYS", "ORLG_GROUP_ASSIGN_KEYS", "ORLG_GROUP_CUT_KEYS", "ORLG_GROUP_USAGE_KEYS"};
    for (int i = 0; i < 10; i++) printf("list %s %d\n", wave_lists[i], wave[i]);
    printf("list ORLG_WAVE_GN_MM_KEYS %d\nlist ORLG_WAVE_GN_AM_KEYS %d\n", mm, am);
    for (int i = 0; i < 5; i++) printf("list %s %d\n", group_lists[i], group[i]);
    printf("list ORLG_PHY_KEYS %d\nlist ORLG_WAVE_QUERIES %d\n", phy, queries);
    printf("checked %d\n", checked);
    return failures ? 1 : 0;
}
