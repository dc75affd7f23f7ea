// variant_names_gn_rules.cpp -- host program of tests/test_gn_rules_args.py, linked against liborlg.so: what variant_names_cut.cpp does
// for the keys of the fewest-cuts window, for the keys of the assignment rules behind the GN-model admission check (csrc/orlg_variants.h
// ORLG_WAVE_GN_ASSIGN_KEY_LIST, ORLG_WAVE_GN_CUT_KEY_LIST; the lookup orlg_pick_gn_rules).  Per word count the library was built for
// and per key: the lookup returns a kernel; the symbol at that address, demangled, spaces and trailing default arguments left out, IS
// the name the host reports for the key; no two keys share a kernel, and none of them is a kernel of the lists any other launch
// reaches; orlg_pick, the lookup of every other launch, still answers these keys with null.  A key of the older lists, a USAGE key
// and a key without ASSIGN have no kernel here.  Launches nothing and calls no HIP function.  Prints "checked N" and exits 0 when
// all of that holds.
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "orlg_variants.h"

static int checked = 0, failures = 0;

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
    if (close == std::string::npos) return "(not a template instantiation: " + s + ")";
    s.erase(close);
    std::string out;
    for (char c : s)
        if (c != ' ') out += c;
    const std::string def = ",false";
    while (out.size() > def.size() && out.compare(out.size() - def.size(), def.size(), def) == 0) out.erase(out.size() - def.size());
    return out + ">";
}

static void walk(int W, const OrlgWaveKey &key, std::set<const void *> &seen, const char *tail) {
    char want[96];
    ++checked;
    orlg_kernel_name(want, sizeof(want), W, key);
    const void *k = reinterpret_cast<const void *>(orlg_pick_gn_rules(W, key));
    if (!k) { printf("FAIL %s: the lookup returned null\n", want); ++failures; return; }
    const std::string got = symbol_name(k);
    if (got != want) { printf("FAIL %s: the lookup returned %s\n", want, got.c_str()); ++failures; }
    if (!seen.insert(k).second) { printf("FAIL %s: another key returned the same kernel\n", want); ++failures; }
    const std::string w(want);
    if (w.size() < strlen(tail) || w.compare(w.size() - strlen(tail), strlen(tail), tail) != 0) { printf("FAIL %s: not a name of its list\n", want); ++failures; }
    if (!key.GN || !key.ASSIGN || key.USAGE || key.DEFER) { printf("FAIL %s: not a GN x ASSIGN key\n", want); ++failures; }
    if (orlg_pick(W, key)) { printf("FAIL %s: the lookup of the other launches knows the key\n", want); ++failures; }
}

template <typename List>
static void none_here(int W, const List &list, const char *what) {
    for (const OrlgWaveKey &key : list)
        if (orlg_pick_gn_rules(W, key)) { printf("FAIL W=%d: a key of %s has a kernel in the new lookup\n", W, what); ++failures; }
}

int main() {
    char want[96];
#define ORLG_WALK_W(n, ...)                                                                                                   \
    if (orlg_wave_kernel_W##n) {                                                                                              \
        if (!orlg_gnrules_kernel_W##n) { printf("FAIL W=%d: the library has the wave kernels and not these\n", n); ++failures; } \
        std::set<const void *> seen;                                                                                          \
        for (const OrlgWaveKey &key : ORLG_WAVE_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key)));     \
        for (const OrlgWaveKey &key : ORLG_WAVE_GN_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key)));  \
        for (const OrlgWaveKey &key : ORLG_WAVE_CAUSE_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgWaveKey &key : ORLG_WAVE_ASSIGN_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgWaveKey &key : ORLG_WAVE_CUT_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgWaveKey &key : ORLG_WAVE_USAGE_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgGroupKey &key : ORLG_GROUP_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key)));   \
        if (seen.count(nullptr)) { printf("FAIL W=%d: a key of an older list has no kernel\n", n); ++failures; }               \
        for (const OrlgWaveKey &key : ORLG_WAVE_GN_ASSIGN_KEY_LIST) walk(n, key, seen, ",true>");                            \
        for (const OrlgWaveKey &key : ORLG_WAVE_GN_CUT_KEY_LIST) walk(n, key, seen, ",true,true>");                          \
        none_here(n, ORLG_WAVE_KEY_LIST, "ORLG_WAVE_KEYS"); none_here(n, ORLG_WAVE_GN_KEY_LIST, "ORLG_WAVE_GN_KEYS");         \
        none_here(n, ORLG_WAVE_CAUSE_KEY_LIST, "ORLG_WAVE_CAUSE_KEYS"); none_here(n, ORLG_WAVE_ASSIGN_KEY_LIST, "ORLG_WAVE_ASSIGN_KEYS"); \
        none_here(n, ORLG_WAVE_CUT_KEY_LIST, "ORLG_WAVE_CUT_KEYS"); none_here(n, ORLG_WAVE_USAGE_KEY_LIST, "ORLG_WAVE_USAGE_KEYS"); \
        if (orlg_pick_gn_rules(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, true, false, true, false, true})) { printf("FAIL W=%d: USAGE with GN has a kernel\n", n); ++failures; } \
        if (orlg_pick_gn_rules(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, true, false, false, true})) { printf("FAIL W=%d: GN and CUT without ASSIGN has a kernel\n", n); ++failures; } \
        if (orlg_pick_gn_rules(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, true, true, false, true})) { printf("FAIL W=%d: GN x ASSIGN with DEFER has a kernel\n", n); ++failures; } \
        if (orlg_pick_gn_rules(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel_ff), 2, false, true, false, true})) { printf("FAIL W=%d: GN x ASSIGN _ff has a kernel\n", n); ++failures; } \
        if (orlg_pick_gn_rules(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_reset_kernel), 2, false, true, false, true})) { printf("FAIL W=%d: GN x ASSIGN reset has a kernel\n", n); ++failures; } \
    }
    ORLG_FOR_EACH_W(ORLG_WALK_W, )
    if (sizeof(ORLG_WAVE_GN_ASSIGN_KEY_LIST) / sizeof(ORLG_WAVE_GN_ASSIGN_KEY_LIST[0]) != 6) { printf("FAIL GN x ASSIGN keys\n"); ++failures; }
    if (sizeof(ORLG_WAVE_GN_CUT_KEY_LIST) / sizeof(ORLG_WAVE_GN_CUT_KEY_LIST[0]) != 6) { printf("FAIL GN x CUT keys\n"); ++failures; }
    // the older lists keep their length
    if (sizeof(ORLG_WAVE_KEY_LIST) / sizeof(ORLG_WAVE_KEY_LIST[0]) != 11 || sizeof(ORLG_WAVE_GN_KEY_LIST) / sizeof(ORLG_WAVE_GN_KEY_LIST[0]) != 3 ||
        sizeof(ORLG_WAVE_CAUSE_KEY_LIST) / sizeof(ORLG_WAVE_CAUSE_KEY_LIST[0]) != 6 || sizeof(ORLG_WAVE_ASSIGN_KEY_LIST) / sizeof(ORLG_WAVE_ASSIGN_KEY_LIST[0]) != 6 ||
        sizeof(ORLG_WAVE_CUT_KEY_LIST) / sizeof(ORLG_WAVE_CUT_KEY_LIST[0]) != 6 || sizeof(ORLG_WAVE_USAGE_KEY_LIST) / sizeof(ORLG_WAVE_USAGE_KEY_LIST[0]) != 6) {
        printf("FAIL an older key list changed its length\n"); ++failures;
    }
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, true, false, true});
    if (std::string(want) != "orlg_rmsa_kernel<5,2,false,true,false,true>") { printf("FAIL GN x ASSIGN name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 0, false, true, true, true, true});
    if (std::string(want) != "orlg_rmsa_kernel<5,0,false,true,true,true,true>") { printf("FAIL GN x CUT name %s\n", want); ++failures; }
    printf("checked %d\n", checked);
    return failures ? 1 : 0;
}
