// variant_names_window.cpp -- host program of tests/test_window_rules.py, linked against liborlg.so: what variant_names_cut.cpp does
// for the keys of the fewest-cuts window, for the keys of the rule MOST_USED and the route BEST_WINDOW (csrc/orlg_variants.h
// ORLG_WAVE_USAGE_KEY_LIST, ORLG_GROUP_USAGE_KEY_LIST).  Per word count the library was built for and per key: the lookup returns a
// kernel; the symbol at that address, demangled, spaces and trailing default arguments left out, IS the name the host reports for
// the key; no two keys share a kernel, and none of them is a kernel of the lists any other launch reaches, the ASSIGN and CUT lists
// among them.  A USAGE key without ASSIGN, with CUT, or of a kind that has no rules (_ff, DEFER, HBMQ, a gate) returns null.  Launches nothing and calls no HIP function.  Prints
// "checked N" and exits 0 when all of that holds.
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

template <typename Key>
static void walk(int W, const Key &key, std::set<const void *> &seen, const char *tail) {
    char want[96];
    ++checked;
    orlg_kernel_name(want, sizeof(want), W, key);
    const void *k = reinterpret_cast<const void *>(orlg_pick(W, key));
    if (!k) { printf("FAIL %s: the lookup returned null\n", want); ++failures; return; }
    const std::string got = symbol_name(k);
    if (got != want) { printf("FAIL %s: the lookup returned %s\n", want, got.c_str()); ++failures; }
    if (!seen.insert(k).second) { printf("FAIL %s: another key returned the same kernel\n", want); ++failures; }
    const std::string w(want);
    if (w.size() < strlen(tail) || w.compare(w.size() - strlen(tail), strlen(tail), tail) != 0) { printf("FAIL %s: not a USAGE name\n", want); ++failures; }
}

int main() {
    char want[96];
#define ORLG_WALK_W(n, ...)                                                                                                   \
    if (orlg_wave_kernel_W##n) {                                                                                              \
        std::set<const void *> seen;                                                                                          \
        for (const OrlgWaveKey &key : ORLG_WAVE_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key)));     \
        for (const OrlgWaveKey &key : ORLG_WAVE_GN_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key)));  \
        for (const OrlgWaveKey &key : ORLG_WAVE_CAUSE_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgGroupKey &key : ORLG_GROUP_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key)));   \
        for (const OrlgGroupKey &key : ORLG_GROUP_CAUSE_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgWaveKey &key : ORLG_WAVE_ASSIGN_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgGroupKey &key : ORLG_GROUP_ASSIGN_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgWaveKey &key : ORLG_WAVE_CUT_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgGroupKey &key : ORLG_GROUP_CUT_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key))); \
        for (const OrlgWaveKey &key : ORLG_WAVE_USAGE_KEY_LIST) walk(n, key, seen, ",true,false,true>");                    \
        for (const OrlgGroupKey &key : ORLG_GROUP_USAGE_KEY_LIST) walk(n, key, seen, ",true,false,true>");                  \
        if (orlg_pick(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, false, false, false, false, true})) { printf("FAIL W=%d: USAGE without ASSIGN has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, true, false, false, true, false, true})) { printf("FAIL W=%d: USAGE with DEFER has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, true, false, true, false, true})) { printf("FAIL W=%d: USAGE with GN has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel_ff), 2, false, false, false, true, false, true})) { printf("FAIL W=%d: USAGE _ff has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, false, false, true, true, true})) { printf("FAIL W=%d: USAGE with CUT has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgGroupKey{2, false, false, false, false, false, false, false, true})) { printf("FAIL W=%d: group USAGE without ASSIGN has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgGroupKey{2, true, false, false, false, false, true, false, true})) { printf("FAIL W=%d: USAGE with HBMQ has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgGroupKey{2, false, true, false, false, false, true, false, true})) { printf("FAIL W=%d: group USAGE with DEFER has a kernel\n", n); ++failures; } \
    }
    ORLG_FOR_EACH_W(ORLG_WALK_W, )
    if (sizeof(ORLG_WAVE_USAGE_KEY_LIST) / sizeof(ORLG_WAVE_USAGE_KEY_LIST[0]) != 6) { printf("FAIL wave USAGE keys\n"); ++failures; }
    if (sizeof(ORLG_GROUP_USAGE_KEY_LIST) / sizeof(ORLG_GROUP_USAGE_KEY_LIST[0]) != 18) { printf("FAIL group USAGE keys\n"); ++failures; }
    // the names of the keys without the flag do not change with the USAGE member at its default
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false});
    if (std::string(want) != "orlg_rmsa_kernel<5,2>") { printf("FAIL plain name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 0, false, false, false, true});
    if (std::string(want) != "orlg_rmsa_kernel<5,0,false,false,false,true>") { printf("FAIL assign name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 0, false, false, true, true, true});
    if (std::string(want) != "orlg_rmsa_kernel<5,0,false,false,true,true,true>") { printf("FAIL cut name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgGroupKey{1, false, false, false, true, false, true});
    if (std::string(want) != "orlg_rmsa_group_kernel<5,1,false,false,false,true,false,true>") { printf("FAIL assign group name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgGroupKey{1, false, false, false, true, false, true, true});
    if (std::string(want) != "orlg_rmsa_group_kernel<5,1,false,false,false,true,false,true,true>") { printf("FAIL cut group name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 0, false, false, true, true, false, true});
    if (std::string(want) != "orlg_rmsa_kernel<5,0,false,false,true,true,false,true>") { printf("FAIL usage name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgGroupKey{1, false, false, false, true, false, true, false, true});
    if (std::string(want) != "orlg_rmsa_group_kernel<5,1,false,false,false,true,false,true,false,true>") { printf("FAIL usage group name %s\n", want); ++failures; }
    printf("checked %d\n", checked);
    return failures ? 1 : 0;
}
