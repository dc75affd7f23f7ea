// variant_names.cpp -- host program of tests/test_variant_names.py, linked against liborlg.so.  Walks every legal key of every
// kernel family (csrc/orlg_variants.h) at every word count the library was built for and requires, per key: the lookup returns a
// kernel; the symbol at the returned address, demangled, spaces and trailing default arguments left out, IS the name the host
// would report for that key (orlg_kernel_name); no two keys of a family share a kernel.  Keys outside the list return null.
// Launches nothing and calls no HIP function.  Prints "checked N" and exits 0 when all of that holds.
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "orlg_variants.h"

static int checked = 0, failures = 0;

// "void orlg_phy_kernel<5, false, true, -1, false, false>(OrlgPhyParams)" -> "orlg_phy_kernel<5,false,true,-1>": every defaulted
// template parameter of the kernels is a bool whose default is false, and the parameter before the first of them is an int
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
    s.erase(close);   // "name<args"
    std::string out;
    for (char c : s)
        if (c != ' ') out += c;
    const std::string def = ",false";
    while (out.size() > def.size() && out.compare(out.size() - def.size(), def.size(), def) == 0) out.erase(out.size() - def.size());
    return out + ">";
}

static void check(const void *kernel, const char *want, std::set<const void *> *seen) {
    ++checked;
    if (!kernel) { printf("FAIL %s: the lookup returned null\n", want); ++failures; return; }
    const std::string got = symbol_name(kernel);
    if (got != want) { printf("FAIL %s: the lookup returned %s\n", want, got.c_str()); ++failures; }
    if (!seen->insert(kernel).second) { printf("FAIL %s: another key of the family returned the same kernel\n", want); ++failures; }
}

template <typename Key, size_t N>
static void walk(int W, const Key (&list)[N], std::set<const void *> *seen) {
    char want[96];
    for (const Key &key : list) {
        orlg_kernel_name(want, sizeof(want), W, key);
        check(reinterpret_cast<const void *>(orlg_pick(W, key)), want, seen);
    }
}

template <typename Key>
static void absent(int W, const Key &key, const char *what) {
    if (orlg_pick(W, key)) { printf("FAIL W=%d: %s is not in the list and has a kernel\n", W, what); ++failures; }
}

int main() {
    char want[96];
#define ORLG_WALK_W(n, ...)                                                                                                   \
    if (orlg_wave_kernel_W##n) {                                                                                              \
        std::set<const void *> wave, group, one;                                                                              \
        walk(n, ORLG_WAVE_KEY_LIST, &wave);                                                                                   \
        walk(n, ORLG_GROUP_KEY_LIST, &group);                                                                                 \
        snprintf(want, sizeof(want), "orlg_path_masks_kernel<%d>", n);                                                        \
        check(reinterpret_cast<const void *>(orlg_pick_masks(n)), want, &one);                                                \
        snprintf(want, sizeof(want), "orlg_deeprmsa_obs_kernel<%d>", n);                                                      \
        check(reinterpret_cast<const void *>(orlg_pick_obs(n)), want, &one);                                                  \
        snprintf(want, sizeof(want), "orlg_action_masks_kernel<%d>", n);                                                      \
        check(reinterpret_cast<const void *>(orlg_pick_action_masks(n)), want, &one);                                         \
        absent(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 1, true}, "orlg_rmsa_kernel with STATS=1, DEFER");          \
        absent(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_reset_kernel), 2, true}, "orlg_rmsa_reset_kernel with DEFER");       \
        absent(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 3, false}, "STATS=3");                                      \
        absent(n, OrlgGroupKey{2, true, true, false, false}, "HBMQ with DEFER");                                              \
        absent(n, OrlgGroupKey{1, false, true, false, false}, "DEFER with STATS=1");                                          \
        absent(n, OrlgGroupKey{0, false, false, true, true}, "TRAFFIC with TRACE");                                           \
    }
    ORLG_FOR_EACH_W(ORLG_WALK_W, )
#define ORLG_WALK_PHY_W(n, ...)                                                                                               \
    if (orlg_phy_kernel_W##n) {                                                                                               \
        std::set<const void *> phy;                                                                                           \
        walk(n, ORLG_PHY_KEY_LIST, &phy);                                                                                     \
        for (int trace = 0; trace < 2; trace++) {                                                                             \
            absent(n, OrlgPhyKey{true, false, ORLG_PHY_POLICY_BMFA_CUT, true, trace != 0}, "CONT with DF");                   \
            absent(n, OrlgPhyKey{false, false, 7, false, trace != 0}, "POL=7");                                               \
            absent(n, OrlgPhyKey{false, false, -2, false, trace != 0}, "POL=-2");                                             \
        }                                                                                                                     \
    }
    ORLG_FOR_EACH_PHY_W(ORLG_WALK_PHY_W, )
    absent(7, ORLG_WAVE_KEY_LIST[0], "W=7");
    absent(7, ORLG_GROUP_KEY_LIST[0], "W=7");
    absent(6, ORLG_PHY_KEY_LIST[0], "W=6");
    printf("checked %d\n", checked);
    return failures ? 1 : 0;
}
