// mm_variant_names.cpp -- host program of tests/test_gn_max_margin_args.py, linked against liborlg.so: variant_names.cpp for the keys
// of the max-margin step kernel (csrc/orlg_variants.h ORLG_WAVE_GN_MM_KEYS, lookup orlg_gnmm_kernel_W<n>, orlg_inst_gnmm.hip).  Per word
// count the library was built for and per key: the lookup returns a kernel; the symbol at the returned address, demangled, spaces and
// trailing default arguments left out, IS the name the host would report (orlg_kernel_name); no two keys share a kernel; a key outside
// the list and a W outside the library return null.  Launches nothing and calls no HIP function.  Prints "checked N", exits 0.
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdlib>
#include <set>
#include <string>

#include "orlg_variants.h"

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
    const std::string params = s.substr(close + 1);
    s.erase(close);
    std::string out;
    for (char c : s)
        if (c != ' ') out += c;
    const std::string def = ",false";
    while (out.size() > def.size() && out.compare(out.size() - def.size(), def.size(), def) == 0) out.erase(out.size() - def.size());
    return out + ">" + (params == "(OrlgParams, OrlgMmArgs)" ? "" : " with parameters " + params);
}

int main() {
    int checked = 0, failures = 0;
    char want[96];
#define ORLG_WALK_W(n, ...)                                                                                        \
    if (orlg_gnmm_kernel_W##n) {                                                                                   \
        std::set<const void *> seen;                                                                               \
        for (const OrlgMmKey &key : ORLG_WAVE_GN_MM_KEY_LIST) {                                                    \
            orlg_kernel_name(want, sizeof(want), n, key);                                                          \
            const void *k = reinterpret_cast<const void *>(orlg_pick_gn_mm(n, key));                               \
            ++checked;                                                                                             \
            if (!k) { printf("FAIL %s: the lookup returned null\n", want); ++failures; continue; }                 \
            const std::string got = symbol_name(k);                                                                \
            if (got != want) { printf("FAIL %s: the lookup returned %s\n", want, got.c_str()); ++failures; }       \
            if (!seen.insert(k).second) { printf("FAIL %s: another key returned the same kernel\n", want); ++failures; } \
        }                                                                                                          \
        if (orlg_pick_gn_mm(n, OrlgMmKey{3, false})) { printf("FAIL W=%d: STATS=3 has a kernel\n", n); ++failures; } \
        printf("W=%d %s\n", n, want);                                                                              \
    }
    ORLG_FOR_EACH_W(ORLG_WALK_W, )
    if (orlg_pick_gn_mm(7, ORLG_WAVE_GN_MM_KEY_LIST[0])) { printf("FAIL: W=7 has a kernel\n"); ++failures; }
    printf("checked %d\n", checked);
    return failures ? 1 : 0;
}
