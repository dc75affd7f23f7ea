// variant_names_gn.cpp -- host program of tests/test_variant_names_gn.py, linked against liborlg.so: what variant_names.cpp does
// for the lists it walks, for the keys of the GN-model admission check (csrc/orlg_variants.h ORLG_WAVE_GN_KEY_LIST).  Per word
// count the library was built for and per key: the lookup returns a kernel; the symbol at that address, demangled, spaces and
// trailing default arguments left out, IS the name the host reports for the key; no two keys share a kernel, and none of them is
// a kernel of the ungated list.  A gated key that is not legal (DEFER, the _ff kernel) returns null.  Launches nothing and calls
// no HIP function.  Prints "checked N" and exits 0 when all of that holds.
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdlib>
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

int main() {
    char want[96];
#define ORLG_WALK_W(n, ...)                                                                                                   \
    if (orlg_wave_kernel_W##n) {                                                                                              \
        std::set<const void *> seen;                                                                                          \
        for (const OrlgWaveKey &key : ORLG_WAVE_KEY_LIST) seen.insert(reinterpret_cast<const void *>(orlg_pick(n, key)));     \
        for (const OrlgWaveKey &key : ORLG_WAVE_GN_KEY_LIST) {                                                                \
            ++checked;                                                                                                        \
            orlg_kernel_name(want, sizeof(want), n, key);                                                                     \
            const void *k = reinterpret_cast<const void *>(orlg_pick(n, key));                                                \
            if (!k) { printf("FAIL %s: the lookup returned null\n", want); ++failures; continue; }                            \
            const std::string got = symbol_name(k);                                                                           \
            if (got != want) { printf("FAIL %s: the lookup returned %s\n", want, got.c_str()); ++failures; }                  \
            if (!seen.insert(k).second) { printf("FAIL %s: another key returned the same kernel\n", want); ++failures; }      \
            if (std::string(want).find(",false,true>") == std::string::npos) { printf("FAIL %s: not a GN name\n", want); ++failures; } \
        }                                                                                                                     \
        if (orlg_pick(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, true, true})) { printf("FAIL W=%d: GN with DEFER has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel_ff), 2, false, true})) { printf("FAIL W=%d: GN _ff has a kernel\n", n); ++failures; } \
        if (orlg_pick(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_reset_kernel), 2, false, true})) { printf("FAIL W=%d: GN reset has a kernel\n", n); ++failures; } \
    }
    ORLG_FOR_EACH_W(ORLG_WALK_W, )
    // the names of the ungated keys do not change with the GN member at its default
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false});
    if (std::string(want) != "orlg_rmsa_kernel<5,2>") { printf("FAIL ungated name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, true});
    if (std::string(want) != "orlg_rmsa_kernel<5,2,true>") { printf("FAIL deferred name %s\n", want); ++failures; }
    printf("checked %d\n", checked);
    return failures ? 1 : 0;
}
