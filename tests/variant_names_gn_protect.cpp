// variant_names_gn_protect.cpp -- host program of tests/test_variant_names_gn_protect.py, linked against liborlg.so: what
// variant_names_gn_rules.cpp does for the keys of the assignment rules behind the GN-model admission check, for the keys of a handle
// that protects its running lightpaths (csrc/orlg_variants.h ORLG_WAVE_GN_PROTECT_KEY_LIST, ORLG_WAVE_GN_PROTECT_CAUSE_KEY_LIST; the
// lookup orlg_pick_gn_protect).  Per word count the library was built for and per key: the lookup returns a kernel; the symbol at
// that address, demangled, spaces and trailing default arguments left out, IS the name the host reports for the key; no two keys
// share a kernel, and none of them is a kernel of the lists any other launch reaches; the other lookups answer these keys with
// null.  Every key of the older lists has no kernel here and answers as before: its own lookup returns a kernel whose symbol is the
// key's name.  Launches nothing and calls no HIP function.  Prints "checked N" and exits 0 when all of that holds.
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

static void walk(int W, const OrlgWaveKey &key, std::set<const void *> &seen, bool cause) {
    char want[112];
    ++checked;
    orlg_kernel_name(want, sizeof(want), W, key);
    const void *k = reinterpret_cast<const void *>(orlg_pick_gn_protect(W, key));
    if (!k) { printf("FAIL %s: the lookup returned null\n", want); ++failures; return; }
    const std::string got = symbol_name(k);
    if (got != want) { printf("FAIL %s: the lookup returned %s\n", want, got.c_str()); ++failures; }
    if (!seen.insert(k).second) { printf("FAIL %s: another key returned the same kernel\n", want); ++failures; }
    const char *tail = cause ? ",false,true,true,false,false,false,true>" : ",false,true,false,false,false,false,true>";
    const std::string w(want);
    if (w.size() < strlen(tail) || w.compare(w.size() - strlen(tail), strlen(tail), tail) != 0) { printf("FAIL %s: not a name of its list\n", want); ++failures; }
    if (!key.GN || !key.PROTECT || key.ASSIGN || key.CUT || key.USAGE || key.DEFER || key.CAUSE != cause) { printf("FAIL %s: not a GN x PROTECT key\n", want); ++failures; }
    if (orlg_pick(W, key) || orlg_pick_gn_rules(W, key)) { printf("FAIL %s: a lookup of the other launches knows the key\n", want); ++failures; }
}

// a key of an older list: no kernel in the new lookup, and its own lookup answers as before
template <typename List>
static void as_before(int W, const List &list, const char *what, bool gn_rules, std::set<const void *> &seen) {
    char want[112];
    for (const OrlgWaveKey &key : list) {
        ++checked;
        orlg_kernel_name(want, sizeof(want), W, key);
        if (orlg_pick_gn_protect(W, key)) { printf("FAIL W=%d: a key of %s has a kernel in the new lookup\n", W, what); ++failures; }
        const void *k = reinterpret_cast<const void *>(gn_rules ? orlg_pick_gn_rules(W, key) : orlg_pick(W, key));
        if (!k) { printf("FAIL %s (%s): no kernel\n", want, what); ++failures; continue; }
        if (symbol_name(k) != want) { printf("FAIL %s (%s): the lookup returned %s\n", want, what, symbol_name(k).c_str()); ++failures; }
        if (!seen.insert(k).second) { printf("FAIL %s (%s): another key returned the same kernel\n", want, what); ++failures; }
    }
}

int main() {
    char want[112];
#define ORLG_WALK_W(n, ...)                                                                                                     \
    if (orlg_wave_kernel_W##n) {                                                                                                \
        if (!orlg_gnprotect_kernel_W##n) { printf("FAIL W=%d: the library has the wave kernels and not these\n", n); ++failures; } \
        std::set<const void *> seen;                                                                                            \
        as_before(n, ORLG_WAVE_KEY_LIST, "ORLG_WAVE_KEYS", false, seen); as_before(n, ORLG_WAVE_GN_KEY_LIST, "ORLG_WAVE_GN_KEYS", false, seen); \
        as_before(n, ORLG_WAVE_CAUSE_KEY_LIST, "ORLG_WAVE_CAUSE_KEYS", false, seen); as_before(n, ORLG_WAVE_ASSIGN_KEY_LIST, "ORLG_WAVE_ASSIGN_KEYS", false, seen); \
        as_before(n, ORLG_WAVE_CUT_KEY_LIST, "ORLG_WAVE_CUT_KEYS", false, seen); as_before(n, ORLG_WAVE_USAGE_KEY_LIST, "ORLG_WAVE_USAGE_KEYS", false, seen); \
        as_before(n, ORLG_WAVE_GN_ASSIGN_KEY_LIST, "ORLG_WAVE_GN_ASSIGN_KEYS", true, seen); as_before(n, ORLG_WAVE_GN_CUT_KEY_LIST, "ORLG_WAVE_GN_CUT_KEYS", true, seen); \
        for (const OrlgWaveKey &key : ORLG_WAVE_GN_PROTECT_KEY_LIST) walk(n, key, seen, false);                                 \
        for (const OrlgWaveKey &key : ORLG_WAVE_GN_PROTECT_CAUSE_KEY_LIST) walk(n, key, seen, true);                            \
        if (orlg_pick_gn_protect(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, false, false, false, false, false, true})) { printf("FAIL W=%d: PROTECT without GN has a kernel\n", n); ++failures; } \
        if (orlg_pick_gn_protect(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, true, false, true, false, false, true})) { printf("FAIL W=%d: PROTECT with ASSIGN has a kernel\n", n); ++failures; } \
        if (orlg_pick_gn_protect(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, true, true, false, false, false, false, true})) { printf("FAIL W=%d: PROTECT with DEFER has a kernel\n", n); ++failures; } \
        if (orlg_pick_gn_protect(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel_ff), 2, false, true, false, false, false, false, true})) { printf("FAIL W=%d: PROTECT _ff has a kernel\n", n); ++failures; } \
        if (orlg_pick_gn_protect(n, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_reset_kernel), 2, false, true, false, false, false, false, true})) { printf("FAIL W=%d: PROTECT reset has a kernel\n", n); ++failures; } \
    }
    ORLG_FOR_EACH_W(ORLG_WALK_W, )
    if (sizeof(ORLG_WAVE_GN_PROTECT_KEY_LIST) / sizeof(ORLG_WAVE_GN_PROTECT_KEY_LIST[0]) != 3) { printf("FAIL GN x PROTECT keys\n"); ++failures; }
    if (sizeof(ORLG_WAVE_GN_PROTECT_CAUSE_KEY_LIST) / sizeof(ORLG_WAVE_GN_PROTECT_CAUSE_KEY_LIST[0]) != 3) { printf("FAIL GN x PROTECT x CAUSE keys\n"); ++failures; }
    // the older lists keep their length
    if (sizeof(ORLG_WAVE_KEY_LIST) / sizeof(ORLG_WAVE_KEY_LIST[0]) != 11 || sizeof(ORLG_WAVE_GN_KEY_LIST) / sizeof(ORLG_WAVE_GN_KEY_LIST[0]) != 3 ||
        sizeof(ORLG_WAVE_CAUSE_KEY_LIST) / sizeof(ORLG_WAVE_CAUSE_KEY_LIST[0]) != 6 || sizeof(ORLG_WAVE_ASSIGN_KEY_LIST) / sizeof(ORLG_WAVE_ASSIGN_KEY_LIST[0]) != 6 ||
        sizeof(ORLG_WAVE_CUT_KEY_LIST) / sizeof(ORLG_WAVE_CUT_KEY_LIST[0]) != 6 || sizeof(ORLG_WAVE_USAGE_KEY_LIST) / sizeof(ORLG_WAVE_USAGE_KEY_LIST[0]) != 6 ||
        sizeof(ORLG_WAVE_GN_ASSIGN_KEY_LIST) / sizeof(ORLG_WAVE_GN_ASSIGN_KEY_LIST[0]) != 6 || sizeof(ORLG_WAVE_GN_CUT_KEY_LIST) / sizeof(ORLG_WAVE_GN_CUT_KEY_LIST[0]) != 6) {
        printf("FAIL an older key list changed its length\n"); ++failures;
    }
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, true, false, false, false, false, true});
    if (std::string(want) != "orlg_rmsa_kernel<5,2,false,true,false,false,false,false,true>") { printf("FAIL GN x PROTECT name %s\n", want); ++failures; }
    orlg_kernel_name(want, sizeof(want), 5, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), 2, false, true});
    if (std::string(want) != "orlg_rmsa_kernel<5,2,false,true>") { printf("FAIL the gated name changed: %s\n", want); ++failures; }
    printf("checked %d\n", checked);
    return failures ? 1 : 0;
}
