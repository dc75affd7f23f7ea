// orlg_variants.h -- which instantiations of the step kernels liborlg.so holds, written once.  Per kernel family: a key (the
// template parameters after W, under the kernels' own names), the list of the legal keys, and from them the lookups the
// instantiation units export (orlg_inst_*.hip expand the list), the name a launch reports (last_kernel) and a dense index.
// Plain C++: no HIP, no device code -- orlg_host.h includes it, and so can a host program that only links the library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/orlg.h"   // ORLG_PHY_POLICY_*

// ---------------------------------------------------------------------------------------- keys
// wave-per-environment kernels (orlg_kernels.hip): template <int W, int STATS, bool DEFER = false, bool GN = false, bool CAUSE = false,
// bool ASSIGN = false, bool CUT = false>; the reset kernel has no DEFER, and only orlg_rmsa_kernel has GN (the GN-model admission
// check, orlg_rmsa_gn.h), CAUSE (the blocking cause of every step, orlg_block_cause.h), ASSIGN (the spectrum-assignment rules beyond
// the reference's first fit, orlg_assign.h), CUT (ASSIGN with the fewest-cuts window in the rules' place, orlg_cut.h) and, after it,
// USAGE (ASSIGN with the rule MOST_USED and the route BEST_WINDOW, orlg_usage.h) and, last, PROTECT (GN with the check of the
// running lightpaths, orlg_rmsa_gn_protect.h)
#define ORLG_WAVE_KERNELS(X) X(orlg_rmsa_kernel) X(orlg_rmsa_kernel_ff) X(orlg_rmsa_reset_kernel)
#define ORLG_WAVE_KERNEL(name) ORLG_IS_##name
enum OrlgWaveKernel {
#define X(name) ORLG_WAVE_KERNEL(name),
    ORLG_WAVE_KERNELS(X)
#undef X
};
struct OrlgWaveKey { OrlgWaveKernel kernel; int STATS; bool DEFER; bool GN = false; bool CAUSE = false; bool ASSIGN = false; bool CUT = false; bool USAGE = false; bool PROTECT = false; };
// orlg_rmsa_group_kernel (orlg_group_kernels.hip)
struct OrlgGroupKey { int STATS; bool HBMQ, DEFER, TRAFFIC, TRACE; bool CAUSE = false; bool ASSIGN = false; bool CUT = false; bool USAGE = false; };
// orlg_phy_kernel (orlg_phy_kernels.hip)
struct OrlgPhyKey { bool DF, GN; int POL; bool CONT, TRACE; };

inline bool operator==(const OrlgWaveKey &a, const OrlgWaveKey &b) { return a.kernel == b.kernel && a.STATS == b.STATS && a.DEFER == b.DEFER && a.GN == b.GN && a.CAUSE == b.CAUSE && a.ASSIGN == b.ASSIGN && a.CUT == b.CUT && a.USAGE == b.USAGE && a.PROTECT == b.PROTECT; }
inline bool operator==(const OrlgGroupKey &a, const OrlgGroupKey &b) {
    return a.STATS == b.STATS && a.HBMQ == b.HBMQ && a.DEFER == b.DEFER && a.TRAFFIC == b.TRAFFIC && a.TRACE == b.TRACE && a.CAUSE == b.CAUSE && a.ASSIGN == b.ASSIGN && a.CUT == b.CUT && a.USAGE == b.USAGE;
}
inline bool operator==(const OrlgPhyKey &a, const OrlgPhyKey &b) {
    return a.DF == b.DF && a.GN == b.GN && a.POL == b.POL && a.CONT == b.CONT && a.TRACE == b.TRACE;
}

// ---------------------------------------------------------------------------------------- the legal keys
// X(kernel, STATS[, DEFER]).  DEFER: full statistics with the links' float64 part deferred (link_replay); _ff: the first-fit
// policies only (k <= 8).  (A list's order is the order of the kernels in the unit's code object: levels 1, 2, 0 as they have
// always lain there, so that a build can be compared with its predecessor byte by byte.)
#define ORLG_WAVE_KEYS(X)                                                                    \
    X(orlg_rmsa_kernel, 1) X(orlg_rmsa_kernel, 2) X(orlg_rmsa_kernel, 0)                     \
    X(orlg_rmsa_kernel_ff, 1) X(orlg_rmsa_kernel_ff, 2) X(orlg_rmsa_kernel_ff, 0)            \
    X(orlg_rmsa_kernel, 2, true) X(orlg_rmsa_kernel_ff, 2, true)                             \
    X(orlg_rmsa_reset_kernel, 1) X(orlg_rmsa_reset_kernel, 2) X(orlg_rmsa_reset_kernel, 0)
// X(kernel, STATS, DEFER, GN): what a handle with a GN-model admission check launches (orlg_set_gn_gate) -- the general step kernel
// with the check, per statistics level; no _ff and no DEFER variant.  A list of its own: ORLG_WAVE_KEYS stays what a handle without
// a gate can reach, in number too (tests/test_variant_names.py counts its lookups); an instantiation unit expands both, these
// last, so that the kernels in front of them lie in the code object where they lay.
#define ORLG_WAVE_GN_KEYS(X) X(orlg_rmsa_kernel, 1, false, true) X(orlg_rmsa_kernel, 2, false, true) X(orlg_rmsa_kernel, 0, false, true)
// X(kernel, STATS, DEFER, GN, CAUSE): what a launch that asks for the blocking cause of its steps runs (orlg_step_diag) -- the general
// step kernel with the classifier, per statistics level, without and with the admission check; no _ff and no DEFER variant
// (optimisations that leave the same state: such a launch does without them).  A list of its own for the reasons above, expanded
// after the GN keys.
#define ORLG_WAVE_CAUSE_KEYS(X)                                                                                             \
    X(orlg_rmsa_kernel, 1, false, false, true) X(orlg_rmsa_kernel, 2, false, false, true) X(orlg_rmsa_kernel, 0, false, false, true) \
    X(orlg_rmsa_kernel, 1, false, true, true) X(orlg_rmsa_kernel, 2, false, true, true) X(orlg_rmsa_kernel, 0, false, true, true)
// X(kernel, STATS, DEFER, GN, CAUSE, ASSIGN): what a launch under an assignment rule other than the reference's first fit runs
// (orlg_step_assign) -- the general step kernel with the rules, per statistics level, without and with the classifier; no gate
// (refused), no _ff and no DEFER variant.  A list of its own for the reasons above, expanded after the CAUSE keys.
#define ORLG_WAVE_ASSIGN_KEYS(X)                                                                                                          \
    X(orlg_rmsa_kernel, 1, false, false, false, true) X(orlg_rmsa_kernel, 2, false, false, false, true) X(orlg_rmsa_kernel, 0, false, false, false, true) \
    X(orlg_rmsa_kernel, 1, false, false, true, true) X(orlg_rmsa_kernel, 2, false, false, true, true) X(orlg_rmsa_kernel, 0, false, false, true, true)
// X(kernel, STATS, DEFER, GN, CAUSE, ASSIGN, CUT): what a launch under the fewest-cuts window runs (orlg_step_min_cut) -- the ASSIGN
// keys again with CUT.  The rule's hop loop, with its cut counters, is not in the ASSIGN instantiations: inside them it cost the
// classic rules of the group kernel 1.5 %.  A list of its own, expanded last.
#define ORLG_WAVE_CUT_KEYS(X)                                                                                                                       \
    X(orlg_rmsa_kernel, 1, false, false, false, true, true) X(orlg_rmsa_kernel, 2, false, false, false, true, true) X(orlg_rmsa_kernel, 0, false, false, false, true, true) \
    X(orlg_rmsa_kernel, 1, false, false, true, true, true) X(orlg_rmsa_kernel, 2, false, false, true, true, true) X(orlg_rmsa_kernel, 0, false, false, true, true, true)
// X(kernel, STATS, DEFER, GN, CAUSE, ASSIGN, CUT, USAGE): what a launch of orlg_step_window under the rule MOST_USED or the route
// BEST_WINDOW runs (orlg_usage.h) -- the ASSIGN keys again with USAGE, for the reason the CUT keys have.  A list of
// its own, expanded last.
#define ORLG_WAVE_USAGE_KEYS(X)                                                                                                                                   \
    X(orlg_rmsa_kernel, 1, false, false, false, true, false, true) X(orlg_rmsa_kernel, 2, false, false, false, true, false, true) X(orlg_rmsa_kernel, 0, false, false, false, true, false, true) \
    X(orlg_rmsa_kernel, 1, false, false, true, true, false, true) X(orlg_rmsa_kernel, 2, false, false, true, true, false, true) X(orlg_rmsa_kernel, 0, false, false, true, true, false, true)
// X(kernel, STATS, DEFER, GN, CAUSE, ASSIGN[, CUT]): what orlg_step_rule_gn launches -- the ASSIGN keys and the CUT
// keys again with GN: an assignment rule, or the fewest-cuts window, whose proposal goes through the admission check.  No USAGE
// (refused).  Lists of their own, and a unit of its own (orlg_inst_gnrules.hip, one object per W, lookup orlg_gnrules_kernel_W<n>):
// the orlg_inst_wave objects hold what they held.
#define ORLG_WAVE_GN_ASSIGN_KEYS(X)                                                                                                    \
    X(orlg_rmsa_kernel, 1, false, true, false, true) X(orlg_rmsa_kernel, 2, false, true, false, true) X(orlg_rmsa_kernel, 0, false, true, false, true) \
    X(orlg_rmsa_kernel, 1, false, true, true, true) X(orlg_rmsa_kernel, 2, false, true, true, true) X(orlg_rmsa_kernel, 0, false, true, true, true)
#define ORLG_WAVE_GN_CUT_KEYS(X)                                                                                                                   \
    X(orlg_rmsa_kernel, 1, false, true, false, true, true) X(orlg_rmsa_kernel, 2, false, true, false, true, true) X(orlg_rmsa_kernel, 0, false, true, false, true, true) \
    X(orlg_rmsa_kernel, 1, false, true, true, true, true) X(orlg_rmsa_kernel, 2, false, true, true, true, true) X(orlg_rmsa_kernel, 0, false, true, true, true, true)
// X(kernel, STATS, DEFER, GN, CAUSE, ASSIGN, CUT, USAGE, PROTECT): what a handle that protects its running lightpaths launches
// (orlg_set_gn_protect) -- the GN keys again with PROTECT, without and with the classifier.  Lists of their own, and a
// unit of its own (orlg_inst_gnprotect.hip, one object per W, lookup orlg_gnprotect_kernel_W<n>): the orlg_inst_wave and
// orlg_inst_gnrules objects hold what they held.
#define ORLG_WAVE_GN_PROTECT_KEYS(X)                                                                                                              \
    X(orlg_rmsa_kernel, 1, false, true, false, false, false, false, true) X(orlg_rmsa_kernel, 2, false, true, false, false, false, false, true) \
    X(orlg_rmsa_kernel, 0, false, true, false, false, false, false, true)
#define ORLG_WAVE_GN_PROTECT_CAUSE_KEYS(X)                                                                                                      \
    X(orlg_rmsa_kernel, 1, false, true, true, false, false, false, true) X(orlg_rmsa_kernel, 2, false, true, true, false, false, false, true) \
    X(orlg_rmsa_kernel, 0, false, true, true, false, false, false, true)

// X(STATS, HBMQ, DEFER, TRAFFIC, TRACE).  Per kind of handle: every statistics level, the same with the release queue left in HBM
// (launches of very few steps), and full statistics with the link updates deferred (long launches).  The kinds: plain, with
// per-environment traffic (OrlgParams::rates), replaying a request trace (OrlgParams::tr_*)
#define ORLG_GROUP_KEYS_OF(X, TRAFFIC, TRACE)                                                                     \
    X(0, false, false, TRAFFIC, TRACE) X(1, false, false, TRAFFIC, TRACE) X(2, false, false, TRAFFIC, TRACE)      \
    X(0, true, false, TRAFFIC, TRACE) X(1, true, false, TRAFFIC, TRACE) X(2, true, false, TRAFFIC, TRACE)         \
    X(2, false, true, TRAFFIC, TRACE)
#define ORLG_GROUP_KEYS(X) ORLG_GROUP_KEYS_OF(X, false, false) ORLG_GROUP_KEYS_OF(X, true, false) ORLG_GROUP_KEYS_OF(X, false, true)
// X(STATS, HBMQ, DEFER, TRAFFIC, TRACE, CAUSE): the launches that ask for the blocking cause -- the plain kind of instantiation
// (queue in LDS, statistics at every step) per statistics level and kind of handle.  HBMQ, DEFER and its lean body are
// optimisations that leave identical state; orlg_group_plan.h keeps a cause launch off them.  A list of its own, expanded last
#define ORLG_GROUP_CAUSE_KEYS_OF(X, TRAFFIC, TRACE) \
    X(0, false, false, TRAFFIC, TRACE, true) X(1, false, false, TRAFFIC, TRACE, true) X(2, false, false, TRAFFIC, TRACE, true)
#define ORLG_GROUP_CAUSE_KEYS(X) \
    ORLG_GROUP_CAUSE_KEYS_OF(X, false, false) ORLG_GROUP_CAUSE_KEYS_OF(X, true, false) ORLG_GROUP_CAUSE_KEYS_OF(X, false, true)
// X(STATS, HBMQ, DEFER, TRAFFIC, TRACE, CAUSE, ASSIGN): the launches under an assignment rule other than the reference's first fit
// -- the plain kind per statistics level and kind of handle, without and with the classifier (orlg_group_plan.h keeps such a
// launch off HBMQ, DEFER and the lean body through ORLG_OUT_ASSIGN_BIT).  A list of its own, expanded after the CAUSE keys
#define ORLG_GROUP_ASSIGN_KEYS_OF(X, TRAFFIC, TRACE, CAUSE) \
    X(0, false, false, TRAFFIC, TRACE, CAUSE, true) X(1, false, false, TRAFFIC, TRACE, CAUSE, true) X(2, false, false, TRAFFIC, TRACE, CAUSE, true)
#define ORLG_GROUP_ASSIGN_KEYS(X)                                                                                                           \
    ORLG_GROUP_ASSIGN_KEYS_OF(X, false, false, false) ORLG_GROUP_ASSIGN_KEYS_OF(X, true, false, false) ORLG_GROUP_ASSIGN_KEYS_OF(X, false, true, false) \
    ORLG_GROUP_ASSIGN_KEYS_OF(X, false, false, true) ORLG_GROUP_ASSIGN_KEYS_OF(X, true, false, true) ORLG_GROUP_ASSIGN_KEYS_OF(X, false, true, true)
// X(STATS, HBMQ, DEFER, TRAFFIC, TRACE, CAUSE, ASSIGN, CUT): the launches under the fewest-cuts window -- the ASSIGN keys again with
// CUT (as ORLG_WAVE_CUT_KEYS).  A list of its own, expanded last
#define ORLG_GROUP_CUT_KEYS_OF(X, TRAFFIC, TRACE, CAUSE) \
    X(0, false, false, TRAFFIC, TRACE, CAUSE, true, true) X(1, false, false, TRAFFIC, TRACE, CAUSE, true, true) X(2, false, false, TRAFFIC, TRACE, CAUSE, true, true)
#define ORLG_GROUP_CUT_KEYS(X)                                                                                                     \
    ORLG_GROUP_CUT_KEYS_OF(X, false, false, false) ORLG_GROUP_CUT_KEYS_OF(X, true, false, false) ORLG_GROUP_CUT_KEYS_OF(X, false, true, false) \
    ORLG_GROUP_CUT_KEYS_OF(X, false, false, true) ORLG_GROUP_CUT_KEYS_OF(X, true, false, true) ORLG_GROUP_CUT_KEYS_OF(X, false, true, true)
// X(STATS, HBMQ, DEFER, TRAFFIC, TRACE, CAUSE, ASSIGN, CUT, USAGE): the launches of orlg_step_window under the rule MOST_USED or the
// route BEST_WINDOW -- the ASSIGN keys again with USAGE (as ORLG_WAVE_USAGE_KEYS).  A list of its own, expanded last
#define ORLG_GROUP_USAGE_KEYS_OF(X, TRAFFIC, TRACE, CAUSE) \
    X(0, false, false, TRAFFIC, TRACE, CAUSE, true, false, true) X(1, false, false, TRAFFIC, TRACE, CAUSE, true, false, true) X(2, false, false, TRAFFIC, TRACE, CAUSE, true, false, true)
#define ORLG_GROUP_USAGE_KEYS(X)                                                                                                         \
    ORLG_GROUP_USAGE_KEYS_OF(X, false, false, false) ORLG_GROUP_USAGE_KEYS_OF(X, true, false, false) ORLG_GROUP_USAGE_KEYS_OF(X, false, true, false) \
    ORLG_GROUP_USAGE_KEYS_OF(X, false, false, true) ORLG_GROUP_USAGE_KEYS_OF(X, true, false, true) ORLG_GROUP_USAGE_KEYS_OF(X, false, true, true)

// X(DF, GN, POL, CONT, TRACE), one instantiation per policy (-1 external actions .. 6).  Discrete bit rates: the step kernel
// proper, + periodic defragmentation, + defragmentation and the GN-model admission check, + the check alone (a handle without
// defrag_period does not carry the defragmentation's registers).  bit_rate_selection="continuous": the step kernel proper and
// + the check (no defragmentation: refused at create time).  TRACE: handles that replay a request trace (OrlgPhyParams::tr_*),
// the same keys again.
#define ORLG_PHY_KEYS_DISCRETE(X, POL, TRACE) \
    X(false, false, POL, false, TRACE) X(true, false, POL, false, TRACE) X(true, true, POL, false, TRACE) X(false, true, POL, false, TRACE)
#define ORLG_PHY_KEYS_CONT(X, POL, TRACE) X(false, false, POL, true, TRACE) X(false, true, POL, true, TRACE)
#ifdef ORLG_PHY_FEW_POLICIES   // (instrumented single-unit builds of tools/: external actions and bmfa, discrete only)
#define ORLG_PHY_KEYS_OF(X, TRACE) \
    ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_EXTERNAL, TRACE) ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_BMFA_CUT, TRACE)
#else
#define ORLG_PHY_KEYS_OF(X, TRACE)                                                                                      \
    ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_EXTERNAL, TRACE) ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_BMFA_CUT, TRACE)    \
    ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_BMFA_RSS_METRIC, TRACE) ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_SAPFF, TRACE) \
    ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_BMFF, TRACE) ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_SAPBM, TRACE)           \
    ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_FAFF, TRACE) ORLG_PHY_KEYS_DISCRETE(X, ORLG_PHY_POLICY_FAFF_RSS, TRACE)        \
    ORLG_PHY_KEYS_CONT(X, ORLG_PHY_POLICY_EXTERNAL, TRACE) ORLG_PHY_KEYS_CONT(X, ORLG_PHY_POLICY_BMFA_CUT, TRACE)            \
    ORLG_PHY_KEYS_CONT(X, ORLG_PHY_POLICY_BMFA_RSS_METRIC, TRACE) ORLG_PHY_KEYS_CONT(X, ORLG_PHY_POLICY_SAPFF, TRACE)        \
    ORLG_PHY_KEYS_CONT(X, ORLG_PHY_POLICY_BMFF, TRACE) ORLG_PHY_KEYS_CONT(X, ORLG_PHY_POLICY_SAPBM, TRACE)                   \
    ORLG_PHY_KEYS_CONT(X, ORLG_PHY_POLICY_FAFF, TRACE) ORLG_PHY_KEYS_CONT(X, ORLG_PHY_POLICY_FAFF_RSS, TRACE)
#endif
#define ORLG_PHY_KEYS(X) ORLG_PHY_KEYS_OF(X, false) ORLG_PHY_KEYS_OF(X, true)

// the lists as arrays; a key's position is its dense index (orlg_phy_env::resident_blocks), -1 for a key that is not legal
#define ORLG_WAVE_KEY_ENTRY(name, ...) OrlgWaveKey{ORLG_WAVE_KERNEL(name), __VA_ARGS__},
#define ORLG_GROUP_KEY_ENTRY(...) OrlgGroupKey{__VA_ARGS__},
#define ORLG_PHY_KEY_ENTRY(...) OrlgPhyKey{__VA_ARGS__},
inline constexpr OrlgWaveKey ORLG_WAVE_KEY_LIST[] = {ORLG_WAVE_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_GN_KEY_LIST[] = {ORLG_WAVE_GN_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_CAUSE_KEY_LIST[] = {ORLG_WAVE_CAUSE_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_ASSIGN_KEY_LIST[] = {ORLG_WAVE_ASSIGN_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_CUT_KEY_LIST[] = {ORLG_WAVE_CUT_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_USAGE_KEY_LIST[] = {ORLG_WAVE_USAGE_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_GN_ASSIGN_KEY_LIST[] = {ORLG_WAVE_GN_ASSIGN_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_GN_CUT_KEY_LIST[] = {ORLG_WAVE_GN_CUT_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_GN_PROTECT_KEY_LIST[] = {ORLG_WAVE_GN_PROTECT_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgWaveKey ORLG_WAVE_GN_PROTECT_CAUSE_KEY_LIST[] = {ORLG_WAVE_GN_PROTECT_CAUSE_KEYS(ORLG_WAVE_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_KEY_LIST[] = {ORLG_GROUP_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_CAUSE_KEY_LIST[] = {ORLG_GROUP_CAUSE_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_ASSIGN_KEY_LIST[] = {ORLG_GROUP_ASSIGN_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_CUT_KEY_LIST[] = {ORLG_GROUP_CUT_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_USAGE_KEY_LIST[] = {ORLG_GROUP_USAGE_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgPhyKey ORLG_PHY_KEY_LIST[] = {ORLG_PHY_KEYS(ORLG_PHY_KEY_ENTRY)};
template <typename Key, size_t N>
static int orlg_key_index(const Key (&list)[N], const Key &key) {
    for (size_t i = 0; i < N; i++)
        if (list[i] == key) return (int)i;
    return -1;
}

// ---------------------------------------------------------------------------------------- names
// "kernel<W,arg,...>" as the compiler names the instantiation, spaces left out; trailing arguments that equal their default are
// dropped.  kind: 'i' an int, 'b' a bool, 'd' a bool whose default is false.
struct OrlgArg { int value; char kind; };
inline void orlg_format_kernel(char *buf, size_t cap, const char *kernel, int W, const OrlgArg *args, int n) {
    while (n > 0 && args[n - 1].kind == 'd' && !args[n - 1].value) --n;
    size_t at = (size_t)snprintf(buf, cap, "%s<%d", kernel, W);
    for (int i = 0; i < n && at < cap; i++)
        at += (size_t)(args[i].kind == 'i' ? snprintf(buf + at, cap - at, ",%d", args[i].value)
                                           : snprintf(buf + at, cap - at, ",%s", args[i].value ? "true" : "false"));
    if (at < cap) snprintf(buf + at, cap - at, ">");
}
inline void orlg_kernel_name(char *buf, size_t cap, int W, const OrlgWaveKey &k) {
#define X(name) #name,
    static const char *const names[] = {ORLG_WAVE_KERNELS(X)};
#undef X
    const OrlgArg args[] = {{k.STATS, 'i'}, {k.DEFER, 'd'}, {k.GN, 'd'}, {k.CAUSE, 'd'}, {k.ASSIGN, 'd'}, {k.CUT, 'd'}, {k.USAGE, 'd'}, {k.PROTECT, 'd'}};
    orlg_format_kernel(buf, cap, names[k.kernel], W, args, k.kernel == ORLG_WAVE_KERNEL(orlg_rmsa_reset_kernel) ? 1 : 8);
}
inline void orlg_kernel_name(char *buf, size_t cap, int W, const OrlgGroupKey &k) {
    const OrlgArg args[] = {{k.STATS, 'i'}, {k.HBMQ, 'd'}, {k.DEFER, 'd'}, {k.TRAFFIC, 'd'}, {k.TRACE, 'd'}, {k.CAUSE, 'd'}, {k.ASSIGN, 'd'}, {k.CUT, 'd'}, {k.USAGE, 'd'}};
    orlg_format_kernel(buf, cap, "orlg_rmsa_group_kernel", W, args, 9);
}
inline void orlg_kernel_name(char *buf, size_t cap, int W, const OrlgPhyKey &k) {
    const OrlgArg args[] = {{k.DF, 'b'}, {k.GN, 'b'}, {k.POL, 'i'}, {k.CONT, 'd'}, {k.TRACE, 'd'}};
    orlg_format_kernel(buf, cap, "orlg_phy_kernel", W, args, 5);
}

// ---------------------------------------------------------------------------------------- kernel instantiation units
// Every unit (orlg_inst_*.hip, one object per word count W so that the library builds in parallel: build.py) exports one lookup
// per W: key -> instantiation, null for a key that is not legal.  A W the library was not built for is a null (weak) symbol.
struct OrlgParams;
struct OrlgPhyParams;
typedef void (*orlg_rmsa_kernel_t)(const OrlgParams);
typedef void (*orlg_masks_kernel_t)(const OrlgParams, int, int, int, uint64_t *, int32_t *);   // orlg_path_masks_kernel
typedef void (*orlg_obs_kernel_t)(const OrlgParams, uint8_t *, int);                          // orlg_deeprmsa_obs_kernel
typedef void (*orlg_action_masks_kernel_t)(const OrlgParams, uint8_t *, int, uint64_t *);     // orlg_action_masks_kernel
typedef void (*orlg_gn_action_masks_kernel_t)(const OrlgParams, uint8_t *, double *, uint8_t *, double *, int);   // orlg_gn_action_masks_kernel
typedef void (*orlg_fit_levels_kernel_t)(const OrlgParams, uint8_t *);                         // orlg_fit_levels_kernel
typedef void (*orlg_min_cuts_kernel_t)(const OrlgParams, int16_t *, int16_t *);                // orlg_min_cuts_kernel
typedef void (*orlg_usage_kernel_t)(const OrlgParams, uint8_t *, int32_t *, int16_t *);     // orlg_usage_kernel
typedef void (*orlg_gn_path_windows_kernel_t)(const OrlgParams, int, int16_t *, double *, uint8_t *);   // orlg_gn_path_windows_kernel
// orlg_gn_admission_kernels.hip: masks / rule windows that know both halves of the GN-model admission check
typedef void (*orlg_gn_admission_masks_kernel_t)(const OrlgParams, uint8_t *, double *, double *, uint8_t *, double *, double *, int, int);
typedef void (*orlg_gn_admission_windows_kernel_t)(const OrlgParams, int, int16_t *, double *, double *, uint8_t *, int);
typedef void (*orlg_phy_kernel_t)(const OrlgPhyParams);
// orlg_gn_audit_kernels.hip: the two kernels of the audit know no word count -- one object, one lookup each, no W
typedef void (*orlg_gn_audit_kernel_t)(const OrlgParams, const double *, orlg_gn_audit_summary *, double *, double *, double *, double *);
typedef void (*orlg_running_services_kernel_t)(const OrlgParams, int32_t *, int32_t *, int32_t *, int16_t *, int16_t *, int32_t *, double *, int16_t *);
orlg_gn_audit_kernel_t orlg_gn_audit_kernel_lookup();
orlg_running_services_kernel_t orlg_running_services_kernel_lookup();
#define ORLG_FOR_EACH_W(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__) X(6, __VA_ARGS__) X(8, __VA_ARGS__)
#define ORLG_FOR_EACH_PHY_W(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__)
#define ORLG_DECL_W(n, ...)                                                                       \
    orlg_rmsa_kernel_t orlg_wave_kernel_W##n(OrlgWaveKey) __attribute__((weak));                  \
    orlg_masks_kernel_t orlg_masks_kernel_W##n() __attribute__((weak));                           \
    orlg_obs_kernel_t orlg_obs_kernel_W##n() __attribute__((weak));                               \
    orlg_action_masks_kernel_t orlg_action_masks_kernel_W##n() __attribute__((weak));             \
    orlg_gn_action_masks_kernel_t orlg_gn_action_masks_kernel_W##n() __attribute__((weak));       \
    orlg_fit_levels_kernel_t orlg_fit_levels_kernel_W##n() __attribute__((weak));                 \
    orlg_min_cuts_kernel_t orlg_min_cuts_kernel_W##n() __attribute__((weak));                     \
    orlg_usage_kernel_t orlg_usage_kernel_W##n() __attribute__((weak));                           \
    orlg_rmsa_kernel_t orlg_gnrules_kernel_W##n(OrlgWaveKey) __attribute__((weak));   /* orlg_inst_gnrules.hip */ \
    orlg_gn_path_windows_kernel_t orlg_gn_path_windows_kernel_W##n() __attribute__((weak));       \
    orlg_rmsa_kernel_t orlg_gnprotect_kernel_W##n(OrlgWaveKey) __attribute__((weak));   /* orlg_inst_gnprotect.hip */ \
    orlg_gn_admission_masks_kernel_t orlg_gn_admission_masks_kernel_W##n() __attribute__((weak));   /* orlg_inst_gnadmit.hip */ \
    orlg_gn_admission_windows_kernel_t orlg_gn_admission_windows_kernel_W##n() __attribute__((weak)); \
    orlg_rmsa_kernel_t orlg_group_kernel_W##n(OrlgGroupKey) __attribute__((weak));
#define ORLG_DECL_PHY_W(n, ...)                                                                   \
    orlg_phy_kernel_t orlg_phy_kernel_W##n(OrlgPhyKey) __attribute__((weak));                     \
    orlg_phy_kernel_t orlg_phy_trace_kernel_W##n(OrlgPhyKey) __attribute__((weak));   /* orlg_inst_phy.hip with -DORLG_INST_TRACE=1 */
ORLG_FOR_EACH_W(ORLG_DECL_W, )
ORLG_FOR_EACH_PHY_W(ORLG_DECL_PHY_W, )
#undef ORLG_DECL_W
#undef ORLG_DECL_PHY_W
// orlg_gn_slots_kernels.hip: the admission check over every start slot of every path -- a unit of its own (orlg_inst_gnslots.hip,
// one object per W) with a declaration list of its own: the lists above stay what they are
typedef void (*orlg_gn_slots_kernel_t)(const OrlgParams, uint64_t *, double *, double *, int16_t *, double *, int);
#define ORLG_DECL_GN_SLOTS_W(n, ...) orlg_gn_slots_kernel_t orlg_gn_slots_kernel_W##n() __attribute__((weak));
ORLG_FOR_EACH_W(ORLG_DECL_GN_SLOTS_W, )
#undef ORLG_DECL_GN_SLOTS_W
// orlg_rmsa_mm_kernel (orlg_kernels.hip): the gated step kernel under a max-margin policy (orlg_step_max_margin) --
// template <int W, int STATS, bool CAUSE = false>, a kernel name, a key, a key list, a unit (orlg_inst_gnmm.hip, one object per W) and a
// declaration list of its own: the lists above stay what they are.  X(STATS[, CAUSE]): per statistics level, without and with the
// classifier; protection is a runtime argument of the launch (OrlgMmArgs), no key
struct OrlgMmKey { int STATS; bool CAUSE = false; };
inline bool operator==(const OrlgMmKey &a, const OrlgMmKey &b) { return a.STATS == b.STATS && a.CAUSE == b.CAUSE; }
#define ORLG_WAVE_GN_MM_KEYS(X) X(1) X(2) X(0) X(1, true) X(2, true) X(0, true)
#define ORLG_MM_KEY_ENTRY(...) OrlgMmKey{__VA_ARGS__},
inline constexpr OrlgMmKey ORLG_WAVE_GN_MM_KEY_LIST[] = {ORLG_WAVE_GN_MM_KEYS(ORLG_MM_KEY_ENTRY)};
inline void orlg_kernel_name(char *buf, size_t cap, int W, const OrlgMmKey &k) {
    const OrlgArg args[] = {{k.STATS, 'i'}, {k.CAUSE, 'd'}};
    orlg_format_kernel(buf, cap, "orlg_rmsa_mm_kernel", W, args, 2);
}
struct OrlgMmArgs;
typedef void (*orlg_rmsa_mm_kernel_t)(const OrlgParams, const OrlgMmArgs);
#define ORLG_DECL_GN_MM_W(n, ...) orlg_rmsa_mm_kernel_t orlg_gnmm_kernel_W##n(OrlgMmKey) __attribute__((weak));
ORLG_FOR_EACH_W(ORLG_DECL_GN_MM_W, )
#undef ORLG_DECL_GN_MM_W
// orlg_rmsa_am_kernel (orlg_kernels.hip): the gated step kernel of a handle whose gate chooses the modulation from the GSNR
// (orlg_set_gn_modulation) -- template <int W, int STATS>, a kernel name, a key, a key list, a unit (orlg_inst_gnam.hip,
// one object per W, which also holds the modulation query orlg_gn_modulation_kernel) and a declaration list of its own, behind the
// ones above: they stay what they are.  X(STATS): per statistics level
struct OrlgAmKey { int STATS; };
inline bool operator==(const OrlgAmKey &a, const OrlgAmKey &b) { return a.STATS == b.STATS; }
#define ORLG_WAVE_GN_AM_KEYS(X) X(1) X(2) X(0)
#define ORLG_AM_KEY_ENTRY(...) OrlgAmKey{__VA_ARGS__},
inline constexpr OrlgAmKey ORLG_WAVE_GN_AM_KEY_LIST[] = {ORLG_WAVE_GN_AM_KEYS(ORLG_AM_KEY_ENTRY)};
inline void orlg_kernel_name(char *buf, size_t cap, int W, const OrlgAmKey &k) {
    const OrlgArg args[] = {{k.STATS, 'i'}};
    orlg_format_kernel(buf, cap, "orlg_rmsa_am_kernel", W, args, 1);
}
struct OrlgAmArgs;
typedef void (*orlg_rmsa_am_kernel_t)(const OrlgParams, const OrlgAmArgs);
typedef void (*orlg_gn_modulation_kernel_t)(const OrlgParams, int16_t *, double *, uint8_t *, uint8_t *);   // orlg_gn_modulation_kernel
#define ORLG_DECL_GN_AM_W(n, ...)                                                    \
    orlg_rmsa_am_kernel_t orlg_gnam_kernel_W##n(OrlgAmKey) __attribute__((weak)); \
    orlg_gn_modulation_kernel_t orlg_gn_modulation_kernel_W##n() __attribute__((weak));
ORLG_FOR_EACH_W(ORLG_DECL_GN_AM_W, )
#undef ORLG_DECL_GN_AM_W

// the lookup `lookup`<W> called with the arguments after it, as a function body: null when the library holds no such W
#define ORLG_PICK_CASE(n, lookup, ...) case n: return lookup##n ? lookup##n(__VA_ARGS__) : nullptr;
#define ORLG_PICK(FOR_EACH_W, W, lookup, ...) switch (W) { FOR_EACH_W(ORLG_PICK_CASE, lookup, __VA_ARGS__) default: return nullptr; }
static orlg_rmsa_kernel_t orlg_pick(int W, const OrlgWaveKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_wave_kernel_W, key) }
// the GN x ASSIGN keys (ORLG_WAVE_GN_ASSIGN_KEYS, ORLG_WAVE_GN_CUT_KEYS): a lookup of their own -- orlg_pick answers for the keys it
// always answered for, and with null for these
static orlg_rmsa_kernel_t orlg_pick_gn_rules(int W, const OrlgWaveKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gnrules_kernel_W, key) }
// the PROTECT keys (ORLG_WAVE_GN_PROTECT_KEYS, ORLG_WAVE_GN_PROTECT_CAUSE_KEYS): a lookup of their own, for the same reason
static orlg_rmsa_kernel_t orlg_pick_gn_protect(int W, const OrlgWaveKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gnprotect_kernel_W, key) }
static orlg_rmsa_kernel_t orlg_pick(int W, const OrlgGroupKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_group_kernel_W, key) }
static orlg_phy_kernel_t orlg_pick(int W, const OrlgPhyKey &key) {   // the TRACE instantiations are objects of their own
    if (key.TRACE) { ORLG_PICK(ORLG_FOR_EACH_PHY_W, W, orlg_phy_trace_kernel_W, key) }
    ORLG_PICK(ORLG_FOR_EACH_PHY_W, W, orlg_phy_kernel_W, key)
}
static orlg_masks_kernel_t orlg_pick_masks(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_masks_kernel_W, ) }
static orlg_obs_kernel_t orlg_pick_obs(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_obs_kernel_W, ) }
static orlg_action_masks_kernel_t orlg_pick_action_masks(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_action_masks_kernel_W, ) }
static orlg_fit_levels_kernel_t orlg_pick_fit_levels(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_fit_levels_kernel_W, ) }
static orlg_min_cuts_kernel_t orlg_pick_min_cuts(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_min_cuts_kernel_W, ) }
static orlg_usage_kernel_t orlg_pick_usage(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_usage_kernel_W, ) }
static orlg_gn_action_masks_kernel_t orlg_pick_gn_action_masks(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gn_action_masks_kernel_W, ) }
static orlg_gn_path_windows_kernel_t orlg_pick_gn_path_windows(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gn_path_windows_kernel_W, ) }
static orlg_gn_admission_masks_kernel_t orlg_pick_gn_admission_masks(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gn_admission_masks_kernel_W, ) }
static orlg_gn_admission_windows_kernel_t orlg_pick_gn_admission_windows(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gn_admission_windows_kernel_W, ) }
static orlg_gn_slots_kernel_t orlg_pick_gn_slots(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gn_slots_kernel_W, ) }
static orlg_rmsa_mm_kernel_t orlg_pick_gn_mm(int W, const OrlgMmKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gnmm_kernel_W, key) }
static orlg_rmsa_am_kernel_t orlg_pick_gn_am(int W, const OrlgAmKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gnam_kernel_W, key) }
static orlg_gn_modulation_kernel_t orlg_pick_gn_modulation(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gn_modulation_kernel_W, ) }
