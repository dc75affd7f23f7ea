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

constexpr bool operator==(const OrlgWaveKey &a, const OrlgWaveKey &b) { return a.kernel == b.kernel && a.STATS == b.STATS && a.DEFER == b.DEFER && a.GN == b.GN && a.CAUSE == b.CAUSE && a.ASSIGN == b.ASSIGN && a.CUT == b.CUT && a.USAGE == b.USAGE && a.PROTECT == b.PROTECT; }
constexpr bool operator==(const OrlgGroupKey &a, const OrlgGroupKey &b) {
    return a.STATS == b.STATS && a.HBMQ == b.HBMQ && a.DEFER == b.DEFER && a.TRAFFIC == b.TRAFFIC && a.TRACE == b.TRACE && a.CAUSE == b.CAUSE && a.ASSIGN == b.ASSIGN && a.CUT == b.CUT && a.USAGE == b.USAGE;
}
constexpr bool operator==(const OrlgPhyKey &a, const OrlgPhyKey &b) {
    return a.DF == b.DF && a.GN == b.GN && a.POL == b.POL && a.CONT == b.CONT && a.TRACE == b.TRACE;
}

// ---------------------------------------------------------------------------------------- the legal keys
// X(kernel, STATS[, DEFER[, GN[, CAUSE[, ASSIGN[, CUT[, USAGE[, PROTECT]]]]]]]).  A list is written by composition: the statistics
// levels once, in ORLG_STATS_LEVELS (1, 2, 0: the order the kernels have always lain in a unit's code object, so that a build can be
// compared with its predecessor byte by byte -- tools/device_code_diff.py), and of orlg_rmsa_kernel's flags only those the list turns
// on, by name.  One list per launch kind, under the name the instantiation units and the tests know; which unit holds which list:
// ORLG_WAVE_UNITS, below.  A new variant of the wave kernel is one more entry here and one row of orlg_wave_choose (orlg_wave_plan.h).
#define ORLG_STATS_LEVELS(L, ...) L(1, __VA_ARGS__) L(2, __VA_ARGS__) L(0, __VA_ARGS__)
enum { ORLG_F_DEFER = 1, ORLG_F_GN = 2, ORLG_F_CAUSE = 4, ORLG_F_ASSIGN = 8, ORLG_F_CUT = 16, ORLG_F_USAGE = 32, ORLG_F_PROTECT = 64 };
#define ORLG_WAVE_FLAGS(F) \
    ((F) & ORLG_F_DEFER) != 0, ((F) & ORLG_F_GN) != 0, ((F) & ORLG_F_CAUSE) != 0, ((F) & ORLG_F_ASSIGN) != 0, ((F) & ORLG_F_CUT) != 0, ((F) & ORLG_F_USAGE) != 0, ((F) & ORLG_F_PROTECT) != 0
#define ORLG_WAVE_LEVEL_(stats, X, kernel) X(kernel, stats)
#define ORLG_WAVE_LEVEL_OF_(stats, X, F) X(orlg_rmsa_kernel, stats, ORLG_WAVE_FLAGS(F))
#define ORLG_WAVE_LEVELS(X, kernel) ORLG_STATS_LEVELS(ORLG_WAVE_LEVEL_, X, kernel)   // a kernel without flags, per level
#define ORLG_WAVE_LEVELS_OF(X, F) ORLG_STATS_LEVELS(ORLG_WAVE_LEVEL_OF_, X, F)       // orlg_rmsa_kernel with the flags F, per level
// what a handle without a gate reaches under the reference's first fit.  DEFER: full statistics with the links' float64 part
// deferred (link_replay); _ff: the first-fit policies only (k <= 8); the reset kernel has no DEFER
#define ORLG_WAVE_KEYS(X)                                                              \
    ORLG_WAVE_LEVELS(X, orlg_rmsa_kernel) ORLG_WAVE_LEVELS(X, orlg_rmsa_kernel_ff)     \
    X(orlg_rmsa_kernel, 2, true) X(orlg_rmsa_kernel_ff, 2, true)                       \
    ORLG_WAVE_LEVELS(X, orlg_rmsa_reset_kernel)
// what a handle with a GN-model admission check launches (orlg_set_gn_gate): no _ff and no DEFER variant
#define ORLG_WAVE_GN_KEYS(X) ORLG_WAVE_LEVELS_OF(X, ORLG_F_GN)
// a launch that asks for the blocking cause of its steps (orlg_step_diag): the classifier without and with the check; no _ff and no
// DEFER variant (optimisations that leave the same state: such a launch does without them)
#define ORLG_WAVE_CAUSE_KEYS(X) ORLG_WAVE_LEVELS_OF(X, ORLG_F_CAUSE) ORLG_WAVE_LEVELS_OF(X, ORLG_F_GN | ORLG_F_CAUSE)
// a launch under an assignment rule other than the reference's first fit (orlg_step_assign), without and with the classifier
#define ORLG_WAVE_ASSIGN_KEYS(X) ORLG_WAVE_LEVELS_OF(X, ORLG_F_ASSIGN) ORLG_WAVE_LEVELS_OF(X, ORLG_F_CAUSE | ORLG_F_ASSIGN)
// a launch under the fewest-cuts window (orlg_step_min_cut): the ASSIGN keys again with CUT.  The rule's hop loop, with its cut
// counters, is not in the ASSIGN instantiations: inside them it cost the classic rules of the group kernel 1.5 %
#define ORLG_WAVE_CUT_KEYS(X) \
    ORLG_WAVE_LEVELS_OF(X, ORLG_F_ASSIGN | ORLG_F_CUT) ORLG_WAVE_LEVELS_OF(X, ORLG_F_CAUSE | ORLG_F_ASSIGN | ORLG_F_CUT)
// a launch of orlg_step_window under the rule MOST_USED or the route BEST_WINDOW (orlg_usage.h): the ASSIGN keys again
// with USAGE, for the reason the CUT keys have
#define ORLG_WAVE_USAGE_KEYS(X) \
    ORLG_WAVE_LEVELS_OF(X, ORLG_F_ASSIGN | ORLG_F_USAGE) ORLG_WAVE_LEVELS_OF(X, ORLG_F_CAUSE | ORLG_F_ASSIGN | ORLG_F_USAGE)
// what orlg_step_rule_gn launches: the ASSIGN keys and the CUT keys again with GN -- an assignment rule, or the
// fewest-cuts window, whose proposal goes through the admission check.  No USAGE (refused)
#define ORLG_WAVE_GN_ASSIGN_KEYS(X) \
    ORLG_WAVE_LEVELS_OF(X, ORLG_F_GN | ORLG_F_ASSIGN) ORLG_WAVE_LEVELS_OF(X, ORLG_F_GN | ORLG_F_CAUSE | ORLG_F_ASSIGN)
#define ORLG_WAVE_GN_CUT_KEYS(X) \
    ORLG_WAVE_LEVELS_OF(X, ORLG_F_GN | ORLG_F_ASSIGN | ORLG_F_CUT) ORLG_WAVE_LEVELS_OF(X, ORLG_F_GN | ORLG_F_CAUSE | ORLG_F_ASSIGN | ORLG_F_CUT)
// what a handle that protects its running lightpaths launches (orlg_set_gn_protect): the GN keys again with PROTECT,
// without and with the classifier
#define ORLG_WAVE_GN_PROTECT_KEYS(X) ORLG_WAVE_LEVELS_OF(X, ORLG_F_GN | ORLG_F_PROTECT)
#define ORLG_WAVE_GN_PROTECT_CAUSE_KEYS(X) ORLG_WAVE_LEVELS_OF(X, ORLG_F_GN | ORLG_F_CAUSE | ORLG_F_PROTECT)
// Which instantiation unit holds which lists, U(the unit's exported lookup per W, its lists in the order it expands them): the units
// are objects of their own per W (build.py) so that a new list leaves the code objects of the older ones byte for byte what they
// were.  From this table: the family's key array, the weak declarations and the host's one lookup, orlg_pick
#define ORLG_WAVE_UNIT_KEYS(X) \
    ORLG_WAVE_KEYS(X) ORLG_WAVE_GN_KEYS(X) ORLG_WAVE_CAUSE_KEYS(X) ORLG_WAVE_ASSIGN_KEYS(X) ORLG_WAVE_CUT_KEYS(X) ORLG_WAVE_USAGE_KEYS(X)
#define ORLG_GNRULES_UNIT_KEYS(X) ORLG_WAVE_GN_ASSIGN_KEYS(X) ORLG_WAVE_GN_CUT_KEYS(X)
#define ORLG_GNPROTECT_UNIT_KEYS(X) ORLG_WAVE_GN_PROTECT_KEYS(X) ORLG_WAVE_GN_PROTECT_CAUSE_KEYS(X)
#define ORLG_WAVE_UNITS(U)                            /* orlg_inst_wave.hip, orlg_inst_gnrules.hip, orlg_inst_gnprotect.hip */ \
    U(orlg_wave_kernel_W, ORLG_WAVE_UNIT_KEYS) U(orlg_gnrules_kernel_W, ORLG_GNRULES_UNIT_KEYS) U(orlg_gnprotect_kernel_W, ORLG_GNPROTECT_UNIT_KEYS)

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
// optimisations that leave identical state; orlg_group_plan.h keeps a cause launch off them.  Expanded last
#define ORLG_GROUP_CAUSE_KEYS_OF(X, TRAFFIC, TRACE) \
    X(0, false, false, TRAFFIC, TRACE, true) X(1, false, false, TRAFFIC, TRACE, true) X(2, false, false, TRAFFIC, TRACE, true)
#define ORLG_GROUP_CAUSE_KEYS(X) \
    ORLG_GROUP_CAUSE_KEYS_OF(X, false, false) ORLG_GROUP_CAUSE_KEYS_OF(X, true, false) ORLG_GROUP_CAUSE_KEYS_OF(X, false, true)
// X(STATS, HBMQ, DEFER, TRAFFIC, TRACE, CAUSE, ASSIGN): the launches under an assignment rule other than the reference's first fit
// -- the plain kind per statistics level and kind of handle, without and with the classifier (orlg_group_plan.h keeps such a
// launch off HBMQ, DEFER and the lean body through ORLG_OUT_ASSIGN_BIT).  Expanded after the CAUSE keys
#define ORLG_GROUP_ASSIGN_KEYS_OF(X, TRAFFIC, TRACE, CAUSE) \
    X(0, false, false, TRAFFIC, TRACE, CAUSE, true) X(1, false, false, TRAFFIC, TRACE, CAUSE, true) X(2, false, false, TRAFFIC, TRACE, CAUSE, true)
#define ORLG_GROUP_ASSIGN_KEYS(X)                                                                                                           \
    ORLG_GROUP_ASSIGN_KEYS_OF(X, false, false, false) ORLG_GROUP_ASSIGN_KEYS_OF(X, true, false, false) ORLG_GROUP_ASSIGN_KEYS_OF(X, false, true, false) \
    ORLG_GROUP_ASSIGN_KEYS_OF(X, false, false, true) ORLG_GROUP_ASSIGN_KEYS_OF(X, true, false, true) ORLG_GROUP_ASSIGN_KEYS_OF(X, false, true, true)
// X(STATS, HBMQ, DEFER, TRAFFIC, TRACE, CAUSE, ASSIGN, CUT): the launches under the fewest-cuts window -- the ASSIGN keys again with
// CUT (as ORLG_WAVE_CUT_KEYS).  Expanded last
#define ORLG_GROUP_CUT_KEYS_OF(X, TRAFFIC, TRACE, CAUSE) \
    X(0, false, false, TRAFFIC, TRACE, CAUSE, true, true) X(1, false, false, TRAFFIC, TRACE, CAUSE, true, true) X(2, false, false, TRAFFIC, TRACE, CAUSE, true, true)
#define ORLG_GROUP_CUT_KEYS(X)                                                                                                     \
    ORLG_GROUP_CUT_KEYS_OF(X, false, false, false) ORLG_GROUP_CUT_KEYS_OF(X, true, false, false) ORLG_GROUP_CUT_KEYS_OF(X, false, true, false) \
    ORLG_GROUP_CUT_KEYS_OF(X, false, false, true) ORLG_GROUP_CUT_KEYS_OF(X, true, false, true) ORLG_GROUP_CUT_KEYS_OF(X, false, true, true)
// X(STATS, HBMQ, DEFER, TRAFFIC, TRACE, CAUSE, ASSIGN, CUT, USAGE): the launches of orlg_step_window under the rule MOST_USED or the
// route BEST_WINDOW -- the ASSIGN keys again with USAGE (as ORLG_WAVE_USAGE_KEYS).  Expanded last
#define ORLG_GROUP_USAGE_KEYS_OF(X, TRAFFIC, TRACE, CAUSE) \
    X(0, false, false, TRAFFIC, TRACE, CAUSE, true, false, true) X(1, false, false, TRAFFIC, TRACE, CAUSE, true, false, true) X(2, false, false, TRAFFIC, TRACE, CAUSE, true, false, true)
#define ORLG_GROUP_USAGE_KEYS(X)                                                                                                         \
    ORLG_GROUP_USAGE_KEYS_OF(X, false, false, false) ORLG_GROUP_USAGE_KEYS_OF(X, true, false, false) ORLG_GROUP_USAGE_KEYS_OF(X, false, true, false) \
    ORLG_GROUP_USAGE_KEYS_OF(X, false, false, true) ORLG_GROUP_USAGE_KEYS_OF(X, true, false, true) ORLG_GROUP_USAGE_KEYS_OF(X, false, true, true)
// the group kernel's one unit (orlg_inst_group.hip) holds them all, in this order
#define ORLG_GROUP_UNIT_KEYS(X) ORLG_GROUP_KEYS(X) ORLG_GROUP_CAUSE_KEYS(X) ORLG_GROUP_ASSIGN_KEYS(X) ORLG_GROUP_CUT_KEYS(X) ORLG_GROUP_USAGE_KEYS(X)

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
#define ORLG_WAVE_KEY_ARRAY(LIST) inline constexpr OrlgWaveKey LIST##_LIST[] = {LIST##S(ORLG_WAVE_KEY_ENTRY)};
ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_KEY) ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_GN_KEY) ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_CAUSE_KEY)
ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_ASSIGN_KEY) ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_CUT_KEY) ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_USAGE_KEY)
ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_GN_ASSIGN_KEY) ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_GN_CUT_KEY)
ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_GN_PROTECT_KEY) ORLG_WAVE_KEY_ARRAY(ORLG_WAVE_GN_PROTECT_CAUSE_KEY)
#undef ORLG_WAVE_KEY_ARRAY
// the whole family, unit by unit in the table's order
#define ORLG_UNIT_ENTRIES(lookup, KEYS) KEYS(ORLG_WAVE_KEY_ENTRY)
inline constexpr OrlgWaveKey ORLG_WAVE_ALL_KEY_LIST[] = {ORLG_WAVE_UNITS(ORLG_UNIT_ENTRIES)};
#undef ORLG_UNIT_ENTRIES
inline constexpr OrlgGroupKey ORLG_GROUP_KEY_LIST[] = {ORLG_GROUP_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_CAUSE_KEY_LIST[] = {ORLG_GROUP_CAUSE_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_ASSIGN_KEY_LIST[] = {ORLG_GROUP_ASSIGN_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_CUT_KEY_LIST[] = {ORLG_GROUP_CUT_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_USAGE_KEY_LIST[] = {ORLG_GROUP_USAGE_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgGroupKey ORLG_GROUP_ALL_KEY_LIST[] = {ORLG_GROUP_UNIT_KEYS(ORLG_GROUP_KEY_ENTRY)};
inline constexpr OrlgPhyKey ORLG_PHY_KEY_LIST[] = {ORLG_PHY_KEYS(ORLG_PHY_KEY_ENTRY)};
template <typename Key, size_t N>
static int orlg_key_index(const Key (&list)[N], const Key &key) {
    for (size_t i = 0; i < N; i++)
        if (list[i] == key) return (int)i;
    return -1;
}
// what the lists hold, in number, and that no key of the wave family stands in two of them (orlg_pick takes the first unit that answers)
template <typename Key, size_t N>
constexpr size_t orlg_key_count(const Key (&)[N]) { return N; }
template <typename Key, size_t N>
constexpr bool orlg_keys_differ(const Key (&list)[N]) {
    for (size_t i = 0; i < N; i++)
        for (size_t j = i + 1; j < N; j++)
            if (list[i] == list[j]) return false;
    return true;
}
static_assert(orlg_keys_differ(ORLG_WAVE_ALL_KEY_LIST) && orlg_key_count(ORLG_WAVE_ALL_KEY_LIST) == 11 + 3 + 6 + 6 + 6 + 6 + 6 + 6 + 3 + 3, "the wave family's keys");
static_assert(orlg_key_count(ORLG_WAVE_KEY_LIST) == 11 && orlg_key_count(ORLG_WAVE_GN_KEY_LIST) == 3 && orlg_key_count(ORLG_WAVE_CAUSE_KEY_LIST) == 6 &&
              orlg_key_count(ORLG_WAVE_ASSIGN_KEY_LIST) == 6 && orlg_key_count(ORLG_WAVE_CUT_KEY_LIST) == 6 && orlg_key_count(ORLG_WAVE_USAGE_KEY_LIST) == 6, "orlg_inst_wave.hip");
static_assert(orlg_key_count(ORLG_WAVE_GN_ASSIGN_KEY_LIST) == 6 && orlg_key_count(ORLG_WAVE_GN_CUT_KEY_LIST) == 6, "orlg_inst_gnrules.hip");
static_assert(orlg_key_count(ORLG_WAVE_GN_PROTECT_KEY_LIST) == 3 && orlg_key_count(ORLG_WAVE_GN_PROTECT_CAUSE_KEY_LIST) == 3, "orlg_inst_gnprotect.hip");
static_assert(orlg_keys_differ(ORLG_GROUP_ALL_KEY_LIST) && orlg_key_count(ORLG_GROUP_KEY_LIST) == 21 && orlg_key_count(ORLG_GROUP_CAUSE_KEY_LIST) == 9 && orlg_key_count(ORLG_GROUP_ASSIGN_KEY_LIST) == 18 &&
              orlg_key_count(ORLG_GROUP_CUT_KEY_LIST) == 18 && orlg_key_count(ORLG_GROUP_USAGE_KEY_LIST) == 18, "orlg_inst_group.hip");
#ifndef ORLG_PHY_FEW_POLICIES
static_assert(orlg_key_count(ORLG_PHY_KEY_LIST) == 96, "orlg_inst_phy.hip");
#endif

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

// ---------------------------------------------------------------------------------------- the keys of the other two step kernels
// orlg_rmsa_mm_kernel (orlg_kernels.hip): the gated step kernel under a max-margin policy (orlg_step_max_margin) --
// template <int W, int STATS, bool CAUSE = false>; its unit is orlg_inst_gnmm.hip.  The kernel takes a second argument (OrlgMmArgs:
// protection is a runtime argument of the launch, no key), hence a key type and a lookup type of its own.  X(STATS[, CAUSE]): per
// statistics level, without and with the classifier
struct OrlgMmKey { int STATS; bool CAUSE = false; };
constexpr bool operator==(const OrlgMmKey &a, const OrlgMmKey &b) { return a.STATS == b.STATS && a.CAUSE == b.CAUSE; }
#define ORLG_WAVE_GN_MM_KEYS(X) X(1) X(2) X(0) X(1, true) X(2, true) X(0, true)
#define ORLG_MM_KEY_ENTRY(...) OrlgMmKey{__VA_ARGS__},
inline constexpr OrlgMmKey ORLG_WAVE_GN_MM_KEY_LIST[] = {ORLG_WAVE_GN_MM_KEYS(ORLG_MM_KEY_ENTRY)};
inline void orlg_kernel_name(char *buf, size_t cap, int W, const OrlgMmKey &k) {
    const OrlgArg args[] = {{k.STATS, 'i'}, {k.CAUSE, 'd'}};
    orlg_format_kernel(buf, cap, "orlg_rmsa_mm_kernel", W, args, 2);
}
// orlg_rmsa_am_kernel (orlg_kernels.hip): the gated step kernel of a handle whose gate chooses the modulation from the GSNR
// (orlg_set_gn_modulation) -- template <int W, int STATS>; its unit is orlg_inst_gnam.hip, which also holds the
// modulation query.  Second argument: OrlgAmArgs.  X(STATS): per statistics level
struct OrlgAmKey { int STATS; };
constexpr bool operator==(const OrlgAmKey &a, const OrlgAmKey &b) { return a.STATS == b.STATS; }
#define ORLG_WAVE_GN_AM_KEYS(X) X(1) X(2) X(0)
#define ORLG_AM_KEY_ENTRY(...) OrlgAmKey{__VA_ARGS__},
inline constexpr OrlgAmKey ORLG_WAVE_GN_AM_KEY_LIST[] = {ORLG_WAVE_GN_AM_KEYS(ORLG_AM_KEY_ENTRY)};
inline void orlg_kernel_name(char *buf, size_t cap, int W, const OrlgAmKey &k) {
    const OrlgArg args[] = {{k.STATS, 'i'}};
    orlg_format_kernel(buf, cap, "orlg_rmsa_am_kernel", W, args, 1);
}
static_assert(orlg_key_count(ORLG_WAVE_GN_MM_KEY_LIST) == 6 && orlg_key_count(ORLG_WAVE_GN_AM_KEY_LIST) == 3, "orlg_inst_gnmm.hip, orlg_inst_gnam.hip");

// ---------------------------------------------------------------------------------------- kernel instantiation units
// Every unit (orlg_inst_*.hip, one object per word count W so that the library builds in parallel: build.py) exports one lookup
// per W: key -> instantiation, null for a key that is not legal.  A W the library was not built for is a null (weak) symbol.
struct OrlgParams;
struct OrlgPhyParams;
struct OrlgMmArgs;
struct OrlgAmArgs;
typedef void (*orlg_rmsa_kernel_t)(const OrlgParams);
typedef void (*orlg_rmsa_mm_kernel_t)(const OrlgParams, const OrlgMmArgs);
typedef void (*orlg_rmsa_am_kernel_t)(const OrlgParams, const OrlgAmArgs);
typedef void (*orlg_phy_kernel_t)(const OrlgPhyParams);
typedef void (*orlg_masks_kernel_t)(const OrlgParams, int, int, int, uint64_t *, int32_t *);
typedef void (*orlg_obs_kernel_t)(const OrlgParams, uint8_t *, int);
typedef void (*orlg_action_masks_kernel_t)(const OrlgParams, uint8_t *, int, uint64_t *);
typedef void (*orlg_gn_action_masks_kernel_t)(const OrlgParams, uint8_t *, double *, uint8_t *, double *, int);
typedef void (*orlg_fit_levels_kernel_t)(const OrlgParams, uint8_t *);
typedef void (*orlg_min_cuts_kernel_t)(const OrlgParams, int16_t *, int16_t *);
typedef void (*orlg_usage_kernel_t)(const OrlgParams, uint8_t *, int32_t *, int16_t *);
typedef void (*orlg_gn_path_windows_kernel_t)(const OrlgParams, int, int16_t *, double *, uint8_t *);
// (masks / rule windows that know both halves of the GN-model admission check; the check over every start slot of every path)
typedef void (*orlg_gn_admission_masks_kernel_t)(const OrlgParams, uint8_t *, double *, double *, uint8_t *, double *, double *, int, int);
typedef void (*orlg_gn_admission_windows_kernel_t)(const OrlgParams, int, int16_t *, double *, double *, uint8_t *, int);
typedef void (*orlg_gn_slots_kernel_t)(const OrlgParams, uint64_t *, double *, double *, int16_t *, double *, int);
typedef void (*orlg_gn_modulation_kernel_t)(const OrlgParams, int16_t *, double *, uint8_t *, uint8_t *);
// orlg_gn_audit_kernels.hip: the two kernels of the audit know no word count -- one object, one lookup each, no W
typedef void (*orlg_gn_audit_kernel_t)(const OrlgParams, const double *, orlg_gn_audit_summary *, double *, double *, double *, double *);
typedef void (*orlg_running_services_kernel_t)(const OrlgParams, int32_t *, int32_t *, int32_t *, int16_t *, int16_t *, int32_t *, double *, int16_t *);
orlg_gn_audit_kernel_t orlg_gn_audit_kernel_lookup();
orlg_running_services_kernel_t orlg_running_services_kernel_lookup();
// the lookups of one kernel each, per W: X(the host's lookup, the kernel's type, the unit's exported lookup, the kernel) -- by unit:
// orlg_inst_wave.hip, orlg_inst_gnrules.hip, orlg_inst_gnadmit.hip, orlg_inst_gnslots.hip, orlg_inst_gnam.hip
#define ORLG_WAVE_QUERIES(X)                                                                                                      \
    X(orlg_pick_masks, orlg_masks_kernel_t, orlg_masks_kernel_W, orlg_path_masks_kernel)                                          \
    X(orlg_pick_obs, orlg_obs_kernel_t, orlg_obs_kernel_W, orlg_deeprmsa_obs_kernel)                                              \
    X(orlg_pick_action_masks, orlg_action_masks_kernel_t, orlg_action_masks_kernel_W, orlg_action_masks_kernel)                   \
    X(orlg_pick_gn_action_masks, orlg_gn_action_masks_kernel_t, orlg_gn_action_masks_kernel_W, orlg_gn_action_masks_kernel)       \
    X(orlg_pick_fit_levels, orlg_fit_levels_kernel_t, orlg_fit_levels_kernel_W, orlg_fit_levels_kernel)                           \
    X(orlg_pick_min_cuts, orlg_min_cuts_kernel_t, orlg_min_cuts_kernel_W, orlg_min_cuts_kernel)                                   \
    X(orlg_pick_usage, orlg_usage_kernel_t, orlg_usage_kernel_W, orlg_usage_kernel)                                               \
    X(orlg_pick_gn_path_windows, orlg_gn_path_windows_kernel_t, orlg_gn_path_windows_kernel_W, orlg_gn_path_windows_kernel)       \
    X(orlg_pick_gn_admission_masks, orlg_gn_admission_masks_kernel_t, orlg_gn_admission_masks_kernel_W, orlg_gn_admission_masks_kernel) \
    X(orlg_pick_gn_admission_windows, orlg_gn_admission_windows_kernel_t, orlg_gn_admission_windows_kernel_W, orlg_gn_admission_windows_kernel) \
    X(orlg_pick_gn_slots, orlg_gn_slots_kernel_t, orlg_gn_slots_kernel_W, orlg_gn_slots_kernel)                                   \
    X(orlg_pick_gn_modulation, orlg_gn_modulation_kernel_t, orlg_gn_modulation_kernel_W, orlg_gn_modulation_kernel)
#define ORLG_FOR_EACH_W(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__) X(6, __VA_ARGS__) X(8, __VA_ARGS__)
#define ORLG_FOR_EACH_PHY_W(X, ...) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__)
// the weak declarations: the units of ORLG_WAVE_UNITS, the queries, and the units of the other key types
#define ORLG_DECL_LOOKUP_W(n, type, lookup, ...) type lookup##n(__VA_ARGS__) __attribute__((weak));
#define ORLG_DECL_UNIT(lookup, KEYS) ORLG_FOR_EACH_W(ORLG_DECL_LOOKUP_W, orlg_rmsa_kernel_t, lookup, OrlgWaveKey)
#define ORLG_DECL_QUERY(pick, type, lookup, kernel) ORLG_FOR_EACH_W(ORLG_DECL_LOOKUP_W, type, lookup, )
ORLG_WAVE_UNITS(ORLG_DECL_UNIT)
ORLG_WAVE_QUERIES(ORLG_DECL_QUERY)
ORLG_FOR_EACH_W(ORLG_DECL_LOOKUP_W, orlg_rmsa_mm_kernel_t, orlg_gnmm_kernel_W, OrlgMmKey)
ORLG_FOR_EACH_W(ORLG_DECL_LOOKUP_W, orlg_rmsa_am_kernel_t, orlg_gnam_kernel_W, OrlgAmKey)
ORLG_FOR_EACH_W(ORLG_DECL_LOOKUP_W, orlg_rmsa_kernel_t, orlg_group_kernel_W, OrlgGroupKey)
ORLG_FOR_EACH_PHY_W(ORLG_DECL_LOOKUP_W, orlg_phy_kernel_t, orlg_phy_kernel_W, OrlgPhyKey)
ORLG_FOR_EACH_PHY_W(ORLG_DECL_LOOKUP_W, orlg_phy_kernel_t, orlg_phy_trace_kernel_W, OrlgPhyKey)   // orlg_inst_phy.hip with -DORLG_INST_TRACE=1
#undef ORLG_DECL_UNIT
#undef ORLG_DECL_QUERY

// ---------------------------------------------------------------------------------------- the host's lookups
// the lookup `lookup`<W> called with the arguments after it, as a function body: null when the library holds no such W
#define ORLG_PICK_CASE(n, lookup, ...) case n: return lookup##n ? lookup##n(__VA_ARGS__) : nullptr;
#define ORLG_PICK(FOR_EACH_W, W, lookup, ...) switch (W) { FOR_EACH_W(ORLG_PICK_CASE, lookup, __VA_ARGS__) default: return nullptr; }
// one orlg_pick per key type.  The wave family's asks the units in the table's order and returns the first kernel (a key stands in
// one list: the static_assert above), so a caller need not know which unit holds a key
static orlg_rmsa_kernel_t orlg_pick(int W, const OrlgWaveKey &key) {
#define ORLG_PICK_UNIT(lookup, KEYS) \
    if (orlg_rmsa_kernel_t k = [&]() -> orlg_rmsa_kernel_t { ORLG_PICK(ORLG_FOR_EACH_W, W, lookup, key) }()) return k;
    ORLG_WAVE_UNITS(ORLG_PICK_UNIT)
#undef ORLG_PICK_UNIT
    return nullptr;
}
static orlg_rmsa_mm_kernel_t orlg_pick(int W, const OrlgMmKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gnmm_kernel_W, key) }
static orlg_rmsa_am_kernel_t orlg_pick(int W, const OrlgAmKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_gnam_kernel_W, key) }
static orlg_rmsa_kernel_t orlg_pick(int W, const OrlgGroupKey &key) { ORLG_PICK(ORLG_FOR_EACH_W, W, orlg_group_kernel_W, key) }
static orlg_phy_kernel_t orlg_pick(int W, const OrlgPhyKey &key) {   // the TRACE instantiations are objects of their own
    if (key.TRACE) { ORLG_PICK(ORLG_FOR_EACH_PHY_W, W, orlg_phy_trace_kernel_W, key) }
    ORLG_PICK(ORLG_FOR_EACH_PHY_W, W, orlg_phy_kernel_W, key)
}
#define ORLG_PICK_QUERY(pick, type, lookup, kernel) static type pick(int W) { ORLG_PICK(ORLG_FOR_EACH_W, W, lookup, ) }
ORLG_WAVE_QUERIES(ORLG_PICK_QUERY)
#undef ORLG_PICK_QUERY
