// orlg_step_call.h -- what a call of one of the RMSA step entry points (include/orlg.h orlg_step*) asks the device for: the entry
// kind and the caller's route or policy, rule, gn_mode and n_steps, together with whether the handle has a gn_gate and whether that
// gate protects, resolve to the device's (policy, assign) or to a refusal.  Every check that needs no more than those inputs is here,
// each public value is mapped to the device's once, and the order of the checks is the order in which a call that is wrong in several
// ways is refused.  Comparisons only -- no HIP call, no handle -- so all of it runs without a device (orlg_debug_step_call); the
// entries and rmsa_step (orlg_api_step.hip) do what it says.
#pragma once
#include "../../include/orlg.h"
#include "orlg_device.h"   // ORLG_POLICY_*, ORLG_ASSIGN_*: the device's values behind the public ones

int orlg_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));   // orlg_host.h: the message of orlg_last_error

// orlg_step, orlg_step_gn, orlg_step_diag and orlg_step_gn_protect are one kind: a policy, the reference's first fit
enum OrlgStepEntry { ORLG_ENTRY_PLAIN, ORLG_ENTRY_ASSIGN, ORLG_ENTRY_MIN_CUT, ORLG_ENTRY_WINDOW, ORLG_ENTRY_RULE_GN, ORLG_NUM_STEP_ENTRIES };
// OrlgParams::policy and ::assign of the launch; assign != ORLG_ASSIGN_FIRST: an ASSIGN instantiation
struct OrlgStepCall { int32_t policy, assign; };
// policy: the entry's `policy` or `route`; rule: its `assign` or `rule` (orlg_step_assign, orlg_step_window, orlg_step_rule_gn);
// gn_mode: orlg_step_rule_gn's.  An entry without one of them leaves it 0
struct OrlgStepAsk { int32_t entry, policy, rule, gn_mode, n_steps; bool gated, protect; };   // entry: OrlgStepEntry

// a route names paths and leaves the slot to a rule
static inline bool orlg_is_route(int32_t v) {
    return v == ORLG_POLICY_SP_FF || v == ORLG_POLICY_SAP_FF || v == ORLG_POLICY_LLP_FF || v == ORLG_POLICY_PATH_FF_EXTERNAL;
}
// the four window rules of orlg_step_assign other than the reference's first fit
static inline bool orlg_is_window_rule(int32_t v) {
    return v == ORLG_ASSIGN_FIRST_FULL || v == ORLG_ASSIGN_LAST || v == ORLG_ASSIGN_BEST || v == ORLG_ASSIGN_EXACT;
}
static inline int32_t orlg_device_policy(int32_t route, int32_t gn_mode = ORLG_GN_MODE_CHECK) {
    return route == ORLG_ROUTE_FEWEST_CUTS   ? (int32_t)ORLG_POLICY_MIN_CUT
           : route == ORLG_ROUTE_BEST_WINDOW ? (int32_t)ORLG_POLICY_BEST_WINDOW
           : gn_mode == ORLG_GN_MODE_NEXT_PATH ? (int32_t)ORLG_POLICY_SAP_GN   // (the route sap_ff that goes on to the next path)
                                               : route;
}
static inline int32_t orlg_device_assign(int32_t rule) {
    return rule == ORLG_RULE_MOST_USED ? (int32_t)ORLG_ASSIGN_MOST_USED : rule == ORLG_RULE_FEWEST_CUTS ? (int32_t)ORLG_ASSIGN_MIN_CUT : rule;
}

// orlg_step_max_margin: a call of its own beside the entries above -- no OrlgStepEntry, and the policies they accept stay
// what they were.  route: the caller's; actions: the caller gave an action array.  The launch's own refusal, a ring of compacted
// services that does not fit the LDS, needs the handle's layout and is orlg_api_step.hip's.
struct OrlgStepMmAsk { int32_t route, n_steps; bool gated, actions; };
static inline int orlg_step_mm_call(const OrlgStepMmAsk &a, OrlgStepCall *call) {
    if (!a.gated) return orlg_fail(ORLG_ERR_INVALID, "orlg_step_max_margin: the handle has no gn_gate (the margin is the admission check's)");
    if (a.route != ORLG_POLICY_SAP_FF && a.route != ORLG_ROUTE_BEST_WINDOW && a.route != ORLG_POLICY_PATH_FF_EXTERNAL)
        return orlg_fail(ORLG_ERR_INVALID, "orlg_step_max_margin needs a route (ORLG_POLICY_SAP_FF, ORLG_ROUTE_BEST_WINDOW or ORLG_POLICY_PATH_FF_EXTERNAL): got %d", a.route);
    if (a.n_steps < 1) return orlg_fail(ORLG_ERR_INVALID, "n_steps must be >= 1");
    if (a.route == ORLG_POLICY_PATH_FF_EXTERNAL && !a.actions)
        return orlg_fail(ORLG_ERR_INVALID, "orlg_step_max_margin: the route ORLG_POLICY_PATH_FF_EXTERNAL needs an action array");
    *call = {orlg_device_policy(a.route), ORLG_ASSIGN_FIRST};
    return ORLG_OK;
}

static inline int orlg_step_call(const OrlgStepAsk &a, OrlgStepCall *call) {
    const int32_t route = a.policy, rule = a.rule;
    const char *const steps = "n_steps must be >= 1";
    switch (a.entry) {
    case ORLG_ENTRY_PLAIN:
    case ORLG_ENTRY_ASSIGN:
        if (a.n_steps < 1) return orlg_fail(ORLG_ERR_INVALID, "%s", steps);
        if (a.policy < ORLG_POLICY_EXTERNAL || a.policy > ORLG_POLICY_SAP_FF_GN) return orlg_fail(ORLG_ERR_INVALID, "unknown policy %d", a.policy);
        if (a.policy == ORLG_POLICY_SAP_FF_GN && !a.gated)
            return orlg_fail(ORLG_ERR_INVALID, "policy %d (sap_ff_gn) asks the GN-model admission check: the handle has no gn_gate", a.policy);
        *call = {a.policy, ORLG_ASSIGN_FIRST};
        if (a.entry == ORLG_ENTRY_PLAIN) return ORLG_OK;
        // the public rules: ORLG_ASSIGN_MIN_CUT and ORLG_ASSIGN_MOST_USED have entries of their own and are unknown to this one
        if (rule < ORLG_ASSIGN_FIRST || rule >= ORLG_NUM_ASSIGN_RULES) return orlg_fail(ORLG_ERR_INVALID, "unknown assignment rule %d", rule);
        if (rule == ORLG_ASSIGN_FIRST) return ORLG_OK;   // orlg_step_diag, and launches what that launches
        if (!orlg_is_route(a.policy))
            return orlg_fail(ORLG_ERR_INVALID, "assignment rule %d needs a route (sp_ff, sap_ff, llp_ff or path_ff_external): policy %d names its own slot or block", rule, a.policy);
        if (a.gated) return orlg_fail(ORLG_ERR_INVALID, "assignment rule %d on a handle with a gn_gate: this entry runs no rule behind the admission check, orlg_step_rule_gn does", rule);
        call->assign = rule;
        return ORLG_OK;
    case ORLG_ENTRY_MIN_CUT:
        if (!orlg_is_route(route) && route != ORLG_ROUTE_FEWEST_CUTS)
            return orlg_fail(ORLG_ERR_INVALID, "the fewest-cuts window needs a route (sp_ff, sap_ff, llp_ff, path_ff_external or ORLG_ROUTE_FEWEST_CUTS): got %d", route);
        if (a.gated) return orlg_fail(ORLG_ERR_INVALID, "the fewest-cuts window on a handle with a gn_gate: this entry runs no rule behind the admission check, orlg_step_rule_gn does");
        if (a.n_steps < 1) return orlg_fail(ORLG_ERR_INVALID, "%s", steps);
        *call = {orlg_device_policy(route), ORLG_ASSIGN_MIN_CUT};
        return ORLG_OK;
    case ORLG_ENTRY_WINDOW:   // (an old route with an old rule: what orlg_step_assign resolves them to)
        if (!orlg_is_route(route) && route != ORLG_ROUTE_BEST_WINDOW)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_window needs a route (sp_ff, sap_ff, llp_ff, path_ff_external or ORLG_ROUTE_BEST_WINDOW): got %d", route);
        if (!orlg_is_window_rule(rule) && rule != ORLG_RULE_MOST_USED)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_window needs a rule (ORLG_ASSIGN_FIRST_FULL, LAST, BEST, EXACT or ORLG_RULE_MOST_USED): got %d", rule);
        if (a.gated) return orlg_fail(ORLG_ERR_INVALID, "orlg_step_window on a handle with a gn_gate: this entry runs no rule behind the admission check (orlg_step_rule_gn does, for the rules and routes other than MOST_USED and BEST_WINDOW)");
        if (a.n_steps < 1) return orlg_fail(ORLG_ERR_INVALID, "%s", steps);
        *call = {orlg_device_policy(route), orlg_device_assign(rule)};
        return ORLG_OK;
    case ORLG_ENTRY_RULE_GN:   // a route and a rule behind the admission check: a GN x ASSIGN instantiation
        if (!a.gated) return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn: the handle has no gn_gate (orlg_step_assign, orlg_step_min_cut serve it)");
        if (a.protect)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn: the handle protects its running lightpaths (orlg_set_gn_protect), and no assignment rule runs behind that second check yet: orlg_step_gn_protect runs the reference's first fit behind it");
        if (route == ORLG_ROUTE_BEST_WINDOW || rule == ORLG_RULE_MOST_USED)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn: the rule MOST_USED and the route BEST_WINDOW are not served behind a gn_gate (route %d, rule %d)", route, rule);
        if (!orlg_is_route(route) && route != ORLG_ROUTE_FEWEST_CUTS)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn needs a route (sp_ff, sap_ff, llp_ff, path_ff_external or ORLG_ROUTE_FEWEST_CUTS): got %d", route);
        if (rule == ORLG_ASSIGN_FIRST)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn: rule ORLG_ASSIGN_FIRST is the reference's first fit, which orlg_step_gn runs behind the gate");
        if (!orlg_is_window_rule(rule) && rule != ORLG_RULE_FEWEST_CUTS)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn needs a rule (ORLG_ASSIGN_FIRST_FULL, LAST, BEST, EXACT or ORLG_RULE_FEWEST_CUTS): got %d", rule);
        if (a.gn_mode != ORLG_GN_MODE_CHECK && a.gn_mode != ORLG_GN_MODE_NEXT_PATH)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn: unknown gn_mode %d (ORLG_GN_MODE_CHECK or ORLG_GN_MODE_NEXT_PATH)", a.gn_mode);
        if (a.gn_mode == ORLG_GN_MODE_NEXT_PATH && route != ORLG_POLICY_SAP_FF)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn: ORLG_GN_MODE_NEXT_PATH goes with the route sap_ff only: got route %d", route);
        if (route == ORLG_ROUTE_FEWEST_CUTS && rule != ORLG_RULE_FEWEST_CUTS)
            return orlg_fail(ORLG_ERR_INVALID, "orlg_step_rule_gn: the route ORLG_ROUTE_FEWEST_CUTS ranks fewest-cuts windows, it needs the rule ORLG_RULE_FEWEST_CUTS: got %d", rule);
        if (a.n_steps < 1) return orlg_fail(ORLG_ERR_INVALID, "%s", steps);
        *call = {orlg_device_policy(route, a.gn_mode), orlg_device_assign(rule)};
        return ORLG_OK;
    default:
        return orlg_fail(ORLG_ERR_INVALID, "unknown step entry %d", a.entry);
    }
}
