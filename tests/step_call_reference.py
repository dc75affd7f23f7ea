"""What a call of a step entry point resolves to, written from the contract of the entries in ``include/orlg.h`` as allowed sets
per entry kind -- not from the resolver (csrc/orlg_step_call.h), which ``test_step_calls.py`` holds to it without a device and
``test_gpu_step_calls.py`` through the public entry points.

A call is (entry kind, policy or route, rule, gn_mode, n_steps, handle) with the handle one of "plain" (no gn_gate), "gated" and
"protect" (a gate that protects the running lightpaths).  ``expected`` gives (code, (policy, assign) of the device or None, a
substring that tells the refusal from every other refusal of the entry kind, or None).  Where a call is wrong in several ways the
refusal is the first of the entry's list, in the order the header documents them and the entries have always reported them: the
plain entries and orlg_step_assign begin with n_steps, the entries that take a route end with it."""
import itertools
import re

OK, INVALID = 0, -1
ENTRIES = ("plain", "assign", "min_cut", "window", "rule_gn")   # enum OrlgStepEntry; "plain": orlg_step, _gn, _diag, _gn_protect
HANDLES = ("plain", "gated", "protect")

EXTERNAL, SP_FF, SAP_FF, LLP_FF, DEEP_SP_FF, DEEP_SAP_FF, DEEP_EXTERNAL, PATH_FF_EXTERNAL, SAP_FF_GN = range(-1, 8)   # ORLG_POLICY_*
FIRST, FIRST_FULL, LAST, BEST, EXACT = range(5)                                                                     # ORLG_ASSIGN_*
ROUTE_FEWEST_CUTS, RULE_MOST_USED, ROUTE_BEST_WINDOW, RULE_FEWEST_CUTS = 100, 100, 101, 102
MODE_CHECK, MODE_NEXT_PATH = 0, 1
# the device's values behind the public ones (csrc/orlg_device.h)
DEV_SAP_GN, DEV_MIN_CUT_ROUTE, DEV_BEST_WINDOW, DEV_MIN_CUT, DEV_MOST_USED = 7, 8, 9, 5, 6

POLICIES = set(range(EXTERNAL, SAP_FF_GN + 1))
EXTERNAL_POLICIES = {EXTERNAL: 2, DEEP_EXTERNAL: 1, PATH_FF_EXTERNAL: 1}   # the ints per environment of their action arrays
ROUTES = {SP_FF, SAP_FF, LLP_FF, PATH_FF_EXTERNAL}
WINDOW_RULES = {FIRST_FULL, LAST, BEST, EXACT}

# the domain of the tests
DOMAIN = dict(policy=list(range(-2, 11)) + [100, 101, 102], rule=list(range(-1, 8)) + [100, 101, 102], gn_mode=[-1, 0, 1, 2],
              n_steps=[0, 1])


def calls(entry):
    """every call of an entry kind over DOMAIN; an argument the entry does not have is 0"""
    has_rule, has_mode = entry in ("assign", "window", "rule_gn"), entry == "rule_gn"
    for policy, rule, mode, n, handle in itertools.product(DOMAIN["policy"], DOMAIN["rule"] if has_rule else [0],
                                                            DOMAIN["gn_mode"] if has_mode else [0], DOMAIN["n_steps"], HANDLES):
        yield policy, rule, mode, n, handle


def _refuse(text):
    return INVALID, None, text


def expected(entry, policy, rule, mode, n_steps, handle):
    gated = handle != "plain"
    if entry in ("plain", "assign"):
        if n_steps < 1:
            return _refuse("n_steps must be >= 1")
        if policy not in POLICIES:
            return _refuse(f"unknown policy {policy}")
        if policy == SAP_FF_GN and not gated:
            return _refuse("the handle has no gn_gate")
        if entry == "plain":
            return OK, (policy, FIRST), None
        if rule not in {FIRST} | WINDOW_RULES:
            return _refuse(f"unknown assignment rule {rule}")
        if rule == FIRST:   # orlg_step_diag
            return OK, (policy, FIRST), None
        if policy not in ROUTES:
            return _refuse(f"assignment rule {rule} needs a route")
        if gated:
            return _refuse(f"assignment rule {rule} on a handle with a gn_gate")
        return OK, (policy, rule), None
    if entry == "min_cut":
        if policy not in ROUTES | {ROUTE_FEWEST_CUTS}:
            return _refuse(f"the fewest-cuts window needs a route (sp_ff, sap_ff, llp_ff, path_ff_external or ORLG_ROUTE_FEWEST_CUTS): got {policy}")
        if gated:
            return _refuse("the fewest-cuts window on a handle with a gn_gate")
        if n_steps < 1:
            return _refuse("n_steps must be >= 1")
        return OK, (DEV_MIN_CUT_ROUTE if policy == ROUTE_FEWEST_CUTS else policy, DEV_MIN_CUT), None
    if entry == "window":
        if policy not in ROUTES | {ROUTE_BEST_WINDOW}:
            return _refuse(f"orlg_step_window needs a route (sp_ff, sap_ff, llp_ff, path_ff_external or ORLG_ROUTE_BEST_WINDOW): got {policy}")
        if rule not in WINDOW_RULES | {RULE_MOST_USED}:
            return _refuse(f"orlg_step_window needs a rule (ORLG_ASSIGN_FIRST_FULL, LAST, BEST, EXACT or ORLG_RULE_MOST_USED): got {rule}")
        if gated:
            return _refuse("orlg_step_window on a handle with a gn_gate")
        if n_steps < 1:
            return _refuse("n_steps must be >= 1")
        return OK, (DEV_BEST_WINDOW if policy == ROUTE_BEST_WINDOW else policy, DEV_MOST_USED if rule == RULE_MOST_USED else rule), None
    assert entry == "rule_gn"
    if not gated:
        return _refuse("orlg_step_rule_gn: the handle has no gn_gate")
    if handle == "protect":
        return _refuse("orlg_step_rule_gn: the handle protects its running lightpaths")
    if policy == ROUTE_BEST_WINDOW or rule == RULE_MOST_USED:
        return _refuse(f"are not served behind a gn_gate (route {policy}, rule {rule})")
    if policy not in ROUTES | {ROUTE_FEWEST_CUTS}:
        return _refuse(f"orlg_step_rule_gn needs a route (sp_ff, sap_ff, llp_ff, path_ff_external or ORLG_ROUTE_FEWEST_CUTS): got {policy}")
    if rule == FIRST:
        return _refuse("orlg_step_rule_gn: rule ORLG_ASSIGN_FIRST is the reference's first fit")
    if rule not in WINDOW_RULES | {RULE_FEWEST_CUTS}:
        return _refuse(f"orlg_step_rule_gn needs a rule (ORLG_ASSIGN_FIRST_FULL, LAST, BEST, EXACT or ORLG_RULE_FEWEST_CUTS): got {rule}")
    if mode not in (MODE_CHECK, MODE_NEXT_PATH):
        return _refuse(f"orlg_step_rule_gn: unknown gn_mode {mode}")
    if mode == MODE_NEXT_PATH and policy != SAP_FF:
        return _refuse(f"ORLG_GN_MODE_NEXT_PATH goes with the route sap_ff only: got route {policy}")
    if policy == ROUTE_FEWEST_CUTS and rule != RULE_FEWEST_CUTS:
        return _refuse(f"it needs the rule ORLG_RULE_FEWEST_CUTS: got {rule}")
    if n_steps < 1:
        return _refuse("n_steps must be >= 1")
    dev_policy = DEV_MIN_CUT_ROUTE if policy == ROUTE_FEWEST_CUTS else DEV_SAP_GN if mode == MODE_NEXT_PATH else policy
    return OK, (dev_policy, DEV_MIN_CUT if rule == RULE_FEWEST_CUTS else rule), None


def device_cases(entry):
    """the calls of an entry kind that go through the public entry points on a device: every accepted call of DOMAIN (n_steps 1) and
    the first call of every distinct refusal"""
    seen, out = set(), []
    for call in calls(entry):
        code, _, text = expected(entry, *call)
        if code == OK or refusal_kind(text) not in seen:
            out.append(call)
            seen.add(None if code == OK else refusal_kind(text))
    return out


# the public entry points of an entry kind, and their arguments behind the handle (io, diag and the extra outputs: NULL)
ENTRY_POINTS = {"plain": ("orlg_step", "orlg_step_gn", "orlg_step_diag", "orlg_step_gn_protect"), "assign": ("orlg_step_assign",),
                "min_cut": ("orlg_step_min_cut",), "window": ("orlg_step_window",), "rule_gn": ("orlg_step_rule_gn",)}
_PLAIN_TAIL = {"orlg_step": (), "orlg_step_gn": (None,), "orlg_step_diag": (None,), "orlg_step_gn_protect": (None, None)}


def call_entry(L, h, name, policy, rule, mode, n_steps, actions):
    """one call of a public step entry point with auto_reset; returns the code"""
    f = getattr(L, name)
    if name in _PLAIN_TAIL:
        return f(h, policy, n_steps, actions, 1, None, *_PLAIN_TAIL[name])
    if name == "orlg_step_min_cut":
        return f(h, policy, n_steps, actions, 1, None, None)
    if name == "orlg_step_rule_gn":
        return f(h, policy, rule, mode, n_steps, actions, 1, None, None)
    return f(h, policy, rule, n_steps, actions, 1, None, None)   # orlg_step_assign, orlg_step_window


def refusal_kind(text):
    """a refusal's text without the values it names: two refusals of an entry kind are the same refusal when this is equal"""
    return re.sub(r"-?\d+", "#", text)
