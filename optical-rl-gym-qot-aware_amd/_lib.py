"""ctypes binding of liborlg.so (include/orlg.h).  The library is built in-tree by build.py; there is
no Python or CPU fallback -- if the shared object is missing it is built, and if no HIP device is
visible ``orlg_create`` fails and :class:`OrlgError` is raised."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORLG_LIB_PATH") or os.path.join(HERE, "liborlg.so")  # ORLG_LIB_PATH: debug builds (tools/)

ORLG_OK = 0
ERR_NAMES = {-1: "ORLG_ERR_INVALID", -2: "ORLG_ERR_NO_DEVICE", -3: "ORLG_ERR_HIP", -4: "ORLG_ERR_QUEUE_FULL"}

STATS_LEVELS = {"counters": 0, "network": 1, "full": 2}
POLICIES = {"external": -1, "sp_ff": 0, "sap_ff": 1, "llp_ff": 2, "deeprmsa_sp_ff": 3, "deeprmsa_sap_ff": 4,
            "deeprmsa_external": 5, "path_ff_external": 6, "sap_ff_gn": 7}
# include/orlg.h ORLG_ASSIGN_*: where on a route's path the service starts (not in the reference, whose heuristics are first fit
# only, rmsa_env.py:854-937).  "first" is the reference's, with its bound range(0, S - n); the others use every window 0 .. S - n
ASSIGN_RULES = ("first", "first_full", "last", "best", "exact")
_ASSIGN_SUFFIX = {"first_full": "ff_full", "last": "lf", "best": "bf", "exact": "ef"}
# policy name -> (route: the ORLG_POLICY_* that orlg_step_assign reads as one, rule): sp / sap / llp x the four rules, and the
# agent's path x the four rules
ASSIGN_POLICIES = {f"{route}_{suffix}": (POLICIES[route + "_ff"], ASSIGN_RULES.index(rule))
                   for route in ("sp", "sap", "llp") for rule, suffix in _ASSIGN_SUFFIX.items()}
ASSIGN_POLICIES.update({f"path_{suffix}_external": (POLICIES["path_ff_external"], ASSIGN_RULES.index(rule))
                        for rule, suffix in _ASSIGN_SUFFIX.items()})
# include/orlg.h orlg_step_min_cut: the window with the fewest cuts (the links on which it splits a free block in two; DESIGN 2.24,
# not in the reference for these environments).  policy name -> the route orlg_step_min_cut takes: sp / sap / llp and the agent's
# path as above, and "min_cut" = ORLG_ROUTE_FEWEST_CUTS, of all k paths the one whose fewest-cuts window has the fewest cuts.  A
# table of its own: ASSIGN_POLICIES, ASSIGN_RULES and policy_ids answer for the names they always answered for
ROUTE_FEWEST_CUTS = 100
CUT_POLICIES = {"sp_mc": POLICIES["sp_ff"], "sap_mc": POLICIES["sap_ff"], "llp_mc": POLICIES["llp_ff"], "min_cut": ROUTE_FEWEST_CUTS,
                "path_mc_external": POLICIES["path_ff_external"]}
# include/orlg.h orlg_step_window: the rule MOST_USED (the window whose slots are occupied on the most links of the whole network)
# and the route BEST_WINDOW (of all k paths the one whose rule window ranks best by the rule's own order); DESIGN 2.25, not in the
# reference.  policy name -> (route, rule) as orlg_step_window takes them.  A table of its own, as CUT_POLICIES
RULE_MOST_USED = 100
ROUTE_BEST_WINDOW = 101
WINDOW_POLICIES = {"sp_mu": (POLICIES["sp_ff"], RULE_MOST_USED), "sap_mu": (POLICIES["sap_ff"], RULE_MOST_USED),
                   "llp_mu": (POLICIES["llp_ff"], RULE_MOST_USED), "path_mu_external": (POLICIES["path_ff_external"], RULE_MOST_USED),
                   "any_ff_full": (ROUTE_BEST_WINDOW, ASSIGN_RULES.index("first_full")),
                   "any_lf": (ROUTE_BEST_WINDOW, ASSIGN_RULES.index("last")), "any_bf": (ROUTE_BEST_WINDOW, ASSIGN_RULES.index("best")),
                   "any_ef": (ROUTE_BEST_WINDOW, ASSIGN_RULES.index("exact")), "any_mu": (ROUTE_BEST_WINDOW, RULE_MOST_USED)}
# include/orlg.h orlg_step_rule_gn / orlg_gn_path_windows: a route and a rule behind the GN-model admission check.  The
# fewest-cuts window as a rule of these two entries, the two modes, and the rule names the query takes.  No policy names: the
# names of ASSIGN_POLICIES and CUT_POLICIES run through them with ``run(..., gn_rule=)``
RULE_FEWEST_CUTS = 102
GN_RULE_MODES = {"check": 0, "next_path": 1}
GN_PATH_WINDOW_RULES = {"first": 0, "first_full": 1, "last": 2, "best": 3, "exact": 4, "min_cut": RULE_FEWEST_CUTS}
# include/orlg.h orlg_step_max_margin: the admitted window with the largest worst margin, found inside the step (a
# handle with gn_gate= only).  The names, and the route each one is to that entry.  Tables of their own, as CUT_POLICIES
MAX_MARGIN_POLICIES = ("sap_mm", "any_mm", "path_mm_external")
MAX_MARGIN_ROUTES = {"sap_mm": POLICIES["sap_ff"], "any_mm": ROUTE_BEST_WINDOW, "path_mm_external": POLICIES["path_ff_external"]}
# include/orlg.h orlg_set_gn_modulation / orlg_step_modulation: a gate that chooses the spectral efficiency a service runs at from the
# GSNR (a handle with gn_gate=rmsa_gn_gate_parameters(..., modulation="adaptive") only).  The gate's modes, the policy names
# that walk the levels and the value each one is to that entry.  Tables of their own, as CUT_POLICIES
GN_MODULATION_MODES = {"path": 0, "adaptive": 1}
ADAPTIVE_POLICIES = ("sp_ff_am", "sap_ff_am", "path_am_external", "external_am")
ADAPTIVE_POLICY_IDS = {"sp_ff_am": 200, "sap_ff_am": 201, "path_am_external": 202, "external_am": 203}
MAX_MODULATION_LEVELS = 6     # the modulation factors of the GN model end at spectral efficiency 6
MAX_ADAPTIVE_PATHS = 2048     # a service's level takes 3 bits of its descriptor's 14-bit path field


def policy_ids(policy):
    """(ORLG_POLICY_*, ORLG_ASSIGN_*) of a policy name: the reference's policies with rule 0, the names of ``ASSIGN_POLICIES``
    with theirs.  ``KeyError`` for an unknown name."""
    if policy in ASSIGN_POLICIES:
        return ASSIGN_POLICIES[policy]
    return POLICIES[policy], 0


class OrlgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class Topology(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("num_links", C.c_int32), ("k_paths", C.c_int32), ("num_paths", C.c_int32),
                ("pair_path_base", C.c_void_p), ("pair_path_count", C.c_void_p), ("path_hops", C.c_void_p),
                ("path_se", C.c_void_p), ("path_length", C.c_void_p), ("path_link_off", C.c_void_p),
                ("path_links", C.c_void_p)]


STEP_KERNELS = {"auto": 0, "wave": 1, "group": 2}   # include/orlg.h ORLG_KERNEL_*


class RmsaConfig(C.Structure):
    _fields_ = [("num_slots", C.c_int32), ("episode_length", C.c_int32), ("num_bit_rates", C.c_int32),
                ("j", C.c_int32), ("reward_mode", C.c_int32), ("queue_capacity", C.c_int32),
                ("stats_level", C.c_int32), ("step_kernel", C.c_int32),
                ("arrival_lambda", C.c_double), ("holding_lambda", C.c_double), ("channel_width", C.c_double),
                ("bit_rates", C.c_void_p), ("bit_rate_cum", C.c_void_p), ("src_cum", C.c_void_p),
                ("dst_cum", C.c_void_p)]


class StepIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("act_path", "act_slot", "accepted", "done", "reward", "request", "arrival",
                                         "holding", "network_compactness", "network_compactness_difference",
                                         "avg_link_compactness", "avg_link_utilization")]


# numpy dtypes of the step outputs
STEP_IO_DTYPES = {"act_path": "int32", "act_slot": "int32", "accepted": "uint8", "done": "uint8", "reward": "float64",
                  "request": "int32", "arrival": "float64", "holding": "float64", "network_compactness": "float64",
                  "network_compactness_difference": "float64", "avg_link_compactness": "float64",
                  "avg_link_utilization": "float64"}

# include/orlg.h ORLG_CAUSE_* / ORLG_FIT_*: why a step refused its request, and how far a candidate path is from fitting it
BLOCK_CAUSES = ("accepted", "capacity", "contiguity", "alignment", "last_window", "policy", "gn")
NUM_CAUSES = 8   # ORLG_NUM_CAUSES: the row length of cause_counts (code 7 is unused, always 0)
FIT_LEVELS = ("capacity", "contiguity", "alignment", "last_window", "fit")


class StepDiag(C.Structure):   # include/orlg.h struct orlg_step_diag
    _fields_ = [("block_cause", C.c_void_p), ("cause_counts", C.c_void_p), ("gn_gsnr_db", C.c_void_p)]


class Traffic(C.Structure):   # include/orlg.h orlg_traffic
    _fields_ = [("arrival_lambda", C.c_void_p), ("holding_lambda", C.c_void_p), ("group", C.c_void_p),
                ("num_groups", C.c_int32)]


class Trace(C.Structure):   # include/orlg.h orlg_trace
    _fields_ = [("length", C.c_int64), ("arrival", C.c_void_p), ("holding", C.c_void_p), ("src", C.c_void_p),
                ("dst", C.c_void_p), ("bit_rate", C.c_void_p), ("group", C.c_void_p), ("num_groups", C.c_int32)]


class PhyConfig(C.Structure):
    _fields_ = [("num_channels", C.c_int32), ("episode_length", C.c_int32), ("num_bit_rates", C.c_int32),
                ("k_table", C.c_int32), ("num_table_rows", C.c_int32), ("queue_capacity", C.c_int32),
                ("grooming", C.c_int32), ("channel_state_capacity", C.c_int32),
                ("defrag_period", C.c_int32), ("number_moves", C.c_int32), ("defrag_metric", C.c_int32),
                ("defrag_capacity", C.c_int32),
                ("arrival_lambda", C.c_double), ("holding_lambda", C.c_double)] + \
               [(n, C.c_void_p) for n in ("bit_rates", "bit_rate_cum", "src_cum", "dst_cum", "pair_table_row",
                                          "modulation_level", "gsnr", "adj_off", "adj_link", "adj_weight",
                                          "path_node_weights", "node_degree", "link_ends", "gn_gate")]


class GnGate(C.Structure):
    _fields_ = [("launch_power_w", C.c_double), ("channel_bandwidth_hz", C.c_double), ("attenuation_normalized", C.c_double),
                ("noise_figure", C.c_double), ("channel_center_frequency_hz", C.c_void_p), ("link_num_spans", C.c_void_p),
                ("link_span_length_km", C.c_void_p), ("thresholds_db", C.c_void_p), ("num_thresholds", C.c_int32),
                ("pad", C.c_int32)]


class RmsaGnGate(C.Structure):   # include/orlg.h orlg_rmsa_gn_gate
    _fields_ = [("launch_power_density_w_hz", C.c_double), ("frequency_start_hz", C.c_double), ("slot_width_hz", C.c_double),
                ("attenuation_normalized", C.c_double), ("noise_figure", C.c_double), ("link_num_spans", C.c_void_p),
                ("link_span_length_km", C.c_void_p), ("thresholds_db", C.c_void_p), ("num_thresholds", C.c_int32)]


class GnAuditSummary(C.Structure):   # include/orlg.h orlg_gn_audit_summary
    _fields_ = [("n_running", C.c_int32), ("n_below", C.c_int32), ("worst_rank", C.c_int32), ("pad", C.c_int32),
                ("min_margin_db", C.c_double)]


# the same record as a numpy dtype: the [B] summaries of orlg_gn_audit
GN_AUDIT_SUMMARY_DTYPE = [("n_running", "<i4"), ("n_below", "<i4"), ("worst_rank", "<i4"), ("pad", "<i4"), ("min_margin_db", "<f8")]


class PhyStepIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("act_path", "n_channels", "channels", "accepted", "done", "request",
                                         "arrival", "holding", "number_cuts_total", "rss_total_metric",
                                         "channels_used", "defrag_counters", "gn_gsnr_db")]


PHY_MAX_CHANNELS = 14
PHY_STEP_IO_DTYPES = {"act_path": "int32", "n_channels": "int32", "channels": "int16", "accepted": "uint8",
                      "done": "uint8", "request": "int32", "arrival": "float64", "holding": "float64",
                      "number_cuts_total": "float64", "rss_total_metric": "float64", "channels_used": "int16",
                      "defrag_counters": "int32", "gn_gsnr_db": "float64"}
PHY_POLICIES = {"external": -1, "bmfa": 0, "bmfa_rss": 1, "sapff": 2, "bmff": 3, "sapbm": 4, "faff": 5, "faff_rss": 6}

def _prototypes():
    """name -> (restype or None, argtypes or None) of every function include/orlg.h declares; None leaves ctypes' default
    (an int result; arguments converted as they come).  What works on the handle core both C APIs share exists under both
    prefixes with one prototype; ``_handle.BatchedHandle`` is written against those."""
    P, vp, i32, i64, u64 = C.POINTER, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    t = {"orlg_abi_version": (C.c_int, None), "orlg_last_error": (C.c_char_p, None), "orlg_device_count": (C.c_int, None),
         "orlg_host_log": (C.c_double, [C.c_double]),
         "orlg_gn_osnr": (None, None)}   # (its argtypes are set next to its struct, osnr.py)
    for p, config in (("orlg_", RmsaConfig), ("orlg_phy_", PhyConfig)):
        create = [P(Topology), P(config), i32, vp, u64, i32]
        t.update({p + "create": (None, create + [P(vp)]),
                  p + "create_traffic": (None, create + [P(Traffic), P(vp)]),   # per-environment traffic (orlg_traffic)
                  p + "create_trace": (None, [P(Topology), P(config), i32, i32, P(Trace), P(vp)]),   # request traces (orlg_trace)
                  p + "destroy": (None, [vp]), p + "set_stream": (None, [vp, vp]), p + "synchronize": (None, [vp]),
                  p + "last_kernel": (None, [vp, C.c_char_p, i32]), p + "reset": (None, [vp, i32]),
                  p + "reseed": (None, [vp, vp, u64]), p + "trace_length": (i64, [vp]), p + "trace_position": (i64, [vp]),
                  p + "words_per_link": (None, [vp]), p + "num_groups": (None, [vp]), p + "state_size": (i64, [vp]),
                  p + "get_traffic": (None, [vp, vp, vp, vp])})
        for name in ("get_requests", "get_counters", "get_current_time", "get_num_running", "get_occupancy", "save_state",
                     "load_state", "reduce_counters", "reduce_counters_grouped"):
            t[p + name] = (None, [vp, vp])
    # RMSA / DeepRMSA only
    t.update({"orlg_step": (None, [vp, i32, i32, vp, i32, P(StepIO)]), "orlg_launch_info": (None, [vp, vp]),
              "orlg_get_link_stats": (None, [vp, vp, vp, vp, vp]), "orlg_get_graph_stats": (None, [vp, vp, vp, vp]),
              "orlg_get_bit_rate_hist": (None, [vp, vp, vp, vp, vp]), "orlg_get_episodes_done": (None, [vp, vp]),
              "orlg_query_path_masks": (None, [vp, i32, vp, vp]), "orlg_query_path_mask": (None, [vp, i32, i32, vp, vp]),
              "orlg_deeprmsa_observation": (None, [vp, vp]), "orlg_deeprmsa_observation_f32": (None, [vp, vp]),
              "orlg_deeprmsa_obs_dim": (None, [vp]), "orlg_simple_matrix_observation": (None, [vp, vp]),
              "orlg_simple_matrix_obs_dim": (None, [vp]),
              # valid-action masks for the whole batch
              "orlg_set_allow_rejection": (None, [vp, i32]), "orlg_deeprmsa_mask_dim": (None, [vp]),
              "orlg_deeprmsa_observation_masked": (None, [vp, vp, i32, vp]), "orlg_action_masks": (None, [vp, vp, vp]),
              # GN-model admission check inside the step
              "orlg_set_gn_gate": (None, [vp, P(RmsaGnGate)]),
              "orlg_step_gn": (None, [vp, i32, i32, vp, i32, P(StepIO), vp]),
              # ... that also protects the running lightpaths: the switch, and the step with the neighbour margin
              "orlg_set_gn_protect": (None, [vp, i32]),
              "orlg_step_gn_protect": (None, [vp, i32, i32, vp, i32, P(StepIO), P(StepDiag), vp]),
              # valid-action masks that know the admission check
              "orlg_gn_action_masks": (None, [vp, vp, vp, vp, vp]),
              # blocking cause per step, fit level per candidate path
              "orlg_step_diag": (None, [vp, i32, i32, vp, i32, P(StepIO), P(StepDiag)]),
              "orlg_path_fit_levels": (None, [vp, vp]),
              # spectrum-assignment rules beyond the reference's first fit
              "orlg_step_assign": (None, [vp, i32, i32, i32, vp, i32, P(StepIO), P(StepDiag)]),
              # the window with the fewest cuts: the step under it, and every candidate path's such window
              "orlg_step_min_cut": (None, [vp, i32, i32, vp, i32, P(StepIO), P(StepDiag)]),
              "orlg_path_min_cuts": (None, [vp, vp, vp]),
              # most-used windows and the best window over all paths: the step, the slot usage, every path's most-used window
              "orlg_step_window": (None, [vp, i32, i32, i32, vp, i32, P(StepIO), P(StepDiag)]),
              "orlg_slot_usage": (None, [vp, vp]),
              "orlg_path_most_used": (None, [vp, vp, vp]),
              # assignment rules behind the GN-model admission check: the step, every path's rule window and its GSNR
              "orlg_step_rule_gn": (None, [vp, i32, i32, i32, i32, vp, i32, P(StepIO), P(StepDiag)]),
              "orlg_gn_path_windows": (None, [vp, i32, vp, vp, vp]),
              # the running services of every environment and their GN-model audit
              "orlg_queue_capacity": (None, [vp]),
              "orlg_get_running_services": (None, [vp, vp, vp, vp, vp, vp, vp, vp]),
              "orlg_gn_audit": (None, [vp, P(RmsaGnGate), vp, vp, vp, vp, vp]),
              # the masks and rule windows that know both halves of the admission check (a protecting handle's too)
              "orlg_gn_admission_masks": (None, [vp, vp, vp, vp, vp, vp, vp]),
              "orlg_gn_admission_windows": (None, [vp, i32, vp, vp, vp, vp]),
              # ... over every start slot of every path: mask words, GSNR and margin rows, the window with the largest worst margin
              "orlg_gn_admission_slots": (None, [vp, vp, vp, vp, vp, vp]),
              "orlg_step_max_margin": (None, [vp, i32, i32, vp, i32, P(StepIO), P(StepDiag), vp]),
              "orlg_step_max_margin_protect": (None, [vp, i32, i32, vp, i32, P(StepIO), P(StepDiag), vp, vp]),
              # a gate that chooses the modulation from the GSNR: the mode, the step that walks the levels, every level of every path,
              # the running services with the spectral efficiency each one runs at
              "orlg_set_gn_modulation": (None, [vp, i32]),
              "orlg_step_modulation": (None, [vp, i32, i32, vp, i32, P(StepIO), vp, vp]),
              "orlg_gn_modulation_windows": (None, [vp, vp, vp, vp, vp]),
              "orlg_get_running_services_se": (None, [vp, vp, vp, vp, vp, vp, vp, vp, vp])})
    # QoT-aware only
    t.update({"orlg_phy_step": (None, [vp, i32, i32, vp, vp, i32, P(PhyStepIO)]), "orlg_phy_node_vectors": (None, [vp]),
              "orlg_phy_get_episode_stats": (None, [vp, vp]), "orlg_phy_channel_masks": (None, [vp, vp]),
              "orlg_phy_get_channel_state": (None, [vp, i32, vp, vp]), "orlg_phy_channel_state_capacity": (None, [vp]),
              # bit_rate_selection="continuous": float64 shares
              "orlg_phy_continuous": (None, [vp]),
              "orlg_phy_step_ex": (None, [vp, i32, i32, vp, vp, vp, i32, P(PhyStepIO), vp, vp]),
              "orlg_phy_get_channel_state_f64": (None, [vp, i32, vp, vp]),
              "orlg_phy_load_state_checked": (None, [vp, vp, i64])})
    return t


PROTOTYPES = _prototypes()
EXPORTED_SYMBOLS = list(PROTOTYPES)

_lib = None


def load(build_if_missing=True):
    """Load liborlg.so, building it with hipcc first when it is missing or stale, and give every function its prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing and not os.environ.get("ORLG_LIB_PATH"):
        from . import build as _build
        if _build.needs_build():
            _build.build(verbose=False)
    if not os.path.exists(LIB_PATH):
        raise OrlgError(-2, f"{LIB_PATH} is missing: run python optical-rl-gym-qot-aware_amd/build.py (needs hipcc)")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(L, name)
        if restype is not None:
            f.restype = restype
        if argtypes is not None:
            f.argtypes = argtypes
    _lib = L
    return L


def check(rc):
    if rc != ORLG_OK:
        raise OrlgError(rc, load().orlg_last_error().decode())
