"""BatchedRMSAEnv: B independent RMSA / DeepRMSA environments stepped on one MI355X.

Constructor kwargs are the reference's (``rmsa_env.py:29-53``, ``deeprmsa_env.py:10-32``) plus
``batch_size`` / ``device`` / ``stats_level`` / ``queue_capacity``.  Environment ``i`` is seeded with
``seed + i`` (or ``seeds[i]``), i.e. it replays ``RMSAEnv(..., seed=seed + i)`` of the reference.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib, osnr as _osnr, trace as _trace
from ._handle import COUNTER_NAMES, REQUEST_DTYPE, SweepTraffic  # noqa: F401  (their import path: bench.py, tools/, tests)
from ._handle import BatchedHandle, _check_buffer, _dtype_name, _output_names, _ptr

DEFAULT_BIT_RATES = (200, 250, 300, 350, 400, 450, 500, 550, 600, 650, 700, 750, 800, 850, 900, 950, 1000, 1050,
                     1100, 1150, 1200)  # rmsa_env.py:37-38

_STEP_IO_SHAPES = {"request": (4,)}   # per-step outputs wider than [n_steps, B]


class BatchedRMSAEnv(BatchedHandle):
    PREFIX = "orlg_"

    def __init__(self, topology, batch_size: int, *, episode_length: int = 1000, load: float = None,
                 mean_service_holding_time: float = None, num_spectrum_resources: int = 100,
                 bit_rate_selection: str = "discrete", bit_rates: Sequence[int] = DEFAULT_BIT_RATES,
                 bit_rate_probabilities=None, node_request_probabilities=None, seed: Optional[int] = None,
                 seeds=None, allow_rejection: bool = False, channel_width: float = 12.5, j: int = 1,
                 reward_mode: int = 0, stats_level: str = "full", queue_capacity: int = 0, device: int = 0,
                 step_kernel: str = "auto", bit_rate_lower_bound=25, bit_rate_higher_bound=100, groups=None,
                 num_groups=None, trace=None, gn_gate=None):
        load, mean_service_holding_time = self._init_traffic_kwargs(trace, load, mean_service_holding_time, seed, seeds)
        # GN-model GSNR admission check inside the step (osnr.rmsa_gn_gate_parameters; not in the reference: include/orlg.h
        # orlg_rmsa_gn_gate).  Checked before the library is loaded
        self.gn_gate = None if gn_gate is None else _osnr.check_rmsa_gn_gate(gn_gate, topology, step_kernel)
        if bit_rate_selection not in ("continuous", "discrete"):   # rmsa_env.py:74
            raise ValueError("bit_rate_selection must be 'continuous' or 'discrete'")
        self.bit_rate_selection = bit_rate_selection
        if bit_rate_selection == "continuous":
            # rmsa_env.py:95-101: rng.randint(lower, higher) -- every integer rate of the range, drawn by rejection on the device
            lo, hi = int(bit_rate_lower_bound), int(bit_rate_higher_bound)
            if lo != bit_rate_lower_bound or hi != bit_rate_higher_bound or hi < lo:
                raise ValueError("bit_rate_lower_bound / bit_rate_higher_bound must be integers, lower <= higher (random.randint)")
            if hi - lo + 1 > 256:
                raise ValueError("continuous bit rates: at most 256 integer rates (lower .. higher)")
            self.bit_rate_lower_bound, self.bit_rate_higher_bound = lo, hi
            bit_rates, bit_rate_probabilities = list(range(lo, hi + 1)), None
        tables = self._open(topology, batch_size, episode_length, load, mean_service_holding_time, bit_rates,
                            bit_rate_selection == "continuous", bit_rate_probabilities, node_request_probabilities, seed,
                            groups, num_groups)
        self.num_spectrum_resources = int(num_spectrum_resources)
        self.j = int(j)
        self.allow_rejection = bool(allow_rejection)
        self.reject_action = 1 if allow_rejection else 0
        self.channel_width = float(channel_width)
        self.stats_level = stats_level
        cc = _lib.RmsaConfig()
        cc.num_slots, cc.episode_length, cc.num_bit_rates = self.num_spectrum_resources, self.episode_length, len(self.bit_rates)
        cc.j, cc.reward_mode, cc.queue_capacity = self.j, int(reward_mode), int(queue_capacity)
        cc.stats_level = _lib.STATS_LEVELS[stats_level]
        cc.step_kernel = _lib.STEP_KERNELS[step_kernel]
        cc.channel_width = self.channel_width
        self._fill_traffic(cc, *tables)
        self._create(self._topology_struct(), cc, seeds, device)
        self.obs_dim = self.L.orlg_deeprmsa_obs_dim(self.h)
        # the explicit rejection is one more column of the action masks (the step kernels need no flag: an action out of range
        # is a rejection either way)
        _lib.check(self.L.orlg_set_allow_rejection(self.h, self.reject_action))
        self.mask_dim = self.L.orlg_deeprmsa_mask_dim(self.h)
        if self.gn_gate is not None:
            g, gg = self.gn_gate, _lib.RmsaGnGate()
            for name in ("launch_power_density_w_hz", "frequency_start_hz", "slot_width_hz", "attenuation_normalized", "noise_figure"):
                setattr(gg, name, float(g[name]))
            gg.link_num_spans = self._keep_array(g["link_num_spans"], np.int32)
            gg.link_span_length_km = self._keep_array(g["link_span_length_km"], np.float64)
            gg.thresholds_db, gg.num_thresholds = self._keep_array(g["thresholds_db"], np.float64), len(g["thresholds_db"])
            try:
                _lib.check(self.L.orlg_set_gn_gate(self.h, C.byref(gg)))
                if self.gn_protect:
                    _lib.check(self.L.orlg_set_gn_protect(self.h, 1))
                if self.gn_adaptive:
                    _lib.check(self.L.orlg_set_gn_modulation(self.h, _lib.GN_MODULATION_MODES["adaptive"]))
            except Exception:
                self.close()
                raise

    @property
    def gn_protect(self):
        """The gate also protects the running lightpaths (``rmsa_gn_gate_parameters(protect_running=True)``)."""
        return bool(self.gn_gate and self.gn_gate.get("protect_running"))

    @property
    def gn_adaptive(self):
        """The gate chooses the spectral efficiency a service runs at from the GSNR
        (``rmsa_gn_gate_parameters(modulation="adaptive")``)."""
        gate = getattr(self, "gn_gate", None)
        return bool(gate and gate.get("modulation") == "adaptive")

    @property
    def modulation_levels(self):
        """``M``: the levels an adaptive gate chooses among (its ``num_thresholds``), 0 on every other handle."""
        return len(self.gn_gate["thresholds_db"]) if self.gn_adaptive else 0

    def _refuse_adaptive(self, what, why):
        """``ValueError`` on a handle whose gate chooses the modulation, before the library is called: what DESIGN 2.33 leaves for later"""
        if self.gn_adaptive:
            raise ValueError(f"{what}: the handle's gate chooses the modulation (modulation='adaptive'); {why}")

    def launch_info(self):
        """Launch geometry of the step kernel (envs per workgroup, LDS bytes, resident workgroups per CU)."""
        a = np.zeros(4, np.int32)
        _lib.check(self.L.orlg_launch_info(self.h, _ptr(a)))
        return {"envs_per_workgroup": int(a[0]), "lds_bytes_per_workgroup": int(a[1]),
                "workgroups_per_cu": int(a[2]), "words_per_link": int(a[3])}

    # ------------------------------------------------------------------ stepping
    def run(self, policy: str, n_steps: int = 1, *, actions=None, auto_reset: bool = False,
            outputs: Sequence[str] = (), out: Optional[Dict[str, object]] = None, cause_counts=None, gn_rule=None):
        """``n_steps`` x (policy -> step) on the device.  ``outputs`` names per-step arrays to return
        (see ``_lib.STEP_IO_DTYPES``) as numpy arrays of shape [n_steps, B(, 4)]; ``out`` may supply
        preallocated numpy arrays or torch tensors (device tensors are written without staging).  ``"gn_gsnr_db"``: the GSNR
        the GN-model admission check compared (``gn_gate=``), NaN where no check ran; it leaves through ``orlg_step_gn``.

        Why a request was refused (``orlg_step_diag``; codes ``BLOCK_CAUSES``, include/orlg.h ``ORLG_CAUSE_*``):
        ``"block_cause"`` in ``outputs`` -- [n_steps, B] uint8, the cause of every step; ``cause_counts=True`` or a [B, 8] int32
        buffer -- ``"block_cause_counts"``, the steps of THIS launch per cause (the library zeroes the buffer; a row sums to
        ``n_steps``).  Either one makes the launch run the step kernel's instantiation with the classifier: the same steps,
        state and outputs, some percent slower.

        Assignment rules beyond the reference's first fit (``orlg_step_assign``; not in the reference): the policy
        names of ``_lib.ASSIGN_POLICIES`` -- a route ``sp`` / ``sap`` / ``llp`` (``rmsa_env.py:854-937``) with ``_ff_full`` (the
        lowest window of 0 .. S - n, the reference's first fit without its off-by-one), ``_lf`` (the highest window), ``_bf``
        (the shortest free block of >= n slots, ties to the lowest) or ``_ef`` (the lowest block of exactly n slots, else
        ``_ff_full``), and ``path_{ff_full,lf,bf,ef}_external`` (``actions`` [B] names the path; a path out of range or without
        a window is the rejection).  They run wherever ``sap_ff`` runs -- sweep and trace handles, both step kernels, with
        ``block_cause`` / ``cause_counts`` -- except on a handle with ``gn_gate=`` (``ValueError``).  A path has a window iff
        ``path_fit_levels() >= 3``: that query is the mask of the path-only action spaces.

        The window with the fewest cuts (``orlg_step_min_cut``; not in the reference for these environments): the
        names of ``_lib.CUT_POLICIES`` -- ``sp_mc`` / ``sap_mc`` / ``llp_mc`` (the routes above; on the path the window that
        splits a free block in two on the fewest links, ties to the lowest start), ``min_cut`` (of all k paths the one whose such
        window has the fewest cuts, ties to the lowest path) and ``path_mc_external`` (``actions`` [B] names the path).  They run
        where the names above run, with the same exception; :meth:`path_min_cuts` is the matching query.

        Most-used windows and the best window over all paths (``orlg_step_window``; not in the reference): the names
        of ``_lib.WINDOW_POLICIES`` -- ``sp_mu`` / ``sap_mu`` / ``llp_mu`` (the routes above; on the path the window whose slots
        are occupied on the most links of the whole network, ties to the lowest start), ``path_mu_external`` (``actions`` [B]
        names the path) and ``any_ff_full`` / ``any_lf`` / ``any_bf`` / ``any_ef`` / ``any_mu`` (every path proposes its rule
        window; the proposal that ranks best by the rule's own order wins, ties to the lowest path).  They run where the names
        above run, with the same exception; :meth:`slot_usage` and :meth:`path_most_used` are the matching queries.

        An assignment rule behind the admission check (``orlg_step_rule_gn``; not in the reference): ``gn_rule=`` on
        a handle with ``gn_gate=``, with a name of ``_lib.ASSIGN_POLICIES`` or ``_lib.CUT_POLICIES``.  ``"check"``: the route and
        the rule propose what they propose without a gate, the check runs once on that window, and a refusal is a gate refusal
        (not accepted, ``act_path`` / ``act_slot`` the proposal, ``gn_gsnr_db`` the value compared, cause ``"gn"``).
        ``"next_path"`` (the ``sap_*`` names only): the candidate paths in order, the first one whose rule window is admitted is
        provisioned -- ``sap_ff_gn`` with the rule's window in the first fit's place.  ``None``: everything above, unchanged.  The
        most-used rule and the ``any_*`` routes stay without a gate.  :meth:`path_rule_windows` is the matching query.

        A gate that protects the running lightpaths (``rmsa_gn_gate_parameters(protect_running=True)``, ``gn_protect``; not in the
        reference): a candidate that passes its own check is provisioned only if no running service on a shared link
        falls below the threshold of its modulation with the candidate lit.  ``"gn_neighbour_margin_db"`` in ``outputs`` -- the
        smallest ``GSNR - threshold`` over those services, NaN where that check did not run (no own check, the own check refused,
        no running service shares a link, or a handle that does not protect); it leaves through ``orlg_step_gn_protect``.  A
        refusal by either check is the gate's refusal, cause ``"gn"``; ``sap_ff_gn`` goes on to the next path after either.
        ``gn_rule=``, the ``_gn`` mask kinds and :meth:`path_rule_windows` know the candidate's own check only: on a protecting
        handle they raise ``ValueError``.

        Max-margin assignment inside the step (``orlg_step_max_margin``; not in the reference): the names of
        ``_lib.MAX_MARGIN_POLICIES`` on a handle with ``gn_gate=``, protecting or not -- ``sap_mm`` (the first path in order that has
        an admitted window, at the admitted window whose worst margin ``w = min(GSNR - threshold, neighbour margin)`` is the
        largest, ties to the lowest start), ``any_mm`` (of all k paths the one whose such window has the largest ``w``, ties to the
        lowest path) and ``path_mm_external`` (``actions`` [B] names the path).  Where a path in scope has a free window but none is
        admitted, the lowest free start of the first such path is proposed and refused: a gate refusal, cause ``"gn"``.
        ``"gn_window_margin_db"`` in ``outputs`` (these names only) -- the ``w`` of the proposed window, NaN for such a fallback or
        a rejection.  ``n_steps`` steps are one launch; :meth:`max_margin_windows` is the matching query, bit for bit.  Without a
        gate, or with ``gn_rule=``: ``ValueError``.

        Adaptive modulation behind the gate (``orlg_step_modulation``; not in the reference): the names of
        ``_lib.ADAPTIVE_POLICIES`` on a handle with ``gn_gate=rmsa_gn_gate_parameters(..., modulation="adaptive")``.  A level ``m`` in
        ``1..M`` (``M`` = the gate's thresholds) is the spectral efficiency a service runs at: ``n_m`` slots, admitted iff the GSNR of
        the first fit of ``n_m`` meets ``thresholds_db[m - 1]``.  ``sp_ff_am`` (path 0, levels ``M`` down to 1, the first admitted
        candidate), ``sap_ff_am`` (the paths in order, each with its levels), ``path_am_external`` (``actions`` [B] name the path)
        and ``external_am`` (``actions`` [B, 3] = (path, slot, se); an ``se`` outside ``1..M`` is an action out of range).
        Candidates were checked and none admitted: the gate's refusal, with ``act_path`` / ``act_slot`` / ``gn_gsnr_db`` / ``gn_se``
        of the FIRST candidate checked.  ``"gn_se"`` in ``outputs`` (these names only) -- [n_steps, B] uint8, the level of the
        candidate shown, 0 where no check ran.  Every other policy keeps proposing at the path's own spectral efficiency on such a
        handle; ``gn_rule=``, the ``_mm`` names and ``block_cause`` / ``cause_counts`` raise ``ValueError`` there.
        :meth:`modulation_windows` is the matching query."""
        if policy in _lib.ADAPTIVE_POLICIES:
            return self._run_modulation(policy, n_steps, actions, auto_reset, outputs, out, cause_counts, gn_rule)
        if "gn_se" in _output_names(outputs, out):
            raise ValueError(f"policy {policy!r}: gn_se is an output of the names of _lib.ADAPTIVE_POLICIES only")
        if self.gn_adaptive:
            later = "no such launch runs behind an adaptive gate yet"
            if policy in _lib.MAX_MARGIN_POLICIES:
                self._refuse_adaptive(f"policy {policy!r}", later)
            if gn_rule is not None:
                self._refuse_adaptive(f"gn_rule={gn_rule!r}", later)
            if "block_cause" in _output_names(outputs, out) or (cause_counts is not None and cause_counts is not False):
                self._refuse_adaptive("block_cause / cause_counts", "its step kernel holds no classifier yet")
        if policy in _lib.MAX_MARGIN_POLICIES:
            return self._run_max_margin(policy, n_steps, actions, auto_reset, outputs, out, cause_counts, gn_rule)
        if "gn_window_margin_db" in _output_names(outputs, out):
            raise ValueError(f"policy {policy!r}: gn_window_margin_db is an output of the names of _lib.MAX_MARGIN_POLICIES only")
        if gn_rule is not None:
            return self._run_rule_gn(policy, n_steps, actions, auto_reset, outputs, out, cause_counts, gn_rule)
        return self._run(policy, n_steps, actions, auto_reset, outputs, out, cause_counts)

    def _run_modulation(self, policy, n_steps, actions, auto_reset, outputs, out, cause_counts, gn_rule):
        """``run(<a name of ADAPTIVE_POLICIES>)``: the refusals before the library is called, then ``orlg_step_modulation``."""
        if gn_rule is not None:
            raise ValueError(f"policy {policy!r} with gn_rule=: the policy walks the levels of the reference's first fit, no assignment rule runs with it")
        if not self.gn_adaptive:
            raise ValueError(f"policy {policy!r} needs a handle whose gate chooses the modulation "
                             "(gn_gate=rmsa_gn_gate_parameters(..., modulation='adaptive'))")
        names = _output_names(outputs, out)
        if "block_cause" in names or (cause_counts is not None and cause_counts is not False):
            raise ValueError(f"policy {policy!r}: block_cause / cause_counts are not served with the names of _lib.ADAPTIVE_POLICIES yet")
        for name in ("gn_neighbour_margin_db", "gn_window_margin_db"):
            if name in names:
                raise ValueError(f"policy {policy!r}: {name} is not an output of the names of _lib.ADAPTIVE_POLICIES")
        if int(n_steps) < 1:
            raise ValueError(f"n_steps {n_steps}: expected >= 1")
        B = self.batch_size
        ap = None
        if policy in ("path_am_external", "external_am"):
            if actions is None:
                raise ValueError(f"policy {policy!r} needs an actions array")
            if int(n_steps) != 1:
                raise ValueError(f"policy {policy!r}: the actions name one candidate per environment, n_steps must be 1")
            if not hasattr(actions, "data_ptr"):
                actions = np.asarray(actions)
                if actions.dtype.kind not in "iu":
                    raise TypeError(f"actions: dtype {actions.dtype}, expected an integer type")
                actions = np.ascontiguousarray(actions, dtype=np.int32)
            _check_buffer("actions", actions, (B, 3) if policy == "external_am" else (B,), np.int32)
            ap = _ptr(actions)
        io = _lib.StepIO()
        extra = {}
        for name, dtype in (("gn_gsnr_db", "float64"), ("gn_se", "uint8")):
            if name in names:
                names = [n for n in names if n != name]
                extra.update(self._step_outputs([name], n_steps, out, {name: dtype}, {}))
        res = self._step_outputs(names, n_steps, out, _lib.STEP_IO_DTYPES, _STEP_IO_SHAPES, io)
        _lib.check(self.L.orlg_step_modulation(self.h, _lib.ADAPTIVE_POLICY_IDS[policy], int(n_steps), ap, 1 if auto_reset else 0,
                                               C.byref(io), _ptr(extra.get("gn_gsnr_db")), _ptr(extra.get("gn_se"))))
        res.update(extra)
        return res

    def modulation_windows(self, slot_out=None, gsnr_out=None, admitted_out=None, best_se_out=None):
        """Every level of every candidate path of every env's pending request behind a gate that chooses the modulation
        (``orlg_gn_modulation_windows``; one launch, no early exit): ``(slot, gsnr_db, admitted, best_se)`` -- [B, k, M]
        int16 the first fit of ``n_m`` on the path (``S`` = no window), [B, k, M] float64 its GSNR in dB (NaN), [B, k, M] uint8 1 iff
        it meets ``thresholds_db[m - 1]``, and [B, k] uint8 the level ``path_am_external`` provisions on the path (0 = none).  Entry
        ``[p, m - 1]`` is the outcome of ``run("external_am", actions=[p, slot, m])``, with the bits of its ``gn_gsnr_db``: the
        agent's mask and feature for ``external_am`` / ``path_am_external``.  Reads state only; the buffers as ``out`` in
        :meth:`action_masks`."""
        if not self.gn_adaptive:
            raise ValueError("modulation_windows needs a handle whose gate chooses the modulation "
                             "(gn_gate=rmsa_gn_gate_parameters(..., modulation='adaptive'))")
        B, k, M = self.batch_size, self.k_paths, self.modulation_levels
        res = [self._checked_out(name, buf, shape, dt) for name, buf, shape, dt in (
            ("slot_out", slot_out, (B, k, M), np.int16), ("gsnr_out", gsnr_out, (B, k, M), np.float64),
            ("admitted_out", admitted_out, (B, k, M), np.uint8), ("best_se_out", best_se_out, (B, k), np.uint8))]
        _lib.check(self.L.orlg_gn_modulation_windows(self.h, *(_ptr(b) for b in res)))
        return tuple(res)

    def _run_max_margin(self, policy, n_steps, actions, auto_reset, outputs, out, cause_counts, gn_rule):
        """``run(<a name of MAX_MARGIN_POLICIES>)``: the refusals before the library is called, then ``orlg_step_max_margin_protect``."""
        if gn_rule is not None:
            raise ValueError(f"policy {policy!r} with gn_rule=: a max-margin policy names its own window, no assignment rule runs with it")
        if self.gn_gate is None:
            raise ValueError(f"policy {policy!r} needs a handle with a GN-model admission check (gn_gate=): the margin is the check's")
        if int(n_steps) < 1:
            raise ValueError(f"n_steps {n_steps}: expected >= 1")
        B = self.batch_size
        route = _lib.MAX_MARGIN_ROUTES[policy]
        ap = None
        if policy == "path_mm_external":
            if actions is None:
                raise ValueError(f"policy {policy!r} needs an actions array")
            if int(n_steps) != 1:
                raise ValueError(f"policy {policy!r}: the actions name one path per environment, n_steps must be 1")
            if not hasattr(actions, "data_ptr"):
                actions = np.asarray(actions)
                if actions.dtype.kind not in "iu":
                    raise TypeError(f"actions: dtype {actions.dtype}, expected an integer type")
                actions = np.ascontiguousarray(actions, dtype=np.int32)
            _check_buffer("actions", actions, (B,), np.int32)
            ap = _ptr(actions)
        io = _lib.StepIO()
        names = _output_names(outputs, out)
        extra = {}
        for name, dtype in (("gn_gsnr_db", "float64"), ("gn_neighbour_margin_db", "float64"), ("gn_window_margin_db", "float64"),
                            ("block_cause", "uint8")):
            if name in names:
                names = [n for n in names if n != name]
                extra.update(self._step_outputs([name], n_steps, out, {name: dtype}, {}))
        if cause_counts is not None and cause_counts is not False:
            if cause_counts is True:
                cause_counts = np.zeros((B, _lib.NUM_CAUSES), np.int32)
            else:
                _check_buffer("out[cause_counts]", cause_counts, (B, _lib.NUM_CAUSES), np.int32)
            extra["block_cause_counts"] = cause_counts
        res = self._step_outputs(names, n_steps, out, _lib.STEP_IO_DTYPES, _STEP_IO_SHAPES, io)
        d = _lib.StepDiag(_ptr(extra.get("block_cause")), _ptr(extra.get("block_cause_counts")), _ptr(extra.get("gn_gsnr_db")))
        _lib.check(self.L.orlg_step_max_margin_protect(self.h, route, int(n_steps), ap, 1 if auto_reset else 0, C.byref(io), C.byref(d),
                                                       _ptr(extra.get("gn_window_margin_db")), _ptr(extra.get("gn_neighbour_margin_db"))))
        res.update(extra)
        return res

    def _run_rule_gn(self, policy, n_steps, actions, auto_reset, outputs, out, cause_counts, gn_rule):
        """``run(..., gn_rule=)``: every refusal before the library is called."""
        if gn_rule not in _lib.GN_RULE_MODES:
            raise ValueError(f"gn_rule {gn_rule!r}: expected None or one of {tuple(_lib.GN_RULE_MODES)}")
        if policy in _lib.WINDOW_POLICIES:
            raise ValueError(f"policy {policy!r} with gn_rule=: the most-used rule and the any_* routes are not served behind a "
                             "GN-model admission check")
        if policy not in _lib.ASSIGN_POLICIES and policy not in _lib.CUT_POLICIES:
            raise ValueError(f"policy {policy!r} with gn_rule=: expected a name of _lib.ASSIGN_POLICIES or _lib.CUT_POLICIES (a route "
                             "with an assignment rule other than the reference's first fit)")
        if self.gn_gate is None:
            raise ValueError(f"gn_rule={gn_rule!r} needs a handle with a GN-model admission check (gn_gate=)")
        if self.gn_protect:
            raise ValueError(f"gn_rule={gn_rule!r}: the handle protects its running lightpaths (protect_running), and no assignment "
                             "rule runs behind that second check yet")
        if gn_rule == "next_path" and not policy.startswith("sap_"):
            raise ValueError(f"gn_rule='next_path' goes on to the next candidate path: it needs a sap_* name, got {policy!r}")
        return self._run(policy, n_steps, actions, auto_reset, outputs, out, cause_counts, _lib.GN_RULE_MODES[gn_rule])

    def _run(self, policy, n_steps, actions, auto_reset, outputs, out, cause_counts, gn_mode=None):
        cut = policy in _lib.CUT_POLICIES
        window = policy in _lib.WINDOW_POLICIES
        pid, rule = (_lib.CUT_POLICIES[policy], 0) if cut else _lib.WINDOW_POLICIES[policy] if window else _lib.policy_ids(policy)
        if (rule or cut) and self.gn_gate is not None and gn_mode is None:
            raise ValueError(f"policy {policy!r}: an assignment rule other than the reference's first fit does not run on a handle "
                             "with a GN-model admission check (gn_gate=)")
        B = self.batch_size
        io = _lib.StepIO()
        names = _output_names(outputs, out)
        gsnr = None
        if "gn_gsnr_db" in names:
            names = [n for n in names if n != "gn_gsnr_db"]
            gsnr = self._step_outputs(["gn_gsnr_db"], n_steps, out, {"gn_gsnr_db": "float64"}, {})
        margin = None
        if "gn_neighbour_margin_db" in names:
            names = [n for n in names if n != "gn_neighbour_margin_db"]
            margin = self._step_outputs(["gn_neighbour_margin_db"], n_steps, out, {"gn_neighbour_margin_db": "float64"}, {})
        diag = {}
        if "block_cause" in names:
            names = [n for n in names if n != "block_cause"]
            diag.update(self._step_outputs(["block_cause"], n_steps, out, {"block_cause": "uint8"}, {}))
        if cause_counts is not None and cause_counts is not False:
            if cause_counts is True:
                cause_counts = np.zeros((B, _lib.NUM_CAUSES), np.int32)
            else:
                _check_buffer("out[cause_counts]", cause_counts, (B, _lib.NUM_CAUSES), np.int32)
            diag["block_cause_counts"] = cause_counts
        res = self._step_outputs(names, n_steps, out, _lib.STEP_IO_DTYPES, _STEP_IO_SHAPES, io)
        ap = None
        if pid in (_lib.POLICIES["external"], _lib.POLICIES["deeprmsa_external"], _lib.POLICIES["path_ff_external"]):
            if actions is None:
                raise ValueError(f"policy {policy!r} needs an actions array")
            ashape = (B, 2) if pid == _lib.POLICIES["external"] else (B,)
            if not hasattr(actions, "data_ptr"):
                actions = np.asarray(actions)
                if actions.dtype.kind not in "iu":
                    raise TypeError(f"actions: dtype {actions.dtype}, expected an integer type")
                actions = np.ascontiguousarray(actions, dtype=np.int32)
            _check_buffer("actions", actions, ashape, np.int32)
            ap = _ptr(actions)
        if margin is not None:
            if rule or cut or gn_mode is not None:
                raise ValueError(f"policy {policy!r}: gn_neighbour_margin_db leaves a launch of the reference's first fit only "
                                 "(orlg_step_gn_protect); no assignment rule runs behind the check of the running lightpaths")
            d = _lib.StepDiag(_ptr(diag.get("block_cause")), _ptr(diag.get("block_cause_counts")),
                              None if gsnr is None else _ptr(gsnr["gn_gsnr_db"]))
            _lib.check(self.L.orlg_step_gn_protect(self.h, pid, int(n_steps), ap, 1 if auto_reset else 0, C.byref(io), C.byref(d),
                                                   _ptr(margin["gn_neighbour_margin_db"])))
            res.update(diag)
            res.update(gsnr or {})
            res.update(margin)
        elif diag or rule or cut:   # (a name of WINDOW_POLICIES has a rule)
            d = _lib.StepDiag(_ptr(diag.get("block_cause")), _ptr(diag.get("block_cause_counts")),
                              None if gsnr is None else _ptr(gsnr["gn_gsnr_db"]))
            if gn_mode is not None:
                _lib.check(self.L.orlg_step_rule_gn(self.h, pid, _lib.RULE_FEWEST_CUTS if cut else rule, gn_mode, int(n_steps), ap,
                                                    1 if auto_reset else 0, C.byref(io), C.byref(d)))
            elif cut:
                _lib.check(self.L.orlg_step_min_cut(self.h, pid, int(n_steps), ap, 1 if auto_reset else 0, C.byref(io), C.byref(d)))
            elif window:
                _lib.check(self.L.orlg_step_window(self.h, pid, rule, int(n_steps), ap, 1 if auto_reset else 0, C.byref(io), C.byref(d)))
            elif rule:
                _lib.check(self.L.orlg_step_assign(self.h, pid, rule, int(n_steps), ap, 1 if auto_reset else 0, C.byref(io),
                                                   C.byref(d)))
            else:
                _lib.check(self.L.orlg_step_diag(self.h, pid, int(n_steps), ap, 1 if auto_reset else 0, C.byref(io), C.byref(d)))
            res.update(diag)
            res.update(gsnr or {})
        elif gsnr is None:
            _lib.check(self.L.orlg_step(self.h, pid, int(n_steps), ap, 1 if auto_reset else 0, C.byref(io)))
        else:
            _lib.check(self.L.orlg_step_gn(self.h, pid, int(n_steps), ap, 1 if auto_reset else 0,
                                           C.byref(io), _ptr(gsnr["gn_gsnr_db"])))
            res.update(gsnr)
        return res

    def step(self, actions, outputs=("reward", "done", "accepted")):
        """RMSAEnv.step for every env: ``actions`` is [B, 2] int32 (path, initial_slot)."""
        r = self.run("external", 1, actions=actions, outputs=outputs)
        return {k: v[0] for k, v in r.items()}

    def step_deeprmsa(self, actions, outputs=("reward", "done", "accepted")):
        """DeepRMSAEnv.step for every env: ``actions`` is [B] int32 in Discrete(k*j + reject)."""
        r = self.run("deeprmsa_external", 1, actions=actions, outputs=outputs)
        return {k: v[0] for k, v in r.items()}

    # ------------------------------------------------------------------ state read-back
    def occupancy_words(self):
        return self._occupancy_words()

    def available_slots(self):
        """topology.graph["available_slots"] for every env: [B, E, S] uint8 (1 = free)."""
        w = self.occupancy_words()
        bits = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")
        return bits.reshape(self.batch_size, self.topology.num_links, -1)[:, :, :self.num_spectrum_resources]

    def link_stats(self):
        B, E = self.batch_size, self.topology.num_links
        out = [np.zeros((B, E)) for _ in range(4)]
        _lib.check(self.L.orlg_get_link_stats(self.h, *[_ptr(a) for a in out]))
        return dict(zip(("utilization", "external_fragmentation", "compactness", "last_update"), out))

    def graph_stats(self):
        out = [np.zeros(self.batch_size) for _ in range(3)]
        _lib.check(self.L.orlg_get_graph_stats(self.h, *[_ptr(a) for a in out]))
        return dict(zip(("throughput", "compactness", "last_update"), out))

    def bit_rate_hist(self):
        B, n = self.batch_size, len(self.bit_rates)
        out = [np.zeros((B, n), np.int64) for _ in range(4)]
        _lib.check(self.L.orlg_get_bit_rate_hist(self.h, *[_ptr(a) for a in out]))
        return dict(zip(("requested", "provisioned", "episode_requested", "episode_provisioned"), out))

    def episodes_done(self):
        return self._read(self.L.orlg_get_episodes_done, self.batch_size, np.int64)

    def path_masks(self, env_index: int = 0):
        """(masks [k, W] uint64, nslots [k]) for the pending request of one env."""
        m = np.zeros((self.k_paths, self.words_per_link), np.uint64)
        n = np.zeros(self.k_paths, np.int32)
        _lib.check(self.L.orlg_query_path_masks(self.h, int(env_index), _ptr(m), _ptr(n)))
        return m, n

    def path_mask(self, path_gid: int, env_index: int = 0):
        """Free bitmap [W] of one arbitrary path record and its slot demand for the pending bit rate."""
        m = np.zeros(self.words_per_link, np.uint64)
        n = np.zeros(1, np.int32)
        _lib.check(self.L.orlg_query_path_mask(self.h, int(env_index), int(path_gid), _ptr(m), _ptr(n)))
        return m, int(n[0])

    def observation(self, out=None, dtype=np.float64, mask_out=None, return_mask=False):
        """DeepRMSAEnv.observation() for every env: [B, obs_dim] float64 (the reference's Box dtype), or float32 -- the
        float64 vector rounded once, ``obs.astype(np.float32)`` -- with ``dtype=np.float32`` / a float32 ``out`` buffer.

        ``mask_out=`` (a [B, k*j + reject] uint8 buffer) or ``return_mask=True``: the DeepRMSA action mask leaves the same
        launch, and the call returns ``(observation, mask)``; see :meth:`action_masks`."""
        B = self.batch_size
        if out is None:
            out = np.zeros((B, self.obs_dim), dtype)
        elif _dtype_name(out) == "float32":
            dtype = np.float32
        f32 = np.dtype(dtype) == np.float32
        _check_buffer("out", out, (B, self.obs_dim), np.float32 if f32 else np.float64)
        if mask_out is None and not return_mask:
            call = self.L.orlg_deeprmsa_observation_f32 if f32 else self.L.orlg_deeprmsa_observation
            _lib.check(call(self.h, _ptr(out)))
            return out
        if mask_out is None:
            mask_out = np.zeros((B, self.mask_dim), np.uint8)
        else:
            _check_buffer("mask_out", mask_out, (B, self.mask_dim), np.uint8)
        _lib.check(self.L.orlg_deeprmsa_observation_masked(self.h, _ptr(out), 1 if f32 else 0, _ptr(mask_out)))
        return out, mask_out

    MASK_KINDS = ("deeprmsa", "path_ff", "slots", "path_ff_gn", "deeprmsa_gn")
    GN_MASK_KINDS = ("path_ff_gn", "deeprmsa_gn")   # the kinds that know the GN-model admission check (``gn_gate=``)

    def action_mask_shape(self, kind):
        """(shape, dtype) of ``action_masks(kind)``."""
        if kind not in self.MASK_KINDS:
            raise ValueError(f"kind {kind!r}: expected one of {self.MASK_KINDS}")
        B, k = self.batch_size, self.k_paths
        if kind in ("deeprmsa", "deeprmsa_gn"):
            return (B, k * self.j + self.reject_action), np.uint8
        if kind in ("path_ff", "path_ff_gn"):
            return (B, k + self.reject_action), np.uint8
        return (B, k, self.words_per_link), np.uint64

    def action_mask_gsnr_shape(self, kind):
        """(shape, dtype) of the GSNR rows that go with ``action_masks(kind, gsnr_out=...)``: one column per action, none for
        the explicit rejection."""
        if kind not in self.GN_MASK_KINDS:
            raise ValueError(f"kind {kind!r} has no GSNR rows: expected one of {self.GN_MASK_KINDS}")
        return (self.batch_size, self.k_paths * (self.j if kind == "deeprmsa_gn" else 1)), np.float64

    def action_masks(self, kind="deeprmsa", out=None, gsnr_out=None):
        """Valid actions of every env's pending request: ``mask[a] = 1`` iff ``step(a)`` would accept the service.  The explicit
        rejection, where ``allow_rejection`` gives the action space one, is always 1.

        The first three kinds say "the window is free" -- the reference's ``step(a)`` -- on every handle: they do not know a
        GN-model admission check (``gn_gate=``), which may still refuse the service.
        ``"deeprmsa"``  [B, k*j + reject] uint8: action ``a`` = (route ``a // j``, block ``a % j``) is valid iff the route has
                        more than ``block`` free runs of at least ``get_number_slots(route)`` slots (``deeprmsa_env.py:48-58``).
        ``"path_ff"``   [B, k + reject] uint8: ``PathOnlyFirstFitAction.action(p)`` finds a slot -- some ``s`` in
                        ``range(0, S - n)`` is free (``rmsa_env.py:974-1008``; the bound is exclusive, as in the reference).
        ``"slots"``     [B, k, W] uint64, bit ``s`` of word ``w`` = slot ``64 w + s``: ``RMSAEnv.step([p, s])`` provisions --
                        ``s + n <= S`` and the window is free on every hop (start ``S - n`` included).
        The ``_gn`` kinds exist on a handle with ``gn_gate=`` only and say what ITS step does (``orlg_gn_action_masks``):
        ``"path_ff_gn"``   ``path_ff[p]`` and the GSNR of the path's first-fit window meets the threshold of its spectral
                           efficiency: the outcome of ``step_path_first_fit(p)``.
        ``"deeprmsa_gn"``  ``deeprmsa[a]`` and the GSNR of the first ``n`` slots of the block meets the threshold: the outcome of
                           ``step_deeprmsa(a)``.
        ``gsnr_out`` (these two kinds only): a float64 buffer [B, k] / [B, k*j], or ``True`` for a new array -- the GSNR in dB the
        step would compare, NaN where there is no window; the call then returns ``(mask, gsnr)``.
        ``out`` / ``gsnr_out`` may be numpy arrays or torch tensors (device tensors and pinned host tensors are written in
        place)."""
        shape, dt = self.action_mask_shape(kind)
        gn = kind in self.GN_MASK_KINDS
        if gsnr_out is not None and gsnr_out is not False and not gn:
            raise ValueError(f"gsnr_out: kind {kind!r} has no GSNR rows, they go with {self.GN_MASK_KINDS}")
        if gn and self.gn_gate is None:
            raise ValueError(f"kind {kind!r} needs a handle with a GN-model admission check (gn_gate=)")
        if gn:
            self._refuse_adaptive(f"kind {kind!r}", "this mask describes a step at the path's own spectral efficiency against services "
                                  "without levels: modulation_windows() is the query of such a handle")
        if gn and self.gn_protect:
            raise ValueError(f"kind {kind!r}: the handle protects its running lightpaths (protect_running); this mask knows the "
                             "candidate's own check only and would describe a step the handle does not run: "
                             f"admission_masks({kind[:-3]!r}) knows both checks")
        if out is None:
            out = np.zeros(shape, dt)
        else:
            _check_buffer("out", out, shape, dt)
        if gn:
            gsnr = None
            if gsnr_out is True:
                gsnr = np.zeros(self.action_mask_gsnr_shape(kind)[0], np.float64)
            elif gsnr_out is not None and gsnr_out is not False:
                _check_buffer("gsnr_out", gsnr_out, *self.action_mask_gsnr_shape(kind))
                if not hasattr(gsnr_out, "data_ptr") and not gsnr_out.flags["WRITEABLE"]:
                    raise ValueError("gsnr_out: read-only array")
                gsnr = gsnr_out
            gp = None if gsnr is None else _ptr(gsnr)
            if kind == "path_ff_gn":
                _lib.check(self.L.orlg_gn_action_masks(self.h, _ptr(out), gp, None, None))
            else:
                _lib.check(self.L.orlg_gn_action_masks(self.h, None, None, _ptr(out), gp))
            return out if gsnr is None else (out, gsnr)
        if kind == "deeprmsa":
            _lib.check(self.L.orlg_deeprmsa_observation_masked(self.h, None, 0, _ptr(out)))
        elif kind == "path_ff":
            _lib.check(self.L.orlg_action_masks(self.h, _ptr(out), None))
        else:
            _lib.check(self.L.orlg_action_masks(self.h, None, _ptr(out)))
        return out

    def path_fit_levels(self, out=None):
        """How far every candidate path of every env's pending request is from fitting it: [B, k] uint8, an index into
        ``FIT_LEVELS`` (include/orlg.h ``ORLG_FIT_*``) -- 4 a first fit exists (the ``"path_ff"`` mask bit), 3 only the window at
        ``S - n`` that the first-fit loops never try, 2 every link has a run of ``n`` free slots but they do not line up,
        1 every link has ``n`` free slots but some link no run of them, 0 some link has fewer than ``n`` free slots.  Windows
        only, on every handle: it does not know a GN-model admission check.  ``out`` as in :meth:`action_masks`."""
        shape = (self.batch_size, self.k_paths)
        if out is None:
            out = np.zeros(shape, np.uint8)
        else:
            _check_buffer("out", out, shape, np.uint8)
        _lib.check(self.L.orlg_path_fit_levels(self.h, _ptr(out)))
        return out

    def path_min_cuts(self, cuts_out=None, slots_out=None):
        """The fewest-cuts window of every candidate path of every env's pending request (``orlg_path_min_cuts``):
        ``(cuts, slots)``, both [B, k] int16 -- the number of the path's links on which the window leaves free slots on both of
        its sides (it splits a free block in two there), and the window's start; ``-1`` and ``S`` where the path has no window.
        What the ``_lib.CUT_POLICIES`` propose, as a feature and a mask for the path-only action space.  Reads state only;
        ``cuts_out`` / ``slots_out`` as ``out`` in :meth:`action_masks`."""
        shape = (self.batch_size, self.k_paths)
        res = []
        for name, buf in (("cuts_out", cuts_out), ("slots_out", slots_out)):
            if buf is None:
                buf = np.zeros(shape, np.int16)
            else:
                _check_buffer(name, buf, shape, np.int16)
            res.append(buf)
        _lib.check(self.L.orlg_path_min_cuts(self.h, _ptr(res[0]), _ptr(res[1])))
        return res[0], res[1]

    def slot_usage(self, out=None):
        """The slot usage of every env (``orlg_slot_usage``): [B, S] uint8, the number of links of the whole topology
        on which the slot is occupied -- what the most-used rule sums over a window, as a feature.  Reads state only; ``out`` as
        in :meth:`action_masks`."""
        shape = (self.batch_size, self.num_spectrum_resources)
        if out is None:
            out = np.zeros(shape, np.uint8)
        else:
            _check_buffer("out", out, shape, np.uint8)
        _lib.check(self.L.orlg_slot_usage(self.h, _ptr(out)))
        return out

    def path_most_used(self, usage_out=None, slots_out=None):
        """The most-used window of every candidate path of every env's pending request (``orlg_path_most_used``):
        ``(usage, slots)`` -- [B, k] int32, the window's usage (the sum of :meth:`slot_usage` over its slots), and [B, k] int16,
        its start; ``-1`` and ``S`` where the path has no window.  What the ``*_mu`` names of ``_lib.WINDOW_POLICIES`` propose.
        Reads state only; ``usage_out`` / ``slots_out`` as ``out`` in :meth:`action_masks`."""
        shape = (self.batch_size, self.k_paths)
        res = []
        for name, buf, dt in (("usage_out", usage_out, np.int32), ("slots_out", slots_out, np.int16)):
            if buf is None:
                buf = np.zeros(shape, dt)
            else:
                _check_buffer(name, buf, shape, dt)
            res.append(buf)
        _lib.check(self.L.orlg_path_most_used(self.h, _ptr(res[0]), _ptr(res[1])))
        return res[0], res[1]

    def path_rule_windows(self, rule, slots_out=None, gsnr_out=None, admitted_out=None):
        """The window an assignment rule proposes on every candidate path of every env's pending request, and what the GN-model
        admission check says to it (``orlg_gn_path_windows``; a handle with ``gn_gate=`` only): ``(slots, gsnr,
        admitted)`` -- [B, k] int16 the window's start (``S`` = the path has none), [B, k] float64 the GSNR in dB the step would
        compare (NaN = no window), [B, k] uint8 1 iff the window exists and is admitted.  ``rule``: ``"first"`` (the reference's
        first fit: the ``"path_ff_gn"`` mask), ``"first_full"``, ``"last"``, ``"best"``, ``"exact"`` or ``"min_cut"``.  Row ``p`` is
        the outcome of ``run("path_<rule>_external", actions=p, gn_rule="check")``, with the bits of its ``gn_gsnr_db``: the
        agent's feature and mask for the path-only action space.  Reads state only; the buffers as ``out`` in
        :meth:`action_masks`."""
        if rule not in _lib.GN_PATH_WINDOW_RULES:
            raise ValueError(f"rule {rule!r}: expected one of {tuple(_lib.GN_PATH_WINDOW_RULES)}")
        if self.gn_gate is None:
            raise ValueError("path_rule_windows needs a handle with a GN-model admission check (gn_gate=)")
        self._refuse_adaptive("path_rule_windows", "no assignment rule runs behind an adaptive gate yet: modulation_windows() is the query of such a handle")
        if self.gn_protect:
            raise ValueError("path_rule_windows: the handle protects its running lightpaths (protect_running); this query knows the "
                             "candidate's own check only and would describe a step the handle does not run: "
                             "admission_windows(rule) knows both checks")
        shape = (self.batch_size, self.k_paths)
        res = []
        for name, buf, dt in (("slots_out", slots_out, np.int16), ("gsnr_out", gsnr_out, np.float64), ("admitted_out", admitted_out, np.uint8)):
            if buf is None:
                buf = np.zeros(shape, dt)
            else:
                _check_buffer(name, buf, shape, dt)
            res.append(buf)
        _lib.check(self.L.orlg_gn_path_windows(self.h, _lib.GN_PATH_WINDOW_RULES[rule], _ptr(res[0]), _ptr(res[1]), _ptr(res[2])))
        return res[0], res[1], res[2]

    # ------------------------------------------------------------------ masks and rule windows that know both halves of the check
    ADMISSION_MASK_KINDS = ("path_ff", "deeprmsa")

    def _float_rows(self, name, buf, shape):
        """a float64 row buffer of a query: None / False = not asked for, True = a new array, else the caller's, checked"""
        if buf is None or buf is False:
            return None
        if buf is True:
            return np.zeros(shape, np.float64)
        _check_buffer(name, buf, shape, np.float64)
        if not hasattr(buf, "data_ptr") and not buf.flags["WRITEABLE"]:
            raise ValueError(f"{name}: read-only array")
        return buf

    def admission_masks(self, kind, out=None, gsnr_out=None, margin_out=None):
        """Valid actions of every env's pending request under BOTH halves of the GN-model admission check
        (``orlg_gn_admission_masks``; a handle with ``gn_gate=`` only): ``mask[a] = 1`` iff the step THIS handle runs
        would accept the service -- the window exists, its own GSNR meets the threshold of the path's modulation and, on a handle
        that protects its running lightpaths (``protect_running``), no running service that shares a link falls below its own
        threshold (the neighbour margin is not below zero).  ``kind``: ``"path_ff"`` [B, k + reject] uint8, the outcome of
        ``run("path_ff_external", actions=p)``, or ``"deeprmsa"`` [B, k*j + reject], the outcome of ``run("deeprmsa_external",
        actions=a)``; the explicit rejection's column is always 1.  ``gsnr_out`` / ``margin_out``: a float64 buffer [B, k] / [B, k*j]
        or ``True`` for a new array -- the bits of that step's ``gn_gsnr_db`` (NaN = no window) and ``gn_neighbour_margin_db`` (NaN =
        the second check would not run: no window, the own check refuses, no running service shares a link, or the handle does not
        protect).  Returns ``mask``, or a tuple ``(mask[, gsnr][, margin])`` with the rows that were asked for.  On a gated handle
        that does not protect the mask and the GSNR are those of ``action_masks(kind + "_gn")``.  Reads state only; the buffers as
        ``out`` in :meth:`action_masks`."""
        if kind not in self.ADMISSION_MASK_KINDS:
            raise ValueError(f"kind {kind!r}: expected one of {self.ADMISSION_MASK_KINDS}")
        if self.gn_gate is None:
            raise ValueError("admission_masks needs a handle with a GN-model admission check (gn_gate=)")
        self._refuse_adaptive("admission_masks", "modulation_windows() is the query of such a handle")
        shape, dt = self.action_mask_shape(kind)
        rows = (self.batch_size, self.k_paths * (self.j if kind == "deeprmsa" else 1))
        if out is None:
            out = np.zeros(shape, dt)
        else:
            _check_buffer("out", out, shape, dt)
            if not hasattr(out, "data_ptr") and not out.flags["WRITEABLE"]:
                raise ValueError("out: read-only array")
        gsnr = self._float_rows("gsnr_out", gsnr_out, rows)
        margin = self._float_rows("margin_out", margin_out, rows)
        ptrs = (_ptr(out), None if gsnr is None else _ptr(gsnr), None if margin is None else _ptr(margin))
        if kind == "path_ff":
            _lib.check(self.L.orlg_gn_admission_masks(self.h, *ptrs, None, None, None))
        else:
            _lib.check(self.L.orlg_gn_admission_masks(self.h, None, None, None, *ptrs))
        res = (out,) + tuple(r for r in (gsnr, margin) if r is not None)
        return out if len(res) == 1 else res

    def admission_windows(self, rule, slots_out=None, gsnr_out=None, margin_out=None, admitted_out=None):
        """The window an assignment rule proposes on every candidate path of every env's pending request, and what BOTH halves of
        the GN-model admission check say to it (``orlg_gn_admission_windows``; a handle with ``gn_gate=`` only):
        ``(slots, gsnr, margin, admitted)`` -- slots, gsnr and admitted as :meth:`path_rule_windows`, margin [B, k] float64 the
        candidate's neighbour margin in dB (NaN as in :meth:`admission_masks`).  ``rule``: one of ``_lib.GN_PATH_WINDOW_RULES``.
        Row ``p`` is the outcome of ``run("external", actions=[p, slots[p]])`` on this handle, with the bits of its ``gn_gsnr_db``
        and ``gn_neighbour_margin_db``.  On a gated handle that does not protect slots, gsnr and admitted are those of
        :meth:`path_rule_windows` and every margin is NaN.  Reads state only; the buffers as ``out`` in :meth:`action_masks`."""
        if rule not in _lib.GN_PATH_WINDOW_RULES:
            raise ValueError(f"rule {rule!r}: expected one of {tuple(_lib.GN_PATH_WINDOW_RULES)}")
        if self.gn_gate is None:
            raise ValueError("admission_windows needs a handle with a GN-model admission check (gn_gate=)")
        self._refuse_adaptive("admission_windows", "modulation_windows() is the query of such a handle")
        shape = (self.batch_size, self.k_paths)
        res = []
        for name, buf, dt in (("slots_out", slots_out, np.int16), ("gsnr_out", gsnr_out, np.float64), ("margin_out", margin_out, np.float64),
                              ("admitted_out", admitted_out, np.uint8)):
            if buf is None:
                buf = np.zeros(shape, dt)
            else:
                _check_buffer(name, buf, shape, dt)
                if not hasattr(buf, "data_ptr") and not buf.flags["WRITEABLE"]:
                    raise ValueError(f"{name}: read-only array")
            res.append(buf)
        _lib.check(self.L.orlg_gn_admission_windows(self.h, _lib.GN_PATH_WINDOW_RULES[rule], *(_ptr(b) for b in res)))
        return tuple(res)

    # ------------------------------------------------------------------ the check over every start slot of every path
    def _checked_out(self, name, buf, shape, dt):
        """an output buffer of a query: None = a new array, else the caller's, checked"""
        if buf is None:
            return np.zeros(shape, dt)
        _check_buffer(name, buf, shape, dt)
        if not hasattr(buf, "data_ptr") and not buf.flags["WRITEABLE"]:
            raise ValueError(f"{name}: read-only array")
        return buf

    def admission_slot_masks(self, out=None, gsnr_out=None, margin_out=None):
        """The GN-model admission check over the whole spectrum (``orlg_gn_admission_slots``; a handle with
        ``gn_gate=`` only): ``mask`` [B, k, W] uint64, laid out as ``action_masks("slots")`` -- bit ``s`` of path ``p`` is 1 iff
        ``run("external", actions=[p, s])`` on THIS handle would accept the pending request: the window ``[s, s + n)`` is free on
        every hop, its own GSNR meets the threshold of the path's modulation and, on a handle that protects its running lightpaths
        (``protect_running``), the neighbour margin is not below zero.  ``gsnr_out`` / ``margin_out``: a float64 buffer [B, k, S] or
        ``True`` for a new array -- the GSNR in dB the step would compare for that window (NaN = no free window) and the
        candidate's neighbour margin in dB (NaN = the second check would not run: no window, the own check refuses, no running
        service shares a link, or the handle does not protect).  Returns ``mask``, or a tuple ``(mask[, gsnr][, margin])`` with the
        rows that were asked for.  The GSNR agrees with the step's ``gn_gsnr_db`` to ~1e-15 relative (start slots on lanes sum the
        interferers in ring order), the bit is the step's decision, the margin has the bits of ``gn_neighbour_margin_db``.  Reads
        state only; the buffers as ``out`` in :meth:`action_masks`."""
        if self.gn_gate is None:
            raise ValueError("admission_slot_masks needs a handle with a GN-model admission check (gn_gate=)")
        self._refuse_adaptive("admission_slot_masks", "modulation_windows() is the query of such a handle")
        B, k, S = self.batch_size, self.k_paths, self.num_spectrum_resources
        out = self._checked_out("out", out, (B, k, self.words_per_link), np.uint64)
        gsnr = self._float_rows("gsnr_out", gsnr_out, (B, k, S))
        margin = self._float_rows("margin_out", margin_out, (B, k, S))
        _lib.check(self.L.orlg_gn_admission_slots(self.h, _ptr(out), None if gsnr is None else _ptr(gsnr),
                                                  None if margin is None else _ptr(margin), None, None))
        res = (out,) + tuple(r for r in (gsnr, margin) if r is not None)
        return out if len(res) == 1 else res

    def max_margin_windows(self, slots_out=None, margin_out=None):
        """Of all windows of every candidate path that the admission check of THIS handle admits, the one that leaves the most
        margin (``orlg_gn_admission_slots``; a handle with ``gn_gate=`` only): ``(slots, margin)`` -- [B, k] int16, the
        lowest start among the admitted windows with the largest worst margin (``S`` = the path has no admitted window), and
        [B, k] float64, that margin in dB (NaN = none): ``gsnr - threshold`` of the window itself or, where it is smaller, the
        neighbour margin of a protecting handle.  ``run("external", actions=[p, slots[p]])`` accepts wherever ``slots[p] < S``.
        Reads state only; the buffers as ``out`` in :meth:`action_masks`."""
        if self.gn_gate is None:
            raise ValueError("max_margin_windows needs a handle with a GN-model admission check (gn_gate=)")
        self._refuse_adaptive("max_margin_windows", "modulation_windows() is the query of such a handle")
        shape = (self.batch_size, self.k_paths)
        slots = self._checked_out("slots_out", slots_out, shape, np.int16)
        margin = self._checked_out("margin_out", margin_out, shape, np.float64)
        _lib.check(self.L.orlg_gn_admission_slots(self.h, None, None, None, _ptr(slots), _ptr(margin)))
        return slots, margin

    # ------------------------------------------------------------------ the running services and their GN-model audit
    RUNNING_SERVICE_FIELDS = (("count", np.int32, False), ("head", np.int32, False), ("path_gid", np.int32, True),
                              ("slot", np.int16, True), ("num_slots", np.int16, True), ("bit_rate", np.int32, True),
                              ("release_time", np.float64, True), ("se", np.int16, True))   # (name, dtype, [B, Q] rather than [B])
    AUDIT_SERVICE_FIELDS = ("gsnr_db", "margin_db", "osnr_ase_db", "snr_nli_db")

    @property
    def queue_capacity(self):
        """Slots of an environment's release ring (``orlg_queue_capacity``): the row length of the per-service arrays below."""
        return int(self.L.orlg_queue_capacity(self.h))

    def _rank_buffers(self, fields, out, what):
        """one buffer per (name, dtype, per service) of `fields`: the caller's (``out[name]``, checked) or a new numpy array"""
        unknown = set(out or ()) - {f[0] for f in fields}
        if unknown:
            raise ValueError(f"{what}: out= has no buffer named {sorted(unknown)}")
        B, Q = self.batch_size, self.queue_capacity
        res = {}
        for name, dt, wide in fields:
            shape = (B, Q) if wide else (B,)
            buf = (out or {}).get(name)
            res[name] = np.zeros(shape, dt) if buf is None else _check_buffer(f"out[{name!r}]", buf, shape, dt)
        return res

    def running_services(self, out=None):
        """The running services of every environment (``orlg_get_running_services``): a dict -- ``count`` [B] int32,
        the live entries of the release ring; ``head`` [B] int32, the ring slot of rank 0; and [B, Q] each, in rank order (ascending
        release time), ``path_gid`` int32 (the global index of the path record), ``slot`` and ``num_slots`` int16, ``bit_rate`` int32
        and ``release_time`` float64, with -1 / NaN past ``count``; ``se`` int16, the spectral efficiency the service runs at -- its
        path's own, or the level an adaptive gate provisioned it at.  ``Q`` is :attr:`queue_capacity`.  Reads state only; ``out``: a
        dict of preallocated buffers by these names (numpy arrays or torch tensors, as ``out`` in :meth:`action_masks`)."""
        res = self._rank_buffers(self.RUNNING_SERVICE_FIELDS, out, "running_services")
        _lib.check(self.L.orlg_get_running_services_se(self.h, *(_ptr(res[f[0]]) for f in self.RUNNING_SERVICE_FIELDS)))
        return res

    def _gn_gate_struct(self, g):
        """(orlg_rmsa_gn_gate, the arrays it points to) of a checked gate dict; the library copies what it needs"""
        gg = _lib.RmsaGnGate()
        for name in _osnr.RMSA_GN_GATE_SCALARS:
            setattr(gg, name, float(g[name]))
        keep = [np.ascontiguousarray(g["link_num_spans"], np.int32), np.ascontiguousarray(g["link_span_length_km"], np.float64),
                np.ascontiguousarray(g["thresholds_db"], np.float64)]
        gg.link_num_spans, gg.link_span_length_km, gg.thresholds_db = (a.ctypes.data_as(C.c_void_p) for a in keep)
        gg.num_thresholds = len(keep[2])
        return gg, keep

    def qot_audit(self, gate=None, services=False, by_group=False, out=None):
        """The GN-model audit of every running lightpath (``orlg_gn_audit``; not in the reference): for every running
        service its GSNR against the OTHER running services of its environment over the links of its own path -- the victim
        evaluation of ``protect_running`` without a candidate -- and its margin to the threshold of its modulation.  A dict:

        ``n_running`` [B] int32, ``n_below`` [B] int32 (services with a margin below zero), ``min_margin_db`` [B] float64 (NaN where
        nothing runs) and ``worst_rank`` [B] int32 (the lowest rank that attains it, -1 where nothing runs);
        ``services=True`` adds ``gsnr_db``, ``margin_db``, ``osnr_ase_db`` and ``snr_nli_db``, [B, Q] float64 in the rank order of
        :meth:`running_services`, NaN past ``n_running`` (linear: 1 / GSNR = 1 / ase + 1 / nli);
        ``by_group=True`` adds ``by_group``: ``services``, ``below`` [G] int64 and ``min_margin_db`` [G] float64 (NaN for a group in
        which nothing runs), reduced on the host from the [B] arrays over the groups of a sweep handle.

        ``gate``: what :func:`rmsa_gn_gate_parameters` returns, for this call alone -- margins at another launch power, or the
        audit of traffic an ungated handle built; ``protect_running`` is ignored there, and the handle's own gate stays.  ``None``
        is the handle's gate; a handle without one raises ``ValueError``.  Served on gated, protecting and ungated handles, after
        either step kernel.  Reads state only.  ``out``: a dict of preallocated buffers -- the four [B, Q] names (numpy arrays or
        torch tensors; device tensors are written in place; naming one implies it is returned) and ``summary``, [B, 24] uint8, the
        ``orlg_gn_audit_summary`` records as the library writes them (the four [B] arrays are then views of it)."""
        if gate is None and self.gn_gate is None:
            raise ValueError("qot_audit: the handle has no GN-model admission check (gn_gate=); give the audit a gate= of its own")
        g = None if gate is None else _osnr.check_rmsa_gn_gate(gate, self.topology)
        out = dict(out or {})
        unknown = set(out) - set(self.AUDIT_SERVICE_FIELDS) - {"summary"}
        if unknown:
            raise ValueError(f"qot_audit: out= has no buffer named {sorted(unknown)}")
        B = self.batch_size
        summary = out.pop("summary", None)
        if summary is None:
            summary = np.zeros((B, 24), np.uint8)
        else:
            _check_buffer("out['summary']", summary, (B, 24), np.uint8)
        names = [n for n in self.AUDIT_SERVICE_FIELDS if services or n in out]
        res = self._rank_buffers([(n, np.float64, True) for n in names], out, "qot_audit")
        gg, keep = (None, None) if g is None else self._gn_gate_struct(g)
        _lib.check(self.L.orlg_gn_audit(self.h, None if gg is None else C.byref(gg), _ptr(summary),
                                        *(_ptr(res.get(n)) for n in self.AUDIT_SERVICE_FIELDS)))
        del keep
        if hasattr(summary, "data_ptr"):   # a torch tensor: views of the records, on its device
            import torch
            i32 = summary[:, :16].view(torch.int32)
            head = {"n_running": i32[:, 0], "n_below": i32[:, 1], "worst_rank": i32[:, 2],
                    "min_margin_db": summary[:, 16:].view(torch.float64)[:, 0]}
        else:
            rec = summary.view(_lib.GN_AUDIT_SUMMARY_DTYPE)[:, 0]
            head = {n: rec[n] for n in ("n_running", "n_below", "worst_rank", "min_margin_db")}
        if by_group:
            to_np = lambda a: a.cpu().numpy() if hasattr(a, "data_ptr") else a
            n, below, worst = (to_np(head[k]) for k in ("n_running", "n_below", "min_margin_db"))
            G = self.num_groups
            low = np.full(G, np.inf)
            np.fmin.at(low, self.groups, worst)   # (fmin: an environment in which nothing runs has NaN and does not count)
            running = np.bincount(self.groups, weights=n, minlength=G).astype(np.int64)
            head["by_group"] = {"services": running, "below": np.bincount(self.groups, weights=below, minlength=G).astype(np.int64),
                                "min_margin_db": np.where(low == np.inf, np.nan, low)}
        head.update(res)
        return head

    def simple_matrix_observation(self, out=None):
        """SimpleMatrixObservation.observation() for every env: [B, 2N + E*S] uint8 (``rmsa_env.py:940-971``)."""
        dim = self.L.orlg_simple_matrix_obs_dim(self.h)
        if out is None:
            out = np.zeros((self.batch_size, dim), np.uint8)
        else:
            _check_buffer("out", out, (self.batch_size, dim), np.uint8)
        _lib.check(self.L.orlg_simple_matrix_observation(self.h, _ptr(out)))
        return out

    def step_path_first_fit(self, paths, outputs=("reward", "done", "accepted")):
        """PathOnlyFirstFitAction.step for every env: ``paths`` is [B] int32 (k = reject)."""
        r = self.run("path_ff_external", 1, actions=paths, outputs=outputs)
        return {k: v[0] for k, v in r.items()}


class BatchedDeepRMSAEnv(BatchedRMSAEnv):
    """B x DeepRMSAEnv (``deeprmsa_env.py:9-46``): load = holding / inter-arrival, reward +1/-1, actions in
    Discrete(k*j + reject), observation = per-path free-block features."""

    def __init__(self, topology, batch_size: int, *, j: int = 1, episode_length: int = 1000,
                 mean_service_holding_time: float = None, mean_service_inter_arrival_time: float = None,
                 num_spectrum_resources: int = 100, node_request_probabilities=None, seed=None, seeds=None,
                 allow_rejection: bool = False, **extra):
        if extra.get("trace") is not None:   # (the means describe generated traffic)
            _trace.check_trace_kwargs(extra["trace"], dict(mean_service_holding_time=mean_service_holding_time,
                                                           mean_service_inter_arrival_time=mean_service_inter_arrival_time,
                                                           load=extra.get("load"), seed=seed, seeds=seeds))
            BatchedRMSAEnv.__init__(self, topology, batch_size, episode_length=episode_length,
                                    num_spectrum_resources=num_spectrum_resources,
                                    node_request_probabilities=node_request_probabilities, allow_rejection=allow_rejection,
                                    j=j, reward_mode=1, **extra)
            return
        mean_service_holding_time = 25.0 if mean_service_holding_time is None else mean_service_holding_time
        if mean_service_inter_arrival_time is None:
            mean_service_inter_arrival_time = 0.1
        # (either mean may be a length-B array-like: a load sweep, as BatchedRMSAEnv)
        if np.ndim(mean_service_holding_time) > 0 or np.ndim(mean_service_inter_arrival_time) > 0:
            mean_service_holding_time = np.asarray(mean_service_holding_time, np.float64)
            mean_service_inter_arrival_time = np.asarray(mean_service_inter_arrival_time, np.float64)
        super().__init__(topology, batch_size, episode_length=episode_length,
                         load=mean_service_holding_time / mean_service_inter_arrival_time,
                         mean_service_holding_time=mean_service_holding_time,
                         num_spectrum_resources=num_spectrum_resources,
                         node_request_probabilities=node_request_probabilities, seed=seed, seeds=seeds,
                         allow_rejection=allow_rejection, j=j, reward_mode=1, **extra)

    def step(self, actions, outputs=("reward", "done", "accepted")):
        return self.step_deeprmsa(actions, outputs=outputs)
