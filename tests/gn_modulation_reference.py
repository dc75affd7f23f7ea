"""The CPU reference of adaptive modulation behind the GN gate (``include/orlg.h`` ``orlg_set_gn_modulation``,
``orlg_step_modulation``): ``sp_ff_am``, ``sap_ff_am``, ``path_am_external`` and ``external_am`` restated on top of
``gn_gate_reference.GatedOracle``, without touching ``oracle/``.

The oracle environment runs on an EXPANDED topology: every pair has ``k * M`` paths, path ``p * M + (m - 1)`` is path ``p`` with
spectral efficiency ``m``.  The request stream and the statistics do not depend on ``k``, so ``number_slots``, ``is_path_free`` and
``step`` of the oracle serve a (path, level) candidate as they serve a path, and the shadow list carries every service's level: a
running service interferes with the level it was provisioned at.  Helper module of ``test_gn_modulation_args.py``,
``test_gpu_gn_modulation.py`` and ``test_gpu_gn_modulation_shapes.py`` (the table ``SHAPES``); nothing here touches a GPU.
"""
import functools

import numpy as np

import gn_gate_reference as ref
from conftest import load_topology
from gpu_support import device_log_in_oracle

NSF, JPN, RING34 = "nsfnet_chen_5-paths_6-modulations", "jpn12_5-paths_6-modulations", "ring34_3-paths_6-modulations"
B = 8
# the cases of the issue: one launch of `n` steps of sap_ff_am, environment i on seed + i
CASES = {
    "nsfnet_s320_l50_0dbm": dict(topology=NSF, S=320, load=50, seed=10, dbm=0.0, n=200),
    "nsfnet_s320_l50_6dbm": dict(topology=NSF, S=320, load=50, seed=10, dbm=6.0, n=200),
    "nsfnet_s320_l150_0dbm": dict(topology=NSF, S=320, load=150, seed=11, dbm=0.0, n=200),   # more than 64 running services
    "jpn12_s320_l150_6dbm": dict(topology=JPN, S=320, load=150, seed=3, dbm=6.0, n=150),
    "ring34_s100_l60_6dbm": dict(topology=RING34, S=100, load=60, seed=7, dbm=6.0, n=150),   # link masks of four words
    "nsfnet_s64_l12_6dbm": dict(topology=NSF, S=64, load=12, seed=20, dbm=6.0, n=150),       # one word per link
    "nsfnet_s128_l25_6dbm": dict(topology=NSF, S=128, load=25, seed=21, dbm=6.0, n=150),     # two
    "nsfnet_s512_l100_6dbm": dict(topology=NSF, S=512, load=100, seed=22, dbm=6.0, n=150),   # eight
    # every integer rate 600 .. 855: all 8 bits of a descriptor's rate index in use
    "nsfnet_s320_l50_continuous": dict(topology=NSF, S=320, load=50, seed=23, dbm=6.0, n=150,
                                       extra=dict(bit_rate_selection="continuous", bit_rate_lower_bound=600, bit_rate_higher_bound=855)),
}
# the shapes of test_gpu_gn_modulation_shapes.py beyond CASES (test_gn_modulation_args.py pins on the reference what each one reaches).
# M: the gate keeps the first M default thresholds and the topology is clipped(topo, M); B: environments (default 8);
# queue_margin: the device ring gets the reference's peak + this margin, rounded as orlg_create rounds it
SHAPES = {
    "m3_6dbm": dict(topology=NSF, S=128, load=25, seed=21, dbm=6.0, n=150, M=3),
    "m3_0dbm": dict(topology=NSF, S=128, load=25, seed=21, dbm=0.0, n=150, M=3),
    "m1_6dbm": dict(topology=NSF, S=128, load=25, seed=21, dbm=6.0, n=150, M=1),
    "m1_0dbm": dict(topology=NSF, S=128, load=25, seed=21, dbm=0.0, n=150, M=1),
    "chunks3": dict(topology=NSF, S=320, load=250, seed=11, dbm=0.0, n=300, B=4),             # more than 128 running services
    "lap": dict(topology=NSF, S=128, load=25, seed=21, dbm=6.0, n=250, queue_margin=8),       # the ring's head passes Q twice
}
# the shapes of gpu_support.MANY_PATHS an adaptive handle takes (fewer than 2048 path records), at +6 dBm; `load`: where sap_ff_am
# reaches the paths 8 and above (at the shapes' own loads it accepts 0 .. 3 services there per environment)
MANY = {
    "g3x3_k9_s64": dict(load=11, n=300),      # 12 services accepted on path 8 by the eight environments together
    "g4x4_k16_s200": dict(load=150, n=150),   # 33 on paths 8 .. 15
    "g3x4_k10_s384": dict(load=800, n=300),   # 14 on paths 8 and 9
}
MANY_REFUSED = "g4x4_k21_s192"   # 2520 path records
ROUTES = {"sp_ff_am": "sp", "sap_ff_am": "sap", "path_am_external": "path"}


def case_kwargs(case, **over):
    c = CASES[case] if case in CASES else SHAPES[case]
    return dict(dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=ref.HOLDING_TIME,
                     episode_length=ref.EPISODE_LENGTH, seed=c["seed"], **c.get("extra", {})), **over)


def case_gate(topo, dbm, **over):
    from optical_rl_gym_amd import rmsa_gn_gate_parameters
    return rmsa_gn_gate_parameters(topo, **dict(dict(launch_power_dbm_per_50ghz=dbm, modulation="adaptive"), **over))


def shape_gate(topo, dbm, M=None, **over):
    """case_gate with the first M of the default thresholds (M = None: all of them)"""
    g = case_gate(topo, dbm, **over)
    return g if M is None else case_gate(topo, dbm, **dict(over, thresholds_db=np.asarray(g["thresholds_db"], np.float64)[:M].copy()))


def ring_capacity(peak, margin):
    """what orlg_create makes of queue_capacity = peak + margin: whole rows of 16 slots, 64 at the least"""
    return max(64, -(-(peak + margin) // 16) * 16)


@functools.lru_cache(maxsize=None)
def expanded(topo, M, only_se=None):
    """The topology with k * M paths per pair: path p * M + (m - 1) is path p with spectral efficiency m (only_se: every path with
    that one spectral efficiency instead, k paths per pair)."""
    from optical_rl_gym_amd import FrozenTopology
    d = topo.to_json()
    paths = {}
    for key, plist in d["paths"].items():
        if only_se is None:
            paths[key] = [[int(p[0]) * M + m - 1, p[1], p[2], m, p[4]] for p in plist for m in range(1, M + 1)]
        else:
            paths[key] = [[p[0], p[1], p[2], only_se, p[4]] for p in plist]
    d["paths"] = paths
    if only_se is None:
        d["k_paths"] = topo.k_paths * M
    return FrozenTopology.from_json(d)


@functools.lru_cache(maxsize=None)
def clipped(topo, M):
    """The topology with every path's spectral efficiency cut to min(se, M): what a gate of M levels takes (built as `expanded` is)."""
    from optical_rl_gym_amd import FrozenTopology
    d = topo.to_json()
    d["paths"] = {key: [[p[0], p[1], p[2], min(int(p[3]), M), p[4]] for p in plist] for key, plist in d["paths"].items()}
    return FrozenTopology.from_json(d)


def first_fit(free, n, S):
    """the reference's first fit (rmsa_env.py:860-871): the smallest s in [0, S - n) with free[s : s + n] all set, None = no window"""
    if S - n <= 0:
        return None
    c = np.concatenate(([0], np.cumsum(free, dtype=np.int64)))
    ok = np.flatnonzero((c[n:] - c[:-n])[:S - n] == n)
    return int(ok[0]) if ok.size else None


class AdaptiveOracle(ref.GatedOracle):
    """One oracle environment behind a gate that chooses the modulation.  A candidate is (path p of the base topology, level m)."""

    def __init__(self, topo, kw, gate, seed=None, j=1, reward_mode=0):
        self.base, self.M = topo, len(gate["thresholds_db"])
        super().__init__(expanded(topo, self.M), kw, gate, seed=seed, j=j, reward_mode=reward_mode)
        self.K = topo.k_paths          # the policies' paths; the oracle's own index of candidate (p, m) is xp(p, m)
        self.KX = self.K * self.M
        self.levels = []               # per accepted service: (level, the path's own spectral efficiency)
        self.checks_per_step = []
        self.refused_after = []        # levels checked by the steps that ended as a gate refusal
        self.admitted_margins = []
        self.meta = {}                 # release time -> (ordered links, first slot, slots, global path index, bit rate)
        self.level_of = {}             # release time -> (level, the path's own spectral efficiency)
        self.releases = []             # per release, in order: (the step whose start released it, level, the path's own)
        self.running_at = []           # per step: the services still running when its request is served

    def xp(self, p, m):
        return p * self.M + (m - 1)

    def path_se(self, p):
        t, r = self.base, self.o.request()
        return int(t.path_se[int(t.pair_path_base[r.src * t.num_nodes + r.dst]) + p])

    def path_gid(self, p):
        t, r = self.base, self.o.request()
        return int(t.pair_path_base[r.src * t.num_nodes + r.dst]) + p

    def _begin(self):
        now = self.o.current_time()
        t = len(self.running_at)
        self.releases += [(t,) + self.level_of[e[0]] for e in sorted(self.shadow, key=lambda e: e[0]) if e[0] <= now]
        self.shadow = [e for e in self.shadow if not e[0] <= now]
        self.max_running = max(self.max_running, len(self.shadow))
        self.running_at.append(len(self.shadow))

    def _check(self, p, m, s, n):
        links, se = self._path(self.xp(p, m))
        assert se == m
        g = self.gsnr(links, s, n)
        thr = float(self.gate["thresholds_db"][m - 1])
        self.checks += 1
        self.link_ranges = max(self.link_ranges, len({l >> 6 for e in self.shadow for l in e[1]}))
        self.closest = min(self.closest, abs(g - thr))
        return g, g >= thr

    def _finish(self, shown, chosen, n_checked):
        """shown = (p, s, m, gsnr) the step's outputs name, chosen = the admitted candidate or None"""
        o, r = self.o, self.o.request()
        if chosen is not None:
            p, s, m, g = chosen
            n = o.number_slots(self.xp(p, m))
            links, _ = self._path(self.xp(p, m))
            b, f = self._window(s, n)
            self.levels.append((m, self.path_se(p)))
            self.admitted_margins.append(g - float(self.gate["thresholds_db"][m - 1]))
            release = r.arrival_time + r.holding_time
            self.shadow.append((release, frozenset(links), f, b, m))
            self.meta[release] = (tuple(links), s, n, self.path_gid(p), int(r.bit_rate))   # (release times are distinct draws)
            self.level_of[release] = (m, self.path_se(p))
            res = o.step(self.xp(p, m), s)
            assert res.accepted
        else:
            res = o.step(self.KX, self.S)
            assert not res.accepted
            if n_checked:
                self.rejects += 1
                self.refused_after.append(n_checked)
        self.checks_per_step.append(n_checked)
        p, s, m, g = shown
        out = dict(act_path=p, act_slot=s, gn_se=m, accepted=int(chosen is not None), done=int(res.done), gsnr=g, reward=res.reward,
                   request=(r.service_id, r.src, r.dst, r.bit_rate), arrival=r.arrival_time, holding=r.holding_time,
                   network_compactness=res.network_compactness, network_compactness_difference=res.network_compactness_difference,
                   avg_link_compactness=res.avg_link_compactness, avg_link_utilization=res.avg_link_utilization,
                   n_checked=n_checked, n_running=self.running_at[-1])   # (the candidates checked; the services that interfere)
        if res.done:
            o.reset(only_episode_counters=True)
        return out

    def levels_of_path(self, p, avail=None):
        """[(m, s, n, gsnr, admitted)] for the levels M .. 1 of path p that have a window, with no early exit on an admission"""
        avail = self.o.available_slots() if avail is None else avail
        links, _ = self._path(self.xp(p, 1))
        free = avail[links].all(axis=0)
        rows = []
        for m in range(self.M, 0, -1):
            n = self.o.number_slots(self.xp(p, m))
            s = first_fit(free, n, self.S)
            if s is None:
                break
            g, ok = self._check(p, m, s, n)
            rows.append((m, s, n, g, ok))
        return rows

    def step_route(self, route, given=None):
        """sp_ff_am / sap_ff_am / path_am_external (route "sp" / "sap" / "path" with the path `given`)"""
        self._begin()
        K = self.K
        scope = [0] if route == "sp" else list(range(K)) if route == "sap" else ([int(given)] if 0 <= int(given) < K else [])
        avail = self.o.available_slots()
        first, chosen, n_checked = None, None, 0
        for p in scope:
            links, _ = self._path(self.xp(p, 1))
            free = avail[links].all(axis=0)
            for m in range(self.M, 0, -1):
                n = self.o.number_slots(self.xp(p, m))
                s = first_fit(free, n, self.S)
                if s is None:
                    break
                g, ok = self._check(p, m, s, n)
                n_checked += 1
                if first is None:
                    first = (p, s, m, g)
                if ok:
                    chosen = (p, s, m, g)
                    break
            if chosen is not None:
                break
        shown = chosen or first or (K, self.S, 0, np.nan)
        return self._finish(shown, chosen, n_checked)

    def step_external(self, p, s, m):
        """external_am: the agent's (path, slot, se); an se outside 1..M, a path or slot out of range, an occupied window: no check"""
        self._begin()
        chosen, g, shown_m, n_checked = None, np.nan, 0, 0
        if 1 <= m <= self.M and 0 <= p < self.K and 0 <= s < self.S:
            n = self.o.number_slots(self.xp(p, m))
            if self.o.is_path_free(self.xp(p, m), s, n):
                g, ok = self._check(p, m, s, n)
                n_checked, shown_m = 1, m
                if ok:
                    chosen = (p, s, m, g)
        return self._finish((p, s, shown_m, g), chosen, n_checked)

    def step_own_se(self, route):
        """sp_ff / sap_ff / deeprmsa_sap_ff (route "sp" / "sap" / "deeprmsa_sap") on an adaptive handle: the path's own spectral
        efficiency, checked once (what a plain gated handle does), against services that carry their levels"""
        self._begin()
        avail = self.o.available_slots()
        shown, chosen, n_checked = (self.K, self.S, 0, np.nan), None, 0
        for p in ([0] if route == "sp" else range(self.K)):
            m = self.path_se(p)
            links, _ = self._path(self.xp(p, m))
            n = self.o.number_slots(self.xp(p, m))
            if route == "deeprmsa_sap":   # the first block of >= n free slots, wherever it lies (deeprmsa_env.py:48-58)
                starts, _ = self.o.available_blocks(self.xp(p, m))
                s = int(starts[0]) if len(starts) else None
            else:
                s = first_fit(avail[links].all(axis=0), n, self.S)
            if s is not None:
                g, ok = self._check(p, m, s, n)
                n_checked = 1
                shown = (p, s, m, g)
                chosen = shown if ok else None
                break
        row = self._finish(shown, chosen, n_checked)
        row["gn_se"] = 0   # (no level was chosen: the device stores and shows 0, the path's own)
        return row

    def run_route(self, route, n_steps, given=None):
        rows = [self.step_route(route, None if given is None else given[t]) for t in range(n_steps)]
        return {k: np.array([row[k] for row in rows]) for k in rows[0]}

    def drop_due(self):
        now = self.o.current_time()
        self.shadow = [e for e in self.shadow if not e[0] <= now]

    def services(self):
        """the running services in rank order (ascending release time), the due ones dropped: [(links, s, n, se)], path gids, rates"""
        self.drop_due()
        order = sorted(self.shadow, key=lambda e: e[0])
        meta = [self.meta[e[0]] for e in order]
        return [(m[0], m[1], m[2], e[4]) for m, e in zip(meta, order)], [m[3] for m in meta], [m[4] for m in meta], [e[0] for e in order]

    def final(self):
        o, r = self.o, self.o.request()
        return dict(available_slots=o.available_slots(), counters=o.counters(), num_running=o.num_running(), current_time=o.current_time(),
                    link_stats=o.link_stats(), graph_stats=o.graph_stats(), bit_rate_hist=o.bit_rate_hist(),
                    request=(r.service_id, r.src, r.dst, r.bit_rate, r.arrival_time, r.holding_time))

    def figures(self):
        lv = np.array(self.levels).reshape(-1, 2)
        return dict(checks=self.checks, rejects=self.rejects, max_running=self.max_running, closest=self.closest, link_ranges=self.link_ranges,
                    accepted=len(lv), other_level=int((lv[:, 0] != lv[:, 1]).sum()), refused_after=max(self.refused_after, default=0),
                    max_checks=max(self.checks_per_step, default=0), mean_checks=float(np.mean(self.checks_per_step)) if self.checks_per_step else 0.0,
                    min_admitted_margin=min(self.admitted_margins, default=np.nan), released=len(self.releases),
                    # releases of a service whose level is not its path's own, before the last step
                    released_other=sum(1 for t, m, se in self.releases if m != se and t < len(self.running_at) - 1),
                    peak_step=int(np.argmax(self.running_at)) if self.running_at else 0)


def run_case(case, i=0, route="sap", n_steps=None):
    """Environment i of a case stepped by the reference's own choices: (per-step arrays, final state, figures, services at the end).
    Run once per process and shared; read-only by agreement."""
    return _run_case(case, i, route, n_steps)


@functools.lru_cache(maxsize=None)
def _run_case(case, i, route, n_steps):
    c = CASES[case]
    topo = load_topology(c["topology"])
    kw = case_kwargs(case)
    with device_log_in_oracle():
        ao = AdaptiveOracle(topo, kw, case_gate(topo, c["dbm"]), seed=c["seed"] + i)
        tr = ao.run_route(route, n_steps or c["n"])
        final, figures, services = ao.final(), ao.figures(), ao.services()
        ao.close()
    for a in tr.values():
        a.setflags(write=False)
    return tr, final, figures, services


def run_shape(shape, i=0, route="sap", n_steps=None, topo=None, load=None):
    """run_case for a name of SHAPES, or -- with `topo` (one object per topology: cached by identity) and `load` -- of MANY at +6 dBm
    on seed 3 + i."""
    return _run_shape(shape, i, route, n_steps, topo, load)


@functools.lru_cache(maxsize=None)
def _golden(name):
    return load_topology(name)   # (one object per topology: `clipped` and `expanded` are cached by it)


def shape_setup(shape, topo=None, load=None):
    """(topology, keyword arguments, gate, seed of environment 0, steps) of a name of SHAPES or MANY"""
    if shape in MANY:
        from gpu_support import MANY_PATHS_SEED, many_paths_kwargs
        kw = many_paths_kwargs(shape, load=MANY[shape]["load"] if load is None else load)
        return topo, kw, case_gate(topo, 6.0), MANY_PATHS_SEED, MANY[shape]["n"]
    c = SHAPES[shape]
    M = c.get("M")
    topo = _golden(c["topology"]) if topo is None else topo
    topo = topo if M is None else clipped(topo, M)
    return topo, case_kwargs(shape), shape_gate(topo, c["dbm"], M), c["seed"], c["n"]


@functools.lru_cache(maxsize=None)
def _run_shape(shape, i, route, n_steps, topo, load):
    topo, kw, gate, seed, n = shape_setup(shape, topo, load)
    with device_log_in_oracle():
        ao = AdaptiveOracle(topo, kw, gate, seed=seed + i)
        tr = ao.run_route(route, n_steps or n)
        final, figures, services = ao.final(), ao.figures(), ao.services()
        ao.close()
    for a in tr.values():
        a.setflags(write=False)
    return tr, final, figures, services


# releases of services with and without a level interleave (the plan of test_existing_policies_on_an_adaptive_handle)
MIXED_CASE = "nsfnet_s320_l50_6dbm"
MIXED_PLAN = (("sap_ff_am", 40), ("sap_ff", 30), ("sap_ff_am", 30), ("sp_ff", 20), ("sap_ff_am", 20))


@functools.lru_cache(maxsize=None)
def run_mixed(i):
    """Environment i of MIXED_CASE through MIXED_PLAN: (per-step arrays of the whole plan, final state, figures, services at the end)"""
    c = CASES[MIXED_CASE]
    topo = load_topology(c["topology"])
    with device_log_in_oracle():
        ao = AdaptiveOracle(topo, case_kwargs(MIXED_CASE), case_gate(topo, c["dbm"]), seed=c["seed"] + i)
        rows = [ao.step_route("sap") if p == "sap_ff_am" else ao.step_own_se(p[:-3]) for p, n in MIXED_PLAN for _ in range(n)]
        final, figures, services = ao.final(), ao.figures(), ao.services()
        ao.close()
    tr = {k: np.array([row[k] for row in rows]) for k in rows[0]}
    for a in tr.values():
        a.setflags(write=False)
    return tr, final, figures, services


# per-environment loads (make_sweep: environment g * seeds_per_load + r runs loads[g] on seed + r) and a DeepRMSA handle
SWEEP = dict(topology=NSF, S=128, loads=(10, 40), seeds_per_load=3, seed=5, dbm=6.0, n=150)
DEEP = dict(topology=NSF, S=100, load=20, seed=13, dbm=6.0, n=150, n_own=20, j=2, B=4)


def sweep_kwargs(i):
    c = SWEEP
    return dict(num_spectrum_resources=c["S"], load=c["loads"][i // c["seeds_per_load"]], mean_service_holding_time=ref.HOLDING_TIME,
                episode_length=ref.EPISODE_LENGTH, seed=c["seed"] + i % c["seeds_per_load"])


def deep_kwargs():
    c = DEEP
    return dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=25.0, episode_length=1000, seed=c["seed"])


@functools.lru_cache(maxsize=None)
def run_sweep(i):
    topo, kw = _golden(SWEEP["topology"]), sweep_kwargs(i)
    with device_log_in_oracle():
        ao = AdaptiveOracle(topo, kw, case_gate(topo, SWEEP["dbm"]), seed=kw["seed"])
        tr = ao.run_route("sap", SWEEP["n"])
        final, figures, services = ao.final(), ao.figures(), ao.services()
        ao.close()
    return tr, final, figures, services


@functools.lru_cache(maxsize=None)
def run_deep(i):
    """environment i of the DeepRMSA handle (j blocks per path, reward +1 / -1): n steps of sap_ff_am, then n_own of deeprmsa_sap_ff"""
    c, topo = DEEP, _golden(DEEP["topology"])
    with device_log_in_oracle():
        ao = AdaptiveOracle(topo, deep_kwargs(), case_gate(topo, c["dbm"]), seed=c["seed"] + i, j=c["j"], reward_mode=1)
        tr = ao.run_route("sap", c["n"])
        own = [ao.step_own_se("deeprmsa_sap") for _ in range(c["n_own"])]
        final, figures, services = ao.final(), ao.figures(), ao.services()
        ao.close()
    return tr, {k: np.array([row[k] for row in own]) for k in own[0]}, final, figures, services
