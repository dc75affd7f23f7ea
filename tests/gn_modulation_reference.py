"""The CPU reference of adaptive modulation behind the GN gate (``include/orlg.h`` ``orlg_set_gn_modulation``,
``orlg_step_modulation``): ``sp_ff_am``, ``sap_ff_am``, ``path_am_external`` and ``external_am`` restated on top of
``gn_gate_reference.GatedOracle``, without touching ``oracle/``.

The oracle environment runs on an EXPANDED topology: every pair has ``k * M`` paths, path ``p * M + (m - 1)`` is path ``p`` with
spectral efficiency ``m``.  The request stream and the statistics do not depend on ``k``, so ``number_slots``, ``is_path_free`` and
``step`` of the oracle serve a (path, level) candidate as they serve a path, and the shadow list carries every service's level: a
running service interferes with the level it was provisioned at.  Helper module of ``test_gn_modulation_args.py`` and
``test_gpu_gn_modulation.py``; nothing here touches a GPU.
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
ROUTES = {"sp_ff_am": "sp", "sap_ff_am": "sap", "path_am_external": "path"}


def case_kwargs(case, **over):
    c = CASES[case]
    return dict(dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=ref.HOLDING_TIME,
                     episode_length=ref.EPISODE_LENGTH, seed=c["seed"], **c.get("extra", {})), **over)


def case_gate(topo, dbm, **over):
    from optical_rl_gym_amd import rmsa_gn_gate_parameters
    return rmsa_gn_gate_parameters(topo, **dict(dict(launch_power_dbm_per_50ghz=dbm, modulation="adaptive"), **over))


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


def first_fit(free, n, S):
    """the reference's first fit (rmsa_env.py:860-871): the smallest s in [0, S - n) with free[s : s + n] all set, None = no window"""
    if S - n <= 0:
        return None
    c = np.concatenate(([0], np.cumsum(free, dtype=np.int64)))
    ok = np.flatnonzero((c[n:] - c[:-n])[:S - n] == n)
    return int(ok[0]) if ok.size else None


class AdaptiveOracle(ref.GatedOracle):
    """One oracle environment behind a gate that chooses the modulation.  A candidate is (path p of the base topology, level m)."""

    def __init__(self, topo, kw, gate, seed=None):
        self.base, self.M = topo, len(gate["thresholds_db"])
        super().__init__(expanded(topo, self.M), kw, gate, seed=seed)
        self.K = topo.k_paths          # the policies' paths; the oracle's own index of candidate (p, m) is xp(p, m)
        self.KX = self.K * self.M
        self.levels = []               # per accepted service: (level, the path's own spectral efficiency)
        self.checks_per_step = []
        self.refused_after = []        # levels checked by the steps that ended as a gate refusal
        self.admitted_margins = []
        self.meta = {}                 # release time -> (ordered links, first slot, slots, global path index, bit rate)

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
        self.shadow = [e for e in self.shadow if not e[0] <= now]
        self.max_running = max(self.max_running, len(self.shadow))

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
                   request=(r.service_id, r.src, r.dst, r.bit_rate))
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
        """sp_ff / sap_ff on an adaptive handle: the path's own spectral efficiency, checked once (what a plain gated handle does),
        against services that carry their levels"""
        self._begin()
        avail = self.o.available_slots()
        shown, chosen, n_checked = (self.K, self.S, 0, np.nan), None, 0
        for p in ([0] if route == "sp" else range(self.K)):
            m = self.path_se(p)
            links, _ = self._path(self.xp(p, m))
            n = self.o.number_slots(self.xp(p, m))
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
        o = self.o
        return dict(available_slots=o.available_slots(), counters=o.counters(), num_running=o.num_running(), current_time=o.current_time())

    def figures(self):
        lv = np.array(self.levels).reshape(-1, 2)
        return dict(checks=self.checks, rejects=self.rejects, max_running=self.max_running, closest=self.closest, link_ranges=self.link_ranges,
                    accepted=len(lv), other_level=int((lv[:, 0] != lv[:, 1]).sum()), refused_after=max(self.refused_after, default=0),
                    max_checks=max(self.checks_per_step, default=0), mean_checks=float(np.mean(self.checks_per_step)) if self.checks_per_step else 0.0,
                    min_admitted_margin=min(self.admitted_margins, default=np.nan))


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
