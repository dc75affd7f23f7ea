"""The CPU "protecting oracle" of the GN-model admission check that protects the running lightpaths (``include/orlg.h``
``orlg_set_gn_protect``), on top of the gated oracle of ``gn_gate_reference.py``: after the candidate's own check, one
``oracle.gn_osnr`` batch per step whose checks are the running services that share a link with the candidate -- each over the
links of its own path, its interferers the other running services on the link in provision order and the candidate last.  Helper
module of ``test_gn_protect_args.py`` and ``test_gpu_gn_protect.py``; nothing here touches a GPU.

The shadow holds (release time, frozenset of links, centre, bandwidth, SE, ordered links) of every admitted service.
"""
import functools

import numpy as np

import gn_gate_reference as ref
import oracle as orc
from conftest import load_topology
from gpu_support import device_log_in_oracle

NSF, JPN = "nsfnet_chen_5-paths_6-modulations", "jpn12_5-paths_6-modulations"
# the cases of the issue: gn_gate_reference.CASES with three seeds moved off a neighbour margin closer than 1e-4 dB to zero
CASES = {
    "nsfnet_s320_l50_sapff": dict(topology=NSF, S=320, load=50, seed=2, policy="sap_ff"),
    "nsfnet_s320_l150_sapff": dict(topology=NSF, S=320, load=150, seed=11, policy="sap_ff"),
    "nsfnet_s320_l150_llpff": dict(topology=NSF, S=320, load=150, seed=12, policy="llp_ff"),
    "nsfnet_s100_l20_spff": dict(topology=NSF, S=100, load=20, seed=13, policy="sp_ff"),
    "jpn12_s320_l150_sapff": dict(topology=JPN, S=320, load=150, seed=3, policy="sap_ff"),
    "ring34_s100_l60_sapff": dict(topology="ring34_3-paths_6-modulations", S=100, load=60, seed=7, policy="sap_ff"),
    "ring34_s320_l300_llpff": dict(topology="ring34_3-paths_6-modulations", S=320, load=300, seed=8, policy="llp_ff"),
    "ring36_s512_l500_sapff": dict(topology="ring36_3-paths_6-modulations", S=512, load=500, seed=11, policy="sap_ff"),
}
SAP_GN_CASES = ("nsfnet_s320_l50_sapff", "jpn12_s320_l150_sapff")   # the two the issue names for sap_ff_gn
N_STEPS = ref.N_STEPS
EPISODE_LENGTH = ref.EPISODE_LENGTH
B = 8   # environments per case on the device: seeds case seed + 0 .. 7


def case_kwargs(case, **over):
    c = CASES[case]
    return dict(dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=ref.HOLDING_TIME,
                     episode_length=EPISODE_LENGTH, seed=c["seed"]), **over)


def case_gate(topo, protect=True, **over):
    from optical_rl_gym_amd import rmsa_gn_gate_parameters
    return rmsa_gn_gate_parameters(topo, protect_running=protect, **dict(ref.GATE_KWARGS, **over))


class ProtectingOracle(ref.GatedOracle):
    """One oracle environment behind a gate that protects the running lightpaths."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.n_checks = self.n_rejects = 0     # neighbour checks that ran / that refused
        self.n_closest = np.inf                # the neighbour margin closest to zero
        self.max_affected = 0                  # most victims of one neighbour check
        self.n_max_running = 0                 # most running services at a neighbour check
        self.max_links_used = 0                # most links the running services lay on at one check
        self.links_used = set()                # the links running services lay on at any check
        self.max_abs_gsnr = 0.0                # largest |GSNR| computed (the tolerance of the margin scales with it)
        self.any_closest = np.inf              # closest margin of either kind over every candidate evaluated, proposals included

    # ---- the two checks of a candidate, without counting
    def gsnr(self, links, s, n):
        """GatedOracle.gsnr on this shadow (its entries carry the ordered links as a sixth field)"""
        full, self.shadow = self.shadow, [e[:5] for e in self.shadow]
        try:
            return super().gsnr(links, s, n)
        finally:
            self.shadow = full

    def neighbour_margin(self, links, s, n, se):
        """(min over the affected services of GSNR_i - threshold_i with the candidate lit -- NaN without one --, number affected)"""
        g, sh = self.gate, self.shadow
        cset = set(links)
        victims = [i for i, e in enumerate(sh) if cset & e[1]]
        if not victims:
            return np.nan, 0
        by_link = {}
        for i, e in enumerate(sh):   # provision order
            for l in e[5]:
                by_link.setdefault(l, []).append(i)
        cb, cf = self._window(s, n)
        span_off, svc_off, clo, lengths, sb, sf, sse, bw, fc, pw = [0], [0], [0], [], [], [], [], [], [], []
        for v in victims:
            _, _, f_v, b_v, _, vlinks = sh[v]
            for l in vlinks:
                ns = int(g["link_num_spans"][l])
                lengths += [float(g["link_span_length_km"][l])] * ns
                span_off.append(len(lengths))
                for i in by_link[l]:
                    if i != v:
                        sb.append(sh[i][3]); sf.append(sh[i][2]); sse.append(sh[i][4])
                if l in cset:   # the candidate, the last interferer
                    sb.append(cb); sf.append(cf); sse.append(se)
                svc_off.append(len(sb))
            clo.append(len(span_off) - 1)
            bw.append(b_v); fc.append(f_v); pw.append(g["launch_power_density_w_hz"] * b_v)
        n_sp = len(lengths)
        batch = dict(check_link_off=clo, link_span_off=span_off, link_svc_off=svc_off, bandwidth=bw, center_frequency=fc,
                     launch_power=pw, span_length_km=lengths, span_attenuation=[g["attenuation_normalized"]] * n_sp,
                     span_noise_figure=[g["noise_figure"]] * n_sp, svc_bandwidth=sb, svc_center_frequency=sf, svc_se=sse,
                     svc_is_self=[0] * len(sb))
        gs = orc.gn_osnr(batch)
        self.max_abs_gsnr = max(self.max_abs_gsnr, float(np.max(np.abs(gs))))
        thr = np.array([float(g["thresholds_db"][sh[v][4] - 1]) for v in victims])
        return float(np.min(gs - thr)), len(victims)

    def evaluate(self, p, s):
        """(gsnr, own check passed, neighbour margin (NaN = that check did not run), affected services) of a free window"""
        n = self.o.number_slots(p)
        links, se = self._path(p)
        gsnr = self.gsnr(links, s, n)
        self.max_abs_gsnr = max(self.max_abs_gsnr, abs(gsnr))
        thr = float(self.gate["thresholds_db"][se - 1])
        self.any_closest = min(self.any_closest, abs(gsnr - thr))
        if not gsnr >= thr:
            return gsnr, False, np.nan, 0
        margin, affected = self.neighbour_margin(links, s, n, se)
        if affected:
            self.any_closest = min(self.any_closest, abs(margin))
        return gsnr, True, margin, affected

    def _drop_due(self):
        now = self.o.current_time()
        self.shadow = [e for e in self.shadow if not e[0] <= now]

    # ---- proposals
    def propose_sap_ff_gn(self):
        """(path, slot, steps over a neighbour refusal) of sap_ff_gn under protection: the candidate paths in order, the first
        fit of the first path that passes BOTH checks; none passes: the first path with a fit (the step refuses it); no path has
        a fit: the rejection.  The third value: 1 iff a path is taken behind one that the neighbour check refused."""
        self._drop_due()
        first, neighbour_refused = None, 0
        for p in range(self.K):
            n = self.o.number_slots(p)
            starts, _ = self.o.available_blocks(p)
            if not (len(starts) and starts[0] < self.S - n):
                continue
            s = int(starts[0])
            if first is None:
                first = (p, s)
            _, own, margin, _ = self.evaluate(p, s)
            if own and not margin < 0:
                return p, s, neighbour_refused
            neighbour_refused |= int(own)
        return (first + (0,)) if first else (self.K, self.S, 0)

    # ---- one step
    def step(self, p, s):
        """Returns dict(act_path, act_slot, accepted, done, gsnr, margin (NaN = the check did not run), reward, request)."""
        o = self.o
        r = o.request()
        self._drop_due()
        self.max_running = max(self.max_running, len(self.shadow))
        gsnr, margin, admitted = np.nan, np.nan, False
        if 0 <= p < self.K and 0 <= s < self.S:
            n = o.number_slots(p)
            if o.is_path_free(p, s, n):
                links, se = self._path(p)
                gsnr, own, margin, affected = self.evaluate(p, s)
                thr = float(self.gate["thresholds_db"][se - 1])
                self.checks += 1
                self.closest = min(self.closest, abs(gsnr - thr))
                lit = {l for e in self.shadow for l in e[1]}
                self.links_used |= lit
                self.max_links_used = max(self.max_links_used, len(lit))
                self.link_ranges = max(self.link_ranges, len({l >> 6 for e in self.shadow for l in e[1]}))
                self.rejects += int(not own)
                if affected:
                    self.n_checks += 1
                    self.n_rejects += int(margin < 0)
                    self.n_closest = min(self.n_closest, abs(margin))
                    self.max_affected = max(self.max_affected, affected)
                    self.n_max_running = max(self.n_max_running, len(self.shadow))
                admitted = own and not margin < 0
                if admitted:
                    b, f = self._window(s, n)
                    self.shadow.append((r.arrival_time + r.holding_time, frozenset(links), f, b, se, tuple(links)))
        res = o.step(p, s) if admitted else o.step(self.K, self.S)
        assert bool(res.accepted) == admitted
        out = dict(act_path=p, act_slot=s, accepted=int(admitted), done=int(res.done), gsnr=gsnr, margin=margin, reward=res.reward,
                   request=(r.service_id, r.src, r.dst, r.bit_rate))
        if res.done:
            o.reset(only_episode_counters=True)
        return out

    def run(self, policy, n_steps):
        rows, later = [], 0
        for _ in range(n_steps):
            if policy == "sap_ff_gn":
                p, s, behind = self.propose_sap_ff_gn()
                rows.append(self.step(p, s))
                later += behind and rows[-1]["accepted"]
            else:
                rows.append(self.step(*self.propose(policy)))
        self.later_taken = later
        return {k: np.array([row[k] for row in rows]) for k in rows[0]}

    def figures(self):
        return dict(checks=self.checks, rejects=self.rejects, closest=self.closest, n_checks=self.n_checks, n_rejects=self.n_rejects,
                    n_closest=self.n_closest, max_affected=self.max_affected, max_running=self.max_running,
                    n_max_running=self.n_max_running, max_links_used=self.max_links_used, links_used=len(self.links_used), link_ranges=self.link_ranges,
                    max_abs_gsnr=self.max_abs_gsnr, any_closest=self.any_closest, later_taken=getattr(self, "later_taken", 0))


def final_state(o):
    return dict(available_slots=o.available_slots(), counters=o.counters(), num_running=o.num_running(), current_time=o.current_time())


def run_case(case, seed=None, n_steps=N_STEPS, policy=None, gate_items=()):
    """The protecting oracle of a case -- a name of CASES or a (topology, kwargs) pair with its `policy`, as
    gn_gate_reference.run_case takes one -- (seed, policy: the case's own by default; a pair's seed is its kwargs'), run once per
    process and shared: (per-step arrays, final state, figures).  Read-only by agreement."""
    if isinstance(case, str):
        seed, policy = CASES[case]["seed"] if seed is None else seed, policy or CASES[case]["policy"]
    else:
        assert policy is not None, "a (topology, kwargs) case has no policy of its own"
        seed = case[1]["seed"] if seed is None else seed
    return _run_case(ref.cache_key(case), seed, n_steps, policy, tuple(gate_items))


@functools.lru_cache(maxsize=None)
def _run_case(key, seed, n_steps, policy, gate_items):
    if isinstance(key, str):
        topo, kw = load_topology(CASES[key]["topology"]), case_kwargs(key)
    else:
        topo, kw, _ = ref.resolve_case((key[0], dict(key[1])), policy)
    with device_log_in_oracle():
        po = ProtectingOracle(topo, kw, case_gate(topo, **dict(gate_items)), seed=seed)
        tr = po.run(policy, n_steps)
    final, fig = final_state(po.o), po.figures()
    po.close()
    for a in tr.values():
        a.setflags(write=False)
    return tr, final, fig


def run_batch(case, n_steps=N_STEPS, policy=None, batch=B, gate_items=()):
    """run_case for the seeds case seed + 0 .. batch - 1 (a (topology, kwargs) pair's seed is its kwargs')"""
    seed = CASES[case]["seed"] if isinstance(case, str) else case[1]["seed"]
    return [run_case(case, seed=seed + i, n_steps=n_steps, policy=policy, gate_items=gate_items) for i in range(batch)]
