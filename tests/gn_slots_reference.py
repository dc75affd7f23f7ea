"""The CPU reference of the GN-model admission check over the whole spectrum (``include/orlg.h`` ``orlg_gn_admission_slots``, DESIGN
2.31): the admission oracle of ``gn_admission_reference.py`` asked, before each step and after the services due by now are dropped,
about EVERY free window of every candidate path -- what ``evaluate(p, s)`` says for every ``p`` and every ``s in range(S - n + 1)``
with ``is_path_free``.  From those: the mask, the GSNR and neighbour-margin rows, the worst margin ``w`` of every admitted window, the
best window of every path.  Then the case's policy steps.  Helper module of ``test_gn_slots_args.py`` and ``test_gpu_gn_slots.py``;
nothing here touches a GPU.
"""
import functools

import numpy as np

import gn_admission_reference as adm
import gn_gate_reference as ref
import gn_protect_reference as pref
import gn_shapes_reference as sh
import oracle as orc
from gpu_support import MANY_PATHS, device_log_in_oracle, many_paths_kwargs, many_paths_topology, topology, write_topology

MIN_COUNT = 10            # windows of each kind per batch, and paths whose best window is not their first free one
MARGIN_DB = sh.MARGIN_DB  # a mask bit is compared where the reference's deciding margin is at least this far from zero
MAX_LEFT_OUT = 1e-4       # ... which may leave out at most 0.01 % of the free windows of a batch
BEST_TOL_DB = 1e-6        # w_ref[best_slot] >= max(w_ref) - BEST_TOL_DB

K32 = "g4x4_k32_s100"     # the shape with more than eight candidate paths: k = 32, W = 2, four passes of eight paths
# three nodes, three links, two paths per pair, S = 512 and services of two or three slots: after 130 steps about 110 services run
# and up to 81 of them share a link with one path -- two chunks of compacted services in the own check, two ring chunks per victim
TRI = "tri3_k2_s512"
TRI_KW = dict(num_spectrum_resources=512, load=300, mean_service_holding_time=25, episode_length=1000, seed=3, bit_rates=(25, 50))
_tri = {}


def tri_topology(tmp_path):
    """the topology of TRI, frozen once per process (the link list is written under the first caller's tmp_path)"""
    if TRI not in _tri:
        from optical_rl_gym_amd.topology_io import topology_from_txt
        _tri[TRI] = topology_from_txt(write_topology(tmp_path, TRI, 3, [(1, 2, 300), (2, 3, 400), (1, 3, 500)]), TRI, k_paths=2)
    return _tri[TRI]


# the batches of test_gpu_gn_slots.py: a case of gn_protect_reference.CASES (or one of the two shapes above) -> environments, steps with the query
# before each, steps of the case's policy before the first query, whether the handle protects, and the handle's keywords beyond
# the case's
BATCHES = {
    "nsfnet_s100_l20_spff": dict(B=8, n=100, warmup=0, protect=True, handle={}),
    "jpn12_s320_l150_sapff": dict(B=4, n=40, warmup=0, protect=True, handle=dict(queue_capacity=128)),
    "ring34_s320_l300_llpff": dict(B=2, n=60, warmup=90, protect=True, handle={}),
    "ring36_s512_l500_sapff": dict(B=2, n=40, warmup=0, protect=True, handle={}),
    K32: dict(B=2, n=40, warmup=30, protect=True, handle={}),
    TRI: dict(B=2, n=4, warmup=130, protect=True, handle={}),
    "gated:nsfnet_s320_l150_sapff": dict(B=2, n=20, warmup=100, protect=False, handle={}),
    # the word counts no other batch has -- one, three, four and six words per link -- on the shapes of gpu_support.MANY_PATHS (k > 8:
    # the path's words W lanes apart): 60 steps of the shape's own policy, then 40 with the query
    "g3x3_k9_s64": dict(B=2, n=40, warmup=60, protect=True, handle={}),
    "g4x4_k21_s192": dict(B=2, n=40, warmup=60, protect=True, handle={}),
    "g4x4_k16_s200": dict(B=2, n=40, warmup=60, protect=True, handle={}),
    "g3x4_k10_s384": dict(B=2, n=40, warmup=60, protect=True, handle={}),
}
WORDS = ("g3x3_k9_s64", "g4x4_k21_s192", "g4x4_k16_s200", "g3x4_k10_s384")   # W = 1, 3, 4, 6: there for their shape, outside COUNTED
COUNTED = ("nsfnet_s100_l20_spff", "jpn12_s320_l150_sapff", "ring34_s320_l300_llpff", "ring36_s512_l500_sapff")   # every kind of window
SEEDS = {}   # batch -> the first seed of the batch where it had to move off the case's own to meet a condition (none had to)


def _tile(off, nw):
    """an offset array (0 .. T) repeated nw times, each copy shifted by T: the offsets of nw equal checks in one batch"""
    off = np.asarray(off, np.int64)
    T = int(off[-1])
    return np.concatenate([(off[None, :-1] + T * np.arange(nw, dtype=np.int64)[:, None]).ravel(), [nw * T]])


class SlotsOracle(adm.AdmissionOracle):
    """An admission oracle that also answers, before a step, what every free window of every path would meet.  The windows of a
    path differ in their centre frequency alone, so slots() sends them through ``oracle.gn_osnr`` as ONE batch per path and check
    -- the lists of ``GatedOracle.gsnr`` and ``ProtectingOracle.neighbour_margin`` built once and repeated per window: every
    check of a batch is evaluated on its own, so the values are those of ``evaluate(p, s)`` window by window, bit for bit
    (cross_check, asserted in test_gn_slots_args.py), at a tenth of the calls."""

    PROTECTS = True

    def _own_all(self, links, n, starts):
        """GatedOracle.gsnr for the windows [s, s + n), s in starts, of the path with `links`: [len(starts)] GSNR in dB"""
        g, nw = self.gate, len(starts)
        span_off, svc_off, lengths, sb, sf, sse = [0], [0], [], [], [], []
        for l in links:
            ns = int(g["link_num_spans"][l])
            lengths += [float(g["link_span_length_km"][l])] * ns
            span_off.append(len(lengths))
            for e in self.shadow:   # provision order
                if l in e[1]:
                    sb.append(e[3]); sf.append(e[2]); sse.append(e[4])
            svc_off.append(len(sb))
        b = self._window(starts[0], n)[0]
        n_sp = len(lengths) * nw
        batch = dict(check_link_off=np.arange(nw + 1) * len(links), link_span_off=_tile(span_off, nw), link_svc_off=_tile(svc_off, nw),
                     bandwidth=[b] * nw, center_frequency=[self._window(s, n)[1] for s in starts],
                     launch_power=[g["launch_power_density_w_hz"] * b] * nw, span_length_km=np.tile(lengths, nw),
                     span_attenuation=np.full(n_sp, g["attenuation_normalized"]), span_noise_figure=np.full(n_sp, g["noise_figure"]),
                     svc_bandwidth=np.tile(np.array(sb, np.float64), nw), svc_center_frequency=np.tile(np.array(sf, np.float64), nw),
                     svc_se=np.tile(np.array(sse, np.int32), nw), svc_is_self=np.zeros(len(sb) * nw, np.uint8))
        return orc.gn_osnr(batch)

    def _neighbour_all(self, links, n, se, starts):
        """ProtectingOracle.neighbour_margin for the same windows: ([len(starts)] margins, NaN without a victim; victims)"""
        g, sh, nw = self.gate, self.shadow, len(starts)
        cset = set(links)
        victims = [i for i, e in enumerate(sh) if cset & e[1]] if self.PROTECTS else []
        if not victims:
            return np.full(nw, np.nan), 0
        by_link = {}
        for i, e in enumerate(sh):   # provision order
            for l in e[5]:
                by_link.setdefault(l, []).append(i)
        cb = self._window(starts[0], n)[0]
        span_off, svc_off, clo, lengths, sb, sf, sse, bw, fc, pw, cand = [0], [0], [0], [], [], [], [], [], [], [], []
        for v in victims:
            _, _, f_v, b_v, _, vlinks = sh[v]
            for l in vlinks:
                ns = int(g["link_num_spans"][l])
                lengths += [float(g["link_span_length_km"][l])] * ns
                span_off.append(len(lengths))
                for i in by_link[l]:
                    if i != v:
                        sb.append(sh[i][3]); sf.append(sh[i][2]); sse.append(sh[i][4])
                if l in cset:   # the candidate, the last interferer: its centre is the window's
                    cand.append(len(sb))
                    sb.append(cb); sf.append(0.0); sse.append(se)
                svc_off.append(len(sb))
            clo.append(len(span_off) - 1)
            bw.append(b_v); fc.append(f_v); pw.append(g["launch_power_density_w_hz"] * b_v)
        centres = np.tile(np.array(sf, np.float64), nw).reshape(nw, len(sf))
        centres[:, cand] = np.array([self._window(s, n)[1] for s in starts])[:, None]
        n_sp = len(lengths) * nw
        batch = dict(check_link_off=_tile(clo, nw), link_span_off=_tile(span_off, nw), link_svc_off=_tile(svc_off, nw),
                     bandwidth=np.tile(bw, nw), center_frequency=np.tile(fc, nw), launch_power=np.tile(pw, nw),
                     span_length_km=np.tile(lengths, nw), span_attenuation=np.full(n_sp, g["attenuation_normalized"]),
                     span_noise_figure=np.full(n_sp, g["noise_figure"]), svc_bandwidth=np.tile(np.array(sb, np.float64), nw),
                     svc_center_frequency=centres.ravel(), svc_se=np.tile(np.array(sse, np.int32), nw),
                     svc_is_self=np.zeros(len(sb) * nw, np.uint8))
        gs = orc.gn_osnr(batch).reshape(nw, len(victims))
        self.max_abs_gsnr = max(self.max_abs_gsnr, float(np.max(np.abs(gs))))
        thr = np.array([float(g["thresholds_db"][sh[v][4] - 1]) for v in victims])
        return np.min(gs - thr[None, :], axis=1), len(victims)

    def slots(self):
        """The pending request against what is lit now: window [K, S] bool, gsnr / margin [K, S] float64 (NaN as the entry writes
        them), affected [K, S] int32, mask [K, S] bool, w [K, S] float64 (NaN = not admitted), near [K, S] bool (the deciding
        margin lies inside MARGIN_DB), thr [K], best_slot [K] int32 (S = none), best_margin [K], first_free [K] int32 (S = none)."""
        o, K, S = self.o, self.K, self.S
        self._drop_due()
        window = np.zeros((K, S), bool)
        gsnr, margin = np.full((K, S), np.nan), np.full((K, S), np.nan)
        affected = np.zeros((K, S), np.int32)
        thr, n_slots = np.zeros(K), np.zeros(K, np.int32)
        for p in range(K):
            n = o.number_slots(p)
            links, se = self._path(p)
            thr[p], n_slots[p] = float(self.gate["thresholds_db"][se - 1]), n
            starts = [s for s in range(S - n + 1) if o.is_path_free(p, s, n)]
            if not starts:
                continue
            window[p, starts] = True
            gs = self._own_all(links, n, starts)
            gsnr[p, starts] = gs
            self.max_abs_gsnr = max(self.max_abs_gsnr, float(np.max(np.abs(gs))))
            self.any_closest = min(self.any_closest, float(np.min(np.abs(gs - thr[p]))))
            passed = [s for s, g1 in zip(starts, gs) if g1 >= thr[p]]
            if passed:
                mg, n_victims = self._neighbour_all(links, n, se, passed)
                margin[p, passed], affected[p, passed] = mg, n_victims
                if n_victims:
                    self.any_closest = min(self.any_closest, float(np.min(np.abs(mg))))
        own = gsnr - thr[:, None]
        with np.errstate(invalid="ignore"):
            mask = window & (own >= 0) & ~(margin < 0)
            near = window & ((np.abs(own) < MARGIN_DB) | (np.abs(margin) < MARGIN_DB))
        w = np.where(mask, np.fmin(own, margin), np.nan)
        best_slot, best_margin, first_free = np.full(K, S, np.int32), np.full(K, np.nan), np.full(K, S, np.int32)
        for p in range(K):
            if mask[p].any():
                best_slot[p] = int(np.nanargmax(w[p]))
                best_margin[p] = w[p, best_slot[p]]
            if window[p].any():
                first_free[p] = int(np.argmax(window[p]))
        return dict(window=window, gsnr=gsnr, margin=margin, affected=affected, mask=mask, w=w, near=near, thr=thr, n_slots=n_slots,
                    best_slot=best_slot, best_margin=best_margin, first_free=first_free, running=len(self.shadow))

    def window_by_window(self, rows):
        """rows of slots() against evaluate(p, s) for every window, bit for bit; returns the number of windows"""
        for p, s in np.argwhere(rows["window"]):
            g1, own, mg, aff = self.evaluate(int(p), int(s))
            assert g1 == rows["gsnr"][p, s] and aff == rows["affected"][p, s], (p, s)
            assert np.array_equal(mg, rows["margin"][p, s], equal_nan=True) and bool(own and not mg < 0) == bool(rows["mask"][p, s]), (p, s)
        return int(rows["window"].sum())


class GatedSlotsOracle(SlotsOracle):
    """... behind a gate that does not protect: the second check never runs"""

    PROTECTS = False

    def neighbour_margin(self, links, s, n, se):
        return np.nan, 0


def resolve(batch):
    """(name of the batch's case -- of gn_protect_reference.CASES, of gpu_support.MANY_PATHS or TRI --, its policy)"""
    name = batch.split(":")[-1]
    if name == TRI:
        return name, "sap_ff"
    if name in MANY_PATHS:
        return name, MANY_PATHS[name]["policy"]
    return name, pref.CASES[name]["policy"]


def batch_case(batch, tmp_path):
    """(topology, kwargs, policy) of a batch"""
    name, policy = resolve(batch)
    if name == TRI:
        return tri_topology(tmp_path), dict(TRI_KW), policy
    if name in MANY_PATHS:
        return many_paths_topology(name, tmp_path), many_paths_kwargs(name), policy
    return topology(pref.CASES[name]["topology"]), pref.case_kwargs(name), policy


@functools.lru_cache(maxsize=None)
def _run(key, seed, policy, warmup, n_steps, protect):
    topo, kw = key[0], dict(key[1])
    with device_log_in_oracle():
        go = (SlotsOracle if protect else GatedSlotsOracle)(topo, kw, pref.case_gate(topo, protect=protect), seed=seed)
        for _ in range(warmup):
            go.step(*go.propose(policy))
        cols, rows = {}, []
        for _ in range(n_steps):
            for k, v in go.slots().items():
                cols.setdefault(k, []).append(v)
            rows.append(go.step(*go.propose(policy)))
    tr = {"step_" + k: np.array([row[k] for row in rows]) for k in rows[0]}   # (the step has a gsnr and a margin of its own)
    tr.update({k: np.array(v) for k, v in cols.items()})
    fig = go.figures()
    go.close()
    for a in tr.values():
        a.setflags(write=False)
    return tr, fig


def cross_check(batch, tmp_path, steps):
    """The first environment of a batch stepped from its start, slots() held to evaluate() window by window at the given steps:
    the number of windows compared"""
    c = BATCHES[batch]
    topo, kw, policy = batch_case(batch, tmp_path)
    n = 0
    with device_log_in_oracle():
        go = (SlotsOracle if c["protect"] else GatedSlotsOracle)(topo, kw, pref.case_gate(topo, protect=c["protect"]), seed=SEEDS.get(batch, kw["seed"]))
        for t in range(max(steps) + 1):
            if t in steps:
                n += go.window_by_window(go.slots())
            go.step(*go.propose(policy))
        go.close()
    return n


def run_batch(batch, tmp_path):
    """The oracle runs of a batch, one per environment (seed of the case + 0 .. B - 1), once per process and shared: a list of
    (per-step arrays -- the step's as step_<name> and the rows of slots() taken BEFORE the step --, figures).  Read-only by agreement."""
    c = BATCHES[batch]
    topo, kw, policy = batch_case(batch, tmp_path)
    seed = SEEDS.get(batch, kw["seed"])
    return [_run(ref.cache_key((topo, kw)), seed + i, policy, c["warmup"], c["n"], c["protect"]) for i in range(c["B"])]


def counts(runs):
    """Summed over a batch: free windows, refused by their own check, refused by the neighbour check alone, admitted with no
    affected service, admitted behind a neighbour check, windows left out of the mask comparison (near), (path, step) rows with an
    admitted window, of those the rows whose best window is not the path's first free window and the rows whose two best differ
    by less than BEST_TOL_DB; the most running services, the margin closest to zero, the largest |GSNR|."""
    out = dict(windows=0, own_refused=0, neighbour_refused=0, admitted_unaffected=0, admitted_checked=0, near=0, rows=0,
               best_not_first=0, close_best=0)
    for tr, _ in runs:
        window, mask, margin, affected = tr["window"], tr["mask"], tr["margin"], tr["affected"]
        out["windows"] += int(window.sum())
        with np.errstate(invalid="ignore"):
            out["neighbour_refused"] += int((margin < 0).sum())
            out["own_refused"] += int((window & ~mask & ~(margin < 0)).sum())
        out["admitted_unaffected"] += int((mask & (affected == 0)).sum())
        out["admitted_checked"] += int((mask & (affected > 0)).sum())
        out["near"] += int(tr["near"].sum())
        has = tr["best_slot"] < window.shape[-1]
        out["rows"] += int(has.sum())
        out["best_not_first"] += int((has & (tr["best_slot"] != tr["first_free"])).sum())
        for t, p in zip(*np.nonzero(has)):
            w = np.sort(tr["w"][t, p][mask[t, p]])
            out["close_best"] += int(len(w) > 1 and w[-1] - w[-2] < BEST_TOL_DB)
    out["max_running"] = max(int(tr["running"].max()) for tr, _ in runs)
    out["closest"] = min(fig["any_closest"] for _, fig in runs)
    out["max_abs_gsnr"] = max(fig["max_abs_gsnr"] for _, fig in runs)
    return out
