"""The CPU reference of the max-margin policies (``include/orlg.h`` ``orlg_step_max_margin``): ``sap_mm``, ``any_mm`` and
``path_mm_external`` said on the rows of ``gn_slots_reference.SlotsOracle.slots()`` -- the mask, the worst margin ``w`` of every
admitted window, the best window and the first free start of every path.  Three uses:
  * ``proposal``: the rule itself, on the reference's rows or on the device's own query (the twin of ``test_gpu_gn_max_margin.py``);
  * ``follow``: a FOLLOWER.  Given the device's per-step ``(act_path, act_slot)`` it asks ``slots()`` before each step, holds the
    device's choice to the reference's rows with the tolerances of the helpers it builds on, then steps the oracle with the device's
    action: a near tie cannot make the two trajectories part.  With ``kept=`` it also hands back the oracle's own values of every step
    (reward, compactness, link averages, arrival and holding time, the blocking cause of a rejection) and ``final_state`` the oracle's
    at the end: the statistics of a max-margin launch are held to the oracle, not to the twin alone.
  * ``self_run``: every environment of a batch stepped with the reference's OWN max-margin choices, and what those steps exercise;
    ``own_run``: the same for the shapes of ``test_gpu_gn_max_margin_shapes.py`` (the tables at the end), step by step.
Helper module of ``test_gn_max_margin_args.py``, ``test_gpu_gn_max_margin.py`` and ``test_gpu_gn_max_margin_shapes.py``; nothing here
touches a GPU.
"""
import functools

import numpy as np

import block_cause_reference as bcr
import gn_gate_reference as ref
import gn_protect_reference as pref
import gn_slots_reference as sl
from gpu_support import device_log_in_oracle

MARGIN_DB, BEST_TOL_DB = sl.MARGIN_DB, sl.BEST_TOL_DB
ROUTES = {"sap_mm": "sap", "any_mm": "any", "path_mm_external": "path"}
MIN_COUNT = 10        # steps of each kind per counted batch
MAX_NEAR = 0.02       # steps of a batch whose decision may rest on a near value
# the batches long enough to hold MIN_COUNT steps of every kind (gn_slots_reference.COUNTED: 160 to 800 steps each; the other seven are
# there for a shape -- k = 32, two chunks of compacted services, a gate that does not protect, one / three / four / six words per link --
# and have 8 to 80 steps)
COUNTED = sl.COUNTED
# (batch, route) -> the first seed of the batch where it had to move off the case's own to meet a condition of
# test_gn_max_margin_args.py (found on the CPU, from the reference alone; route "path" keeps the case's own)
SEEDS = {
    ("nsfnet_s100_l20_spff", "sap"): 500,      # sap_mm behind sap_ff's path: 2 steps of 800 at the case's seed, 10 here (load 20: rare)
    ("jpn12_s320_l150_sapff", "any"): 163,     # fallbacks: 6 -> 10
    ("ring34_s320_l300_llpff", "sap"): 18,     # sap_mm behind sap_ff's path: 9 -> 18
    ("ring36_s512_l500_sapff", "sap"): 1884,   # near decisions 5 of 80 -> 1, behind sap_ff's path 6 -> 11, fallbacks 7 -> 14 (80 steps have
                                               # to hold ten of each kind: the first of 3 seeds in ~800 tried)
    ("ring36_s512_l500_sapff", "any"): 310,    # near decisions 5 of 80 -> 0, fallbacks 1 -> 11
}


def proposal(best_slot, best_margin, first_free, S, route, given=None):
    """(path, slot, w, kind) of one environment: best_slot / best_margin / first_free [K] as slots() or the query give them (S = none).
    kind: "admitted", "fallback" (w NaN: the step's check refuses it) or "rejection" ((K, S), w NaN)."""
    K = len(best_slot)
    scope = list(range(K)) if route != "path" else ([int(given)] if 0 <= int(given) < K else [])
    has = [p for p in scope if best_slot[p] < S]
    if has:
        p = has[0]
        if route == "any":
            for q in has[1:]:
                if best_margin[q] > best_margin[p]:   # strictly greater: ties go to the lowest index
                    p = q
        return p, int(best_slot[p]), float(best_margin[p]), "admitted"
    free = [p for p in scope if first_free[p] < S]
    if free:
        return free[0], int(first_free[free[0]]), float("nan"), "fallback"
    return K, S, float("nan"), "rejection"


def proposals(best_slot, best_margin, first_free, S, route, given=None):
    """proposal() for a batch: [B, K] rows -> (actions [B, 2] int32, w [B] float64, kinds)"""
    B = len(best_slot)
    got = [proposal(best_slot[i], best_margin[i], first_free[i], S, route, None if given is None else given[i]) for i in range(B)]
    return np.array([g[:2] for g in got], np.int32).reshape(B, 2), np.array([g[2] for g in got], np.float64), [g[3] for g in got]


def first_free_of(window):
    """[..., K] the lowest free start of every path from a [..., K, S] bool window matrix, S = none"""
    S = window.shape[-1]
    return np.where(window.any(axis=-1), np.argmax(window, axis=-1), S).astype(np.int32)


def check_choice(rows, route, p, s, given=None):
    """The device's (p, s) for the pending request against the reference's rows of slots(): raises AssertionError, returns the kind."""
    K, S = rows["window"].shape
    mask, near, w, window = rows["mask"], rows["near"], rows["w"], rows["window"]
    sure = mask & ~near   # windows the reference admits beyond doubt
    scope = list(range(K)) if route != "path" else ([int(given)] if 0 <= int(given) < K else [])
    if p == K:
        assert s == S and not any(window[q].any() for q in scope), ("rejection although a window is free", scope)
        return "rejection"
    assert p in scope and 0 <= s < S and window[p, s], ("not a free window in scope", p, s)
    if not (mask[p, s] or near[p, s]):
        # a fallback: no window in scope is surely admitted, and it is the first free start of the first path in scope with a window
        assert not any(sure[q].any() for q in scope), ("fallback although a window is admitted", p, s)
        first = [q for q in scope if window[q].any()][0]
        assert p == first and s == int(np.argmax(window[p])), ("fallback is not the first free start", p, s, first)
        return "fallback"
    # (a near window that the device refused shows as a refusal in the step: accepted is compared there)
    with np.errstate(invalid="ignore"):
        if mask[p].any():
            top = np.nanmax(w[p])
            assert near[p, s] or w[p, s] >= top - BEST_TOL_DB, ("not the path's best window", p, s, w[p, s], top)
    if route == "sap":
        assert not any(sure[q].any() for q in range(p)), ("an earlier path has an admitted window", p)
    if route == "any" and mask.any() and mask[p, s]:
        assert w[p, s] >= np.nanmax(w) - BEST_TOL_DB, ("not the best window of all paths", p, s, w[p, s], float(np.nanmax(w)))
    return "admitted" if mask[p, s] else "near"


class _Keeping:
    """The oracle environment of a follower with what every step met and returned kept in `last`: the oracle's own reward,
    compactness and link averages, the request's arrival and holding time, and the fit levels of the candidate paths on the state the
    step met (block_cause_reference.path_levels: the blocking cause of a rejection is 1 + their maximum)."""

    def __init__(self, o, topo):
        self._o, self._topo, self.last = o, topo, None

    def __getattr__(self, name):
        return getattr(self._o, name)

    def step(self, p, s):
        r = self._o.request()
        levels = bcr.path_levels(self._o.available_slots(), self._topo, r.src, r.dst, r.bit_rate)
        res = self._o.step(p, s)
        self.last = dict(reward=res.reward, done=int(res.done), network_compactness=res.network_compactness,
                         network_compactness_difference=res.network_compactness_difference, avg_link_compactness=res.avg_link_compactness,
                         avg_link_utilization=res.avg_link_utilization, arrival=r.arrival_time, holding=r.holding_time,
                         rejection_cause=1 + int(np.max(levels)))
        return res


def most_sharing(go):
    """the most running services (the due ones dropped) that share a link with one candidate path of the pending request: the entries
    the kernel compacts for that path"""
    return max(sum(1 for e in go.shadow if e[1] & set(go._path(p)[0])) for p in range(go.K))


def follow(go, dev, i, route, diffs, given=None, kept=None):
    """Environment i of the device's outputs (act_path, act_slot, accepted, gn_gsnr_db, gn_neighbour_margin_db, request: [n, B(, 4)])
    followed on the oracle `go`, which stands where the device's handle stood before the launch.  Returns the kinds' counts; the
    absolute differences of the margins (neighbour and window) are appended to `diffs`: their bound, 1e-9 x the largest |GSNR| the
    reference computed in the batch, is known when the batch is done.  kept: a list that gets one dict per step -- the oracle's own
    values of the step (_Keeping), its kind, accepted, gsnr and margin, the rows of slots() the step met, running / sharing: the services
    in progress when the request is served and the most of them that share a link with one candidate path, and pops: the services
    released so far."""
    n = dev["act_path"].shape[0]
    kinds = dict(admitted=0, near=0, fallback=0, rejection=0)
    if kept is not None and not isinstance(go.o, _Keeping):
        go.o = _Keeping(go.o, go.topo)
    for t in range(n):
        rows = go.slots()
        p, s = int(dev["act_path"][t, i]), int(dev["act_slot"][t, i])
        r = go.o.request()
        assert tuple(int(v) for v in dev["request"][t, i]) == (r.service_id, r.src, r.dst, r.bit_rate), ("request", t, i)
        kind = check_choice(rows, route, p, s, None if given is None else given[t, i])
        kinds[kind] += 1
        pops = int(go.o.counters()["services_accepted"]) - int(rows["running"])   # releases so far: the ring's head is pops % Q
        sharing = most_sharing(go) if kept is not None else 0
        out = go.step(p, s)
        what = (t, i, p, s, kind)
        if kept is not None:
            kept.append(dict(go.o.last, kind=kind, accepted=int(out["accepted"]), gsnr=out["gsnr"], margin=out.get("margin", np.nan),
                             running=int(rows["running"]), sharing=sharing, pops=pops, rows=rows))
        if kind != "near":
            assert bool(dev["accepted"][t, i]) == bool(out["accepted"]), what
        g, m = dev["gn_gsnr_db"][t, i], dev["gn_neighbour_margin_db"][t, i]
        assert np.isnan(g) == np.isnan(out["gsnr"]) and (np.isnan(g) or np.isclose(g, out["gsnr"], rtol=1e-9, atol=0)), what + (g, out["gsnr"])
        want_m = out.get("margin", np.nan)
        assert np.isnan(m) == np.isnan(want_m), what + (m, want_m)
        if not np.isnan(m):
            diffs.append(abs(m - want_m))
        if kind == "near" and bool(dev["accepted"][t, i]) != bool(out["accepted"]):
            raise AssertionError(("a near window was decided differently: the trajectories part", what))
        if "gn_window_margin_db" in dev:
            wm = dev["gn_window_margin_db"][t, i]
            if kind in ("fallback", "rejection"):
                assert np.isnan(wm), what
            elif rows["mask"][p, s]:
                diffs.append(abs(wm - rows["w"][p, s]))
    return kinds


def batch_seed(batch, route, kw):
    """the seed of environment 0 of a batch under a route: the case's own unless SEEDS moved it"""
    return SEEDS.get((batch, route), sl.SEEDS.get(batch, kw["seed"]))


def oracle_at(batch, tmp_path, i, route, warm_policy=None):
    """The oracle of environment i of a batch after the batch's warm-up steps of its case's policy (the caller closes it)"""
    c = sl.BATCHES[batch]
    topo, kw, policy = sl.batch_case(batch, tmp_path)
    seed = batch_seed(batch, route, kw) + i
    return warm_oracle(topo, kw, seed, warm_policy or policy, c["warmup"], c["protect"])


def warm_oracle(topo, kw, seed, policy, warmup, protect=True, **oracle_kw):
    """A slots oracle on `seed` after `warmup` steps of `policy` (the caller closes it; oracle_kw: j, reward_mode)"""
    go = (sl.SlotsOracle if protect else sl.GatedSlotsOracle)(topo, kw, pref.case_gate(topo, protect=protect), seed=seed, **oracle_kw)
    for _ in range(warmup):
        go.step(*go.propose(policy))
    return go


def final_state(go):
    """what the oracle holds at the end of a followed launch: occupancy, counters, clock, services in progress, the link and graph
    statistics, the histograms, the pending request, and the release times of the running services in rank order"""
    o, r = go.o, go.o.request()
    go._drop_due()
    return dict(available_slots=o.available_slots(), counters=o.counters(), num_running=o.num_running(), current_time=o.current_time(),
                link_stats=o.link_stats(), graph_stats=o.graph_stats(), bit_rate_hist=o.bit_rate_hist(),
                request=(r.service_id, r.src, r.dst, r.bit_rate, r.arrival_time, r.holding_time),
                releases=sorted(e[0] for e in go.shadow))


# ---------------------------------------------------------------------------------------- the reference on its own choices
@functools.lru_cache(maxsize=None)
def _self_run(key, seed, policy, warmup, n_steps, protect, route):
    topo, kw = key[0], dict(key[1])
    c = dict(steps=0, near=0, best_not_first=0, later_path=0, fallback=0, rejection=0, neighbour_decided=0, accepted=0, high_path=0,
             max_running=0)
    with device_log_in_oracle():
        go = (sl.SlotsOracle if protect else sl.GatedSlotsOracle)(topo, kw, pref.case_gate(topo, protect=protect), seed=seed)
        for _ in range(warmup):
            go.step(*go.propose(policy))
        K, S = go.K, go.S
        for _ in range(n_steps):
            rows = go.slots()
            given = 0   # (route "path" is exercised on the device with the twin; here the routes that choose)
            p, s, w, kind = proposal(rows["best_slot"], rows["best_margin"], rows["first_free"], S, route, given)
            c["steps"] += 1
            c["high_path"] += int(kind != "rejection" and p >= 8)   # a proposal on a path the kernel lays out W lanes apart
            c["max_running"] = max(c["max_running"], int(rows["running"]))
            if kind != "admitted":
                c[kind] += 1
            # a decision that rests on a near value
            near = False
            if kind == "admitted":
                ws = np.sort(rows["w"][p][rows["mask"][p]])
                # (two windows with the same w to the bit are no near tie: both sides take the lower one)
                near |= bool(abs(w) < MARGIN_DB) or bool(len(ws) > 1 and 0 < ws[-1] - ws[-2] < BEST_TOL_DB)
                near |= bool(rows["near"][:p].any()) if route == "sap" else False   # a deciding earlier-path window
                if route == "any":
                    tops = np.sort(rows["best_margin"][np.isfinite(rows["best_margin"])])
                    near |= bool(len(tops) > 1 and 0 < tops[-1] - tops[-2] < BEST_TOL_DB)
                c["best_not_first"] += int(s != rows["first_free"][p])
                ff = go.propose("sap_ff")
                c["later_path"] += int(route == "sap" and ff[0] < K and p > ff[0])
                own = rows["gsnr"][p, s] - rows["thr"][p]
                c["neighbour_decided"] += int(np.isfinite(rows["margin"][p, s]) and rows["margin"][p, s] < own)
            elif kind == "fallback":
                near |= bool(rows["near"].any())
            c["near"] += int(near)
            c["accepted"] += go.step(p, s)["accepted"]
        go.close()
    return c


def self_run(batch, route, tmp_path):
    """The counts of a batch stepped by the reference's own choices under `route` ("sap" or "any"), summed over its environments"""
    c = sl.BATCHES[batch]
    topo, kw, policy = sl.batch_case(batch, tmp_path)
    seed = batch_seed(batch, route, kw)
    out = {}
    for i in range(c["B"]):
        for k, v in _self_run(ref.cache_key((topo, kw)), seed + i, policy, c["warmup"], c["n"], c["protect"], route).items():
            out[k] = max(out.get(k, 0), v) if k.startswith("max_") else out.get(k, 0) + v
    return out


# ---------------------------------------------------------------------------------------- the shapes of test_gpu_gn_max_margin_shapes.py
SHAPE_B, SHAPE_N = 2, 40   # environments and steps of a word-count case: the first of its batch, after the batch's own warm-up
# words per link -> the batch of gn_slots_reference.BATCHES that stands for it: all six instantiations of orlg_rmsa_mm_kernel<W, ., .>
WORD_CASES = {1: "g3x3_k9_s64", 2: "nsfnet_s100_l20_spff", 3: "g4x4_k21_s192", 4: "g4x4_k16_s200", 5: "jpn12_s320_l150_sapff",
              6: "g3x4_k10_s384", 8: "ring36_s512_l500_sapff"}
# more than 128 services in the ring and on one path: TRI at twice its load, a ring of 256, the three routes in turn on one state (one
# environment and two steps per route: a slots() of the reference walks 400 windows x 150 victims on each of two paths at this load)
CHUNKS = dict(load=600, warmup=260, policy="sap_ff", queue_capacity=256, B=1, plan=(("sap", 2), ("any", 2), ("path", 2)))
# a ring whose head laps: the smallest ring (64 slots), a launch in which every environment releases at least 2 Q services
LAP = dict(batch="nsfnet_s100_l20_spff", queue_capacity=64, B=2, n=300)
# a DeepRMSA handle: j = 2 blocks per path, reward +1 / -1
DEEP = dict(S=100, load=20, seed=13, j=2, B=2, n=60)
# the launch of fewer waves per workgroup: NSFNET with 320 slots and a ring of 1024 -- 8 waves per workgroup for the handle, 6 for the
# max-margin kernel (tests/test_wave_plan.py GEOMETRY) --, 14 environments: three workgroups, the last with two
FEWER = dict(case="nsfnet_s320_l50_sapff", queue_capacity=1024, B=14, warmup=40, n=20)
# a shape the library accepts whose single wave does not fit with up16(4 Q) behind it: a 5 x 5 grid of gpu_support.grid_edges with 20
# paths per pair (12 000 path records: 105 664 bytes of tables) and the largest ring -- 161 744 bytes for the handle's one wave, 178 128
# for the max-margin kernel's.  With 16 paths per pair, or a ring of 2048, the wave fits
REFUSED = dict(rows=5, cols=5, k=20, S=100, load=40, queue_capacity=4096, fits=2048)


def deep_kwargs():
    c = DEEP
    return dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=25.0, episode_length=1000, seed=c["seed"])


def chunks_kwargs():
    return dict(sl.TRI_KW, load=CHUNKS["load"])


@functools.lru_cache(maxsize=None)
def _own_run(key, seed, policy, warmup, plan, protect):
    topo, kw = key[0], dict(key[1])
    steps = []
    with device_log_in_oracle():
        go = warm_oracle(topo, kw, seed, policy, warmup, protect)
        for route, n in plan:
            for _ in range(n):
                rows = go.slots()
                p, s, _, kind = proposal(rows["best_slot"], rows["best_margin"], rows["first_free"], go.S, route, len(steps) % go.K)
                pops = int(go.o.counters()["services_accepted"]) - int(rows["running"])
                steps.append((kind, p, int(rows["running"]), most_sharing(go), pops))
                go.step(p, s)
        go.close()
    return tuple(steps)


def own_run(topo, kw, seed, policy, warmup, plan, protect=True):
    """One environment stepped by the reference's own max-margin choices through `plan` ((route, steps), ...; route "path" is given the
    path step % K): per evaluated step (kind, path, services in progress, most of them sharing a link with one path, releases so far).
    Run once per process and shared."""
    return _own_run(ref.cache_key((topo, kw)), seed, policy, warmup, tuple(plan), protect)


def word_case_run(W, i, tmp_path):
    """own_run of environment i of the word-count case W under sap_mm"""
    batch = WORD_CASES[W]
    topo, kw, policy = sl.batch_case(batch, tmp_path)
    return own_run(topo, kw, batch_seed(batch, "sap", kw) + i, policy, sl.BATCHES[batch]["warmup"], (("sap", SHAPE_N),), sl.BATCHES[batch]["protect"])


def chunks_run(i, tmp_path):
    c, kw = CHUNKS, chunks_kwargs()
    return own_run(sl.tri_topology(tmp_path), kw, kw["seed"] + i, c["policy"], c["warmup"], c["plan"])


def lap_run(i, tmp_path):
    c = LAP
    topo, kw, policy = sl.batch_case(c["batch"], tmp_path)
    return own_run(topo, kw, batch_seed(c["batch"], "sap", kw) + i, policy, 0, (("sap", c["n"]),))
