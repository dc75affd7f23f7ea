"""The cases of ``test_gpu_policy_prefilter.py`` and what ``test_policy_prefilter.py`` pins about them on the CPU (DESIGN 2.5, round
16): the group kernel's first-fit passes after the first look only at the paths whose links all have a free run of n slots, and
a pass without such a path is left out.  Support module: the shapes, their handles' keyword arguments, and the oracle's traces
classified with ``tools/exp_policy_prefilter.py``.  Nothing here touches a GPU or the library's kernels."""
import os
import sys

from conftest import ROOT
from gpu_support import MANY_PATHS, device_log_in_oracle, many_paths_kwargs, many_paths_topology, topology, write_topology

sys.path.insert(0, os.path.join(ROOT, "tools"))
import exp_policy_prefilter as exp   # noqa: E402

NSFNET = "nsfnet_chen_5-paths_6-modulations"
JPN12 = "jpn12_5-paths_6-modulations"
US14 = "us14_3-paths_6-modulations"
SEED0 = 10
PIN_ENVS = 8   # the environments whose traces the CPU file classifies (the GPU cases hold all B to the oracle)

# name -> topo: a golden topology, a MANY_PATHS grid ("grid:<name>") or "ring"; S slots, load; B environments and steps of the GPU
# case; passes: first-fit passes of the shape, ceil(K / (16 // W)).  Loads and seeds chosen on the CPU so that the oracle's traces
# of the first PIN_ENVS environments hold what test_policy_prefilter.py asks for
CASES = {
    "nsf320_load50": dict(topo=NSFNET, S=320, load=50, B=16, steps=400, passes=2),
    "nsf320_load150": dict(topo=NSFNET, S=320, load=150, B=16, steps=400, passes=2),
    "nsf512_three_passes": dict(topo=NSFNET, S=512, load=85, B=16, steps=400, passes=3),
    "nsf128_one_pass": dict(topo=NSFNET, S=128, load=25, B=16, steps=300, passes=1),
    "grid_k21_s192": dict(topo="grid:g4x4_k21_s192", S=192, load=70, B=16, steps=400, passes=5),
    "grid_k12_s320": dict(topo="grid:g4x4_k12_s320", S=320, load=116, B=16, steps=400, passes=4),
    "ring_k8_s320": dict(topo="ring", S=320, load=240, B=16, steps=400, passes=3),
    "jpn12_k5": dict(topo=JPN12, S=320, load=50, B=16, steps=400, passes=2),
    "us14_k3": dict(topo=US14, S=320, load=50, B=16, steps=300, passes=1),
}

# Fifteen nodes on a ring and six chords that all end in node 15: the eight simple paths from node 1 to node 15 have 5, 1, 14, 9,
# 4, 13, 8 and 12 hops in the order of their lengths (the shape test_gpu_policy_pass.py builds for the hop groups), so with W = 5 a
# lane tests hops w, w + 5 and w + 10, and a path shorter than W shares a pass with one of 14 hops
RING_N, RING_K = 15, 8
RING_CHORDS = ((13, 60), (4, 140), (5, 60), (8, 120), (9, 80), (12, 90))
RING_HOPS = [5, 1, 14, 9, 4, 13, 8, 12]
_ring = {}


def ring_topology(tmp_path):
    if not _ring:
        from optical_rl_gym_amd.topology_io import topology_from_txt
        edges = [(j, 15, length) for j, length in RING_CHORDS] + [(i, i + 1, 10) for i in range(1, 14)] + [(14, 15, 20), (15, 1, 110)]
        _ring["topo"] = topology_from_txt(write_topology(tmp_path, "ring15_prefilter", RING_N, edges), "ring15_prefilter", k_paths=RING_K)
    return _ring["topo"]


def case_topology(name, tmp_path):
    t = CASES[name]["topo"]
    if t == "ring":
        return ring_topology(tmp_path)
    if t.startswith("grid:"):
        return many_paths_topology(t[5:], tmp_path)
    return topology(t)


def case_kwargs(name):
    c = CASES[name]
    if c["topo"] == "ring":
        probs = [0.3] + [0.4 / 13] * 13 + [0.3]
        return dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=25, episode_length=150, seed=SEED0,
                    node_request_probabilities=probs)
    if c["topo"].startswith("grid:"):
        assert MANY_PATHS[c["topo"][5:]]["S"] == c["S"]
        return many_paths_kwargs(c["topo"][5:], load=c["load"], episode_length=150, seed=SEED0)
    return dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=25, episode_length=150, seed=SEED0)


def classify(traces, W):
    """What the later passes are to the rows of these traces ((n, ml, start) [steps, K] per environment): the number of steps
    with a later pass ruled out / kept with a window found / kept without one; steps whose middle pass is ruled out and whose
    last pass finds the window; later-pass paths kept by ml == n and dropped by ml == n - 1; paths with a fit that fail the test."""
    PP = 16 // W
    out = dict(ruled_out=0, kept_found=0, kept_none=0, middle_out_last_found=0, kept_by_ml_eq_n=0, dropped_by_ml_eq_n_minus_1=0,
               fit_fails_test=0, later_passes=0)
    for n_all, ml_all, start_all in traces:
        K = n_all.shape[1]
        n_pass = -(-K // PP)
        for n, ml, start in zip(n_all, ml_all, start_all):
            out["fit_fails_test"] += int(((start >= 0) & (ml < n)).sum())
            cls, found_in = exp.row_passes(n, ml, start, PP)
            out["later_passes"] += len(cls)
            out["ruled_out"] += exp.RULED_OUT in cls
            out["kept_found"] += exp.KEPT_FOUND in cls
            out["kept_none"] += exp.KEPT_NONE in cls
            out["middle_out_last_found"] += n_pass >= 3 and found_in == n_pass - 1 and exp.RULED_OUT in cls[:-1]
            reached = slice(PP, min((len(cls) + 1) * PP, K))
            out["kept_by_ml_eq_n"] += int((ml[reached] == n[reached]).sum())
            out["dropped_by_ml_eq_n_minus_1"] += int((ml[reached] == n[reached] - 1).sum())
    return out


def skip_then_find(traces, W):
    """Quad-steps (environments 4q .. 4q + 3 in lockstep, as the kernel steps them) in which a later pass is SKIPPED -- no row that
    still looks has a candidate in it -- and a pass after it runs and finds a window for some row: what `break` in the place of
    `continue` would lose.  The kernel's skip is a vote of the whole quad, so this is counted per quad, not per row."""
    PP = 16 // W
    count = 0
    for q0 in range(0, len(traces) - len(traces) % 4, 4):
        for t in range(traces[q0][0].shape[0]):
            info = [exp.row_passes(*(a[t] for a in traces[q0 + i]), PP) for i in range(4)]
            n_pass = -(-traces[q0][0].shape[1] // PP)
            last = [f if f >= 0 else n_pass - 1 for _, f in info]
            skipped = False
            for j in range(1, max(last) + 1):
                runs = any(j <= l and cls[j - 1] != exp.RULED_OUT for (cls, _), l in zip(info, last))
                if not runs:
                    skipped = True
                elif skipped and any(f == j for _, f in info):
                    count += 1
                    break
    return count


_pins = {}


def case_pins(name, tmp_path):
    """(classify() of the first PIN_ENVS environments of the case, on the logarithm the device uses; their traces) -- once per process"""
    if name not in _pins:
        c, topo, kw = CASES[name], case_topology(name, tmp_path), case_kwargs(name)
        with device_log_in_oracle():
            traces = [exp.oracle_trace(topo, kw, kw["seed"] + i, c["steps"]) for i in range(PIN_ENVS)]
        pins = classify(traces, exp.words_per_link(c["S"]))
        pins["skip_then_find"] = skip_then_find(traces, exp.words_per_link(c["S"]))
        _pins[name] = (pins, traces)
    return _pins[name]
