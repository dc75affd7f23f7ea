"""The QoT-aware environment at one to four occupancy words per link: the channel counts, loads and step counts that
tests/test_oracle_phy_words.py (CPU) and tests/test_gpu_phy_words.py share, the QoT tables cut to their first C columns, the
oracle's run of one environment (computed once per process, read-only by agreement) and the saturation conditions every test
asserts on it, so that no test passes by never reaching the code it is about.  Imports neither the library nor a GPU."""
import functools

import numpy as np

from conftest import load_phy_tables, load_topology, phy_oracle_from_kwargs

TOPOLOGY, TABLES = "us14_3-paths_6-modulations", "us14_k3"
# C -> ((number_spectrum_channels, number_spectrum_channels_s_band), words per link, load, steps, steps with defragmentation).
# Loads and step counts chosen on the oracle alone (CPU), all seeds the tests use: within the steps every environment blocks
# at least 20 requests and accepts at least 30 %, an accepted physical-layer service lights channel C - 1, and the policies
# that use the virtual layer accept on it; with the defragmentation every environment moves services, grooms where grooming
# is on and runs more than 10 cycles (C = 3 needs 2400 steps at load 50 for a grooming move in every environment; at load 100
# it accepts less than 30 %).  First blocked request at step / peak of services in progress, plain / with defragmentation:
#   C = 3: 3..16 / 30 / 34          C = 64, 65: 168..412 / 584 / 959      C = 128, 129: 410..887 / 1102 / 1331
#   C = 192, 193: 645..1311 / 1510 / 1703                                  C = 256: 746..1678 / 1802 / 1996
# (per case: DESIGN.md section 4, "The QoT-aware kernel at one to four words").
WORD_COUNTS = {
    3: ((1, 1), 1, 50, 300, 2400),
    64: ((10, 44), 1, 6000, 800, 2400),
    65: ((10, 45), 2, 6000, 800, 2400),
    128: ((20, 88), 2, 16000, 1300, 2000),
    129: ((20, 89), 3, 16000, 1300, 2000),
    192: ((40, 112), 3, 24000, 1700, 2200),
    193: ((40, 113), 4, 24000, 1700, 2200),
    256: ((80, 96), 4, 32000, 2000, 2400),
}
CHANNEL_COUNTS = tuple(WORD_COUNTS)
POLICIES = ("bmfa", "bmfa_rss", "sapff", "bmff", "sapbm", "faff", "faff_rss")
BATCH = 3   # environments per case, seeds s, s + 1, s + 2
COMMON = dict(mean_service_holding_time=25, episode_length=150)
CS_CAPACITY = 64   # entries per channel_state list: the library's maximum (ORLG_CS_MAX)


def words_of(num_channels):
    return WORD_COUNTS[num_channels][1]


@functools.lru_cache(maxsize=None)
def topology():
    return load_topology(TOPOLOGY)


@functools.lru_cache(maxsize=None)
def cut_tables(num_channels):
    """The shipped US14 tables cut to their first C columns (pairs, modulation_level, gsnr)."""
    pairs, mod, gsnr = load_phy_tables(TABLES)
    return pairs, np.ascontiguousarray(mod[:, :num_channels]), np.ascontiguousarray(gsnr[:, :num_channels])


def words_kwargs(num_channels, seed, policy, defrag=None, load=None, **over):
    """Reference-style keyword arguments of one case: grooming on for bmfa / bmfa_rss, defrag: None, "cut" or "rss"."""
    split, words, ld, _, _ = WORD_COUNTS[num_channels]
    assert 2 * split[0] + split[1] == num_channels and -(-num_channels // 64) == words
    kw = dict(COMMON, load=ld if load is None else load, seed=seed, grooming=policy in ("bmfa", "bmfa_rss"),
              number_spectrum_channels=split[0], number_spectrum_channels_s_band=split[1])
    if defrag:
        kw.update(defrag_period=7, number_moves=6, metric=defrag)
    kw.update(over)
    return kw


def _freeze(v):
    if isinstance(v, dict):
        return tuple(sorted((k, _freeze(x)) for k, x in v.items()))
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    return v


class OracleRun:
    """One environment's run on the oracle: the traces per launch, their concatenation and the state after the last step."""

    def __init__(self, num_channels, kw, policy, launches):
        o = phy_oracle_from_kwargs(topology(), cut_tables(num_channels), kw)
        self.parts = [o.run(policy, n, reset_on_done=True) for n in launches]
        self.tr = {f: np.concatenate([p[f] for p in self.parts]) for f in self.parts[0]}
        self.counters, self.current_time, self.num_running = o.counters(), o.current_time(), o.num_running()
        self.available_channels, self.channel_state = o.available_channels(), o.channel_state()
        o.close()


_runs = {}


def oracle_run(num_channels, kw, policy, launches, log_tag):
    """OracleRun of (C, kwargs with the environment's seed, policy, launches), once per process.  log_tag: which logarithm the
    oracle runs on ("libm" or "device"): part of the key, the caller switches it (gpu_support.device_log_in_oracle)."""
    key = (num_channels, _freeze(kw), policy, tuple(launches), log_tag)
    if key not in _runs:
        _runs[key] = OracleRun(num_channels, kw, policy, tuple(launches))
    return _runs[key]


def saturation(run, num_channels, policy, grooming, min_blocked=20):
    """The conditions every test asserts on the oracle's own outputs of one environment; returns the figures."""
    tr = run.tr
    acc = tr["accepted"] == 1
    phys = acc & (tr["act_path"] >= 0) & (tr["act_path"] < 10)
    virt = acc & (tr["act_path"] >= 20)
    blocked = int((~acc).sum())
    top = int(tr["channels"][phys].max()) if phys.any() else -1
    fig = dict(blocked=blocked, accepted=float(acc.mean()), top=top, virtual=int(virt.sum()),
               peak_running=int(tr["n_running"].max()), first_blocked=int(np.argmax(~acc)) if blocked else -1)
    assert blocked >= min_blocked, fig
    assert fig["accepted"] >= 0.3, fig
    assert top == num_channels - 1, fig
    if grooming or policy not in ("bmfa", "bmfa_rss"):   # the policies that use the virtual layer
        assert fig["virtual"] >= 1, fig
    return fig


def capacities(runs, defrag):
    """Explicit capacities of a parity handle from the oracle's peaks: the release queue takes the peak of services in progress
    plus 64, rounded up to 64 slots; the defragmentation work list (one entry per channel in use that a service fills, at most
    six per service at 600 Gb/s on level 1, 1.4 on average) four entries per queue slot; the channel_state lists the library's
    maximum, which the oracle's longest list at the end of the run must leave a quarter of unused."""
    peak = max(int(r.tr["n_running"].max()) for r in runs)
    q = -(-(peak + 64) // 64) * 64
    longest = max([len(v) for r in runs for v in r.channel_state.values()] or [0])
    assert longest <= CS_CAPACITY * 3 // 4, longest
    kw = dict(queue_capacity=q, channel_state_capacity=CS_CAPACITY)
    if defrag:
        kw["defrag_capacity"] = 4 * q
    return kw
