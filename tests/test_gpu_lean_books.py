"""The lean body keeps two of the step's books on the lanes (csrc/orlg_group_body.h, LANE_HIST and LANE_SUMS): the bit-rate
histograms and the eight counters follow from per-lane counts that are flushed at an episode's end, at a ticket's end and every
32 768 steps of a ticket; ``sum_span`` and ``sum_gaps`` are lane partials joined where they are read.  The full body
(``ORLG_NO_LEAN``) keeps them as it always did: every case holds ``counters()``, ``bit_rate_hist()``, ``graph_stats()``,
``link_stats()`` and ``save_state()`` byte for byte between the two bodies, and one case per shape against the C oracle on the
device's logarithm.  What the shapes reach is asserted on the oracle alone in tests/test_lean_books_args.py."""
import functools

import numpy as np
import pytest

from gpu_support import (RMSA_OUTS as OUTS, against_oracle, device_log_in_oracle, drive, kernel_name, oracle_env_from_kwargs, rmsa_env,
                         same_bytes, snapshot, tooling_env, topology)
from lean_books_cases import B, BOUNDARY_LAUNCHES, CHUNKS, LAUNCHES, LEAN_MAX_RATES, NSF, RATE_COUNTS, RING34, SEED, kwargs, rates

pytestmark = pytest.mark.gpu

NO_LEAN, FORCED = {"ORLG_NO_LEAN": "1"}, {"ORLG_GROUP_CHUNKS": str(CHUNKS)}


def bodies(run):
    return [s.split("body=")[1].split()[0] if "body=" in s else None for s in run["said"]]


def both(make, launches, env_vars=None, lean="lean"):
    """the launches on the body a handle takes by itself (`lean` says which that is) and on the full body"""
    extra = env_vars or {}
    a = drive(make, launches, (), policy="sap_ff", env_vars=extra)
    b = drive(make, launches, (), policy="sap_ff", env_vars=dict(extra, **NO_LEAN))
    assert bodies(a) == [lean] * len(launches) and bodies(b) == ["full"] * len(launches), (a["said"], b["said"])
    assert {k.split("<")[0] for k in a["kernels"] + b["kernels"]} == {"orlg_rmsa_group_kernel"}, a["said"]
    if extra:   # (a launch of 16 steps strides over its quads: no tickets, so no chunks)
        assert all(f"chunks={CHUNKS}" in s for s, n in zip(a["said"], launches) if n > 16), a["said"]
    return a, b


@functools.lru_cache(maxsize=None)
def runs(name, S, batch, launches, chunks, n_rates=0):
    kw = kwargs(S=S, **({"bit_rates": rates(n_rates)} if n_rates else {}))
    return both(lambda: rmsa_env(name, batch, "group", stats_level="full", **kw), launches, FORCED if chunks else None,
                "full" if n_rates > LEAN_MAX_RATES else "lean")


@functools.lru_cache(maxsize=None)
def oracle_books(name, kw_items, launches):
    """counters and histograms of one environment on the oracle"""
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topology(name), dict(kw_items))
        for n in launches:
            o.run("sap_ff", n, reset_on_done=True, fields=[])
    got = dict(counters=o.counters(), hist=o.bit_rate_hist())
    o.close()
    return got


def books_match_oracle(name, kw, run, launches, envs):
    """the state as gpu_support.against_oracle compares it, and the four histograms"""
    against_oracle(name, kw, run, "sap_ff", launches, envs, "full", fields=())
    for i in envs:
        want = oracle_books(name, tuple(sorted(dict(kw, seed=kw["seed"] + i).items())), tuple(launches))
        for k, v in want["hist"].items():
            assert np.array_equal(run["snap"]["bit_rate_hist." + k][i], v), (i, k)
        for k, v in want["counters"].items():
            assert run["snap"]["counters." + k][i] == v, (i, k)


# ---------------------------------------------------------------------------------------- the base case
@pytest.mark.parametrize("chunks", [False, True], ids=["tickets", "chunks7"])
def test_lean_books_equal_full_body(chunks):
    lean, full = runs(NSF, 320, B, LAUNCHES, chunks)
    same_bytes(lean["snap"], full["snap"], ("lean", "full", chunks))
    c = lean["snap"]
    assert (c["counters.services_processed"] == sum(LAUNCHES) + 1).all() and (c["episodes_done"] >= 30).all(), c["episodes_done"]
    assert (c["bit_rate_hist.requested"].sum(axis=1) == sum(LAUNCHES) + 1).all()
    if not chunks:
        books_match_oracle(NSF, kwargs(), lean, LAUNCHES, (0, 3, B - 1))


def test_chunks_leave_the_same_state():
    same_bytes(runs(NSF, 320, B, LAUNCHES, False)[0]["snap"], runs(NSF, 320, B, LAUNCHES, True)[0]["snap"], "chunks")


def test_episode_ends_on_a_chunks_last_step():
    """The flush of the episode's end is the chunk's last act before the ticket-end flush; the next chunk starts from the record."""
    lean, full = runs(NSF, 320, B, BOUNDARY_LAUNCHES, True)
    same_bytes(lean["snap"], full["snap"], "boundary")
    same_bytes(lean["snap"], runs(NSF, 320, B, BOUNDARY_LAUNCHES, False)[0]["snap"], "boundary, chunks or not")
    books_match_oracle(NSF, kwargs(), lean, BOUNDARY_LAUNCHES, (1, B - 1))


# ---------------------------------------------------------------------------------------- words per link, more than 64 links
@pytest.mark.parametrize("S", [64, 512], ids=["W1", "W8"])
def test_words_per_link(S):
    lean, full = runs(NSF, S, B, LAUNCHES, False)
    same_bytes(lean["snap"], full["snap"], S)
    books_match_oracle(NSF, kwargs(S=S), lean, LAUNCHES, (0, B - 1))


def test_more_than_64_links():
    launches = (16, 40, 100)
    lean, full = runs(RING34, 320, 3, launches, False)
    same_bytes(lean["snap"], full["snap"], "ring34")
    books_match_oracle(RING34, kwargs(), lean, launches, (0, 2))


# ---------------------------------------------------------------------------------------- bit rates per lane
@pytest.mark.parametrize("n_rates", RATE_COUNTS)
def test_bit_rate_counts(n_rates):
    """16: one bit rate per lane; 17: lane 0 holds two; 32: every lane holds two; 33: the launch takes the full body and says so."""
    lean, full = runs(NSF, 320, B, LAUNCHES, False, n_rates)
    same_bytes(lean["snap"], full["snap"], n_rates)
    assert lean["snap"]["bit_rate_hist.requested"].shape == (B, n_rates)
    assert (lean["snap"]["bit_rate_hist.provisioned"] >= 1).all()
    books_match_oracle(NSF, kwargs(bit_rates=rates(n_rates)), lean, LAUNCHES, (0, B - 1))


def test_packed_counts_are_flushed_in_time():
    """One bit rate, 70 000 steps of one episode and one ticket: a count of 16 bits would run over without the flush every 32 768."""
    kw = dict(kwargs(load=10), bit_rates=(100,), episode_length=100000)
    lean, full = both(lambda: rmsa_env(NSF, B, "group", stats_level="full", **kw), (70000,))
    same_bytes(lean["snap"], full["snap"], "70 000 steps")
    assert (lean["snap"]["bit_rate_hist.requested"][:, 0] == 70001).all() and (lean["snap"]["episodes_done"] == 0).all()
    assert (lean["snap"]["counters.episode_services_processed"] == 70001).all()


# ---------------------------------------------------------------------------------------- the other kinds of handle
def test_per_environment_traffic():
    from optical_rl_gym_amd import make_sweep
    kw = {k: v for k, v in kwargs().items() if k not in ("load", "seed")}
    make = lambda: make_sweep("rmsa", topology(NSF), loads=(100.0, 400.0), seeds_per_load=3, seed=SEED, step_kernel="group",
                              stats_level="full", **kw)
    lean, full = both(make, LAUNCHES)
    assert set(lean["kernels"]) == {kernel_name("group", 320, "full", defer=True, traffic=True)}, lean["said"]
    same_bytes(lean["snap"], full["snap"], "traffic")


def test_request_trace():
    from optical_rl_gym_amd import RequestTrace
    from optical_rl_gym_amd.batched import DEFAULT_BIT_RATES
    rng, n, N = np.random.default_rng(SEED), sum(LAUNCHES) + 8, topology(NSF).num_nodes
    arrival = np.cumsum(rng.exponential(1 / 12.0, (B, n)), axis=1)
    src = rng.integers(0, N, (B, n))
    dst = (src + rng.integers(1, N, (B, n))) % N
    trace = RequestTrace(arrival, rng.exponential(25.0, (B, n)), src.astype(np.int32), dst.astype(np.int32),
                         rng.choice(DEFAULT_BIT_RATES, (B, n)).astype(np.int32), batch_size=B, layout="env")
    kw = {k: v for k, v in kwargs().items() if k not in ("load", "seed", "mean_service_holding_time")}
    lean, full = both(lambda: rmsa_env(NSF, B, "group", stats_level="full", trace=trace, **kw), LAUNCHES)
    assert set(lean["kernels"]) == {kernel_name("group", 320, "full", defer=True, trace=True)}, lean["said"]
    same_bytes(lean["snap"], full["snap"], "trace")
    assert (lean["snap"]["episodes_done"] >= 30).all()


# ---------------------------------------------------------------------------------------- a state a lean launch left
@pytest.mark.parametrize("env_vars", [{}, FORCED], ids=["tickets", "chunks7"])
def test_launches_on_a_state_a_lean_launch_left(env_vars):
    """lean, full (a launch with outputs), lean: the counters and the two sums pass between the lanes of one body and the registers
    of the other through the record"""
    make = lambda: rmsa_env(NSF, B, "group", stats_level="full", **kwargs())
    launches = [("sap_ff", 100, None, ()), ("sap_ff", 100, None, OUTS), ("sap_ff", 100, None, ())]
    alt = drive(make, launches, env_vars=env_vars)
    full = drive(make, launches, env_vars=dict(env_vars, **NO_LEAN))
    assert bodies(alt) == ["lean", "full", "lean"] and bodies(full) == ["full"] * 3, (alt["said"], full["said"])
    same_bytes(alt["snap"], full["snap"], "state")
    same_bytes(alt["outs"][1], full["outs"][1], "outputs")


def test_restore_after_a_lean_launch():
    with tooling_env():
        a = rmsa_env(NSF, B, "group", stats_level="full", **kwargs())
        a.run("sap_ff", 100, outputs=(), auto_reset=True)
        saved = a.save_state()
        a.run("sap_ff", 100, outputs=(), auto_reset=True)
        assert "body=lean" in a.last_kernel(), a.last_kernel()
        sa = snapshot(a)
        a.close()
    with tooling_env(**NO_LEAN):
        c = rmsa_env(NSF, B, "group", stats_level="full", **kwargs(seed=SEED + 100))
        c.load_state(saved)
        c.run("sap_ff", 100, outputs=(), auto_reset=True)
        assert "body=full" in c.last_kernel(), c.last_kernel()
        sc = snapshot(c)
        c.close()
    same_bytes(sa, sc, "restored, full body")
