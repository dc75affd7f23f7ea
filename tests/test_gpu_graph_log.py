"""The lean body's logged graph statistics (csrc/orlg_graph_log.h, group_graph_replay): an accepted provision of a lean launch
logs what ``_update_network_stats`` consumes, one entry per lane of the environment's row, and the log is worked off when a row's
sixteen lanes are full and before a ticket's state leaves.  The full body (``ORLG_NO_LEAN``) updates the three doubles at every
provision: every case holds the whole state -- ``graph_stats()`` and ``save_state()`` included -- byte for byte between the two
bodies, and one case per shape against the C oracle on the device's logarithm.

What decides how a log fills is the number of accepted provisions per environment and ticket, so the cases assert those numbers
from the ``services_accepted`` counters: fewer than a log holds, exactly a multiple of it, several logs, rows of one quad that
differ, rows that all fill together.  (NSFNET at load 300 accepts the first 16 requests of every seed and blocks two thirds of
them once the spectrum has filled: counted on the CPU oracle, seeds 31 .. 36.)"""
import functools

import numpy as np
import pytest

from gpu_support import RMSA_OUTS as OUTS, against_oracle, device_log_fixture, drive, kernel_name, rmsa_env, same_bytes, snapshot, tooling_env  # noqa: F401

pytestmark = pytest.mark.gpu

NSF, RING34 = "nsfnet_chen_5-paths_6-modulations", "ring34_3-paths_6-modulations"
CAP = 16    # ORLG_GLOG_CAP: entries of an environment's log, one per lane of its row
SEED = 31
B = 6       # one full quad and one quad with two idle rows
# 16 steps: the final replay alone; 40: one full log and a rest; 300: several; 16 steps again, on a filled spectrum: a log that
# stays short of its capacity
LAUNCHES = (16, 40, 300, 16)
NO_LEAN, CHUNKS7 = {"ORLG_NO_LEAN": "1"}, {"ORLG_GROUP_CHUNKS": "7"}


def kwargs(S=320, load=300, seed=SEED):
    return dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=11, seed=seed)


def make(name=NSF, batch=B, **kw):
    return lambda: rmsa_env(name, batch, "group", stats_level="full", **kwargs(**kw))


def bodies(run):
    return [s.split("body=")[1].split()[0] if "body=" in s else None for s in run["said"]]


def accepted_per_launch(run):
    """[launch, environment]: accepted provisions of each launch, from the all-time counter read after every launch"""
    total = np.stack([np.zeros_like(run["each"][0])] + run["each"])
    return np.diff(total, axis=0)


def accepted(env):
    return env.counters()["services_accepted"].copy()


@functools.lru_cache(maxsize=None)
def runs(name, S, load, batch, launches, chunks):
    """lean and full body of one shape, whole-launch tickets or seven forced chunks"""
    run = functools.partial(drive, make(name, batch, S=S, load=load), launches, (), policy="sap_ff", each=accepted)
    extra = CHUNKS7 if chunks else {}
    lean, full = run(env_vars=extra), run(env_vars=dict(extra, **NO_LEAN))
    assert bodies(lean) == ["lean"] * len(launches) and bodies(full) == ["full"] * len(launches), (lean["said"], full["said"])
    assert set(lean["kernels"] + full["kernels"]) == {kernel_name("group", S, "full", defer=True)}, lean["said"]
    if chunks:   # (a launch of 16 steps strides over its quads: no tickets, so no chunks)
        assert all("chunks=7" in s for s, n in zip(lean["said"], launches) if n > 16), lean["said"]
    return lean, full


def check_graph_stats_moved(snap):
    assert (snap["graph_stats.last_update"] > 0).all() and (snap["graph_stats.throughput"] > 0).all()


# ---------------------------------------------------------------------------------------- the base case
@pytest.mark.parametrize("chunks", [False, True], ids=["tickets", "chunks7"])
def test_lean_log_equals_full_body(chunks, device_log_in_oracle):
    lean, full = runs(NSF, 320, 300, B, LAUNCHES, chunks)
    same_bytes(lean["snap"], full["snap"], ("lean", "full", chunks))
    check_graph_stats_moved(lean["snap"])
    acc = accepted_per_launch(lean)
    assert (acc[3] < CAP).any() and (acc[3] > 0).any(), acc       # a log that never fills: only the final replay
    assert (acc[0] == CAP).all(), acc                              # exactly one full log (every seed accepts its first 16 requests)
    assert (acc[2] > 2 * CAP).all(), acc                           # several replays within a launch
    assert ((acc[1] > CAP) & (acc[1] < 3 * CAP)).all(), acc        # a full log and a rest
    against_oracle(NSF, kwargs(), lean, "sap_ff", LAUNCHES, (0, 3, B - 1), "full", fields=())


def test_chunks_leave_the_same_state():
    """A ticket ends with a partly filled log; the next chunk of the quad goes to whichever wave draws it."""
    same_bytes(runs(NSF, 320, 300, B, LAUNCHES, False)[0]["snap"], runs(NSF, 320, 300, B, LAUNCHES, True)[0]["snap"], "chunks")


@pytest.mark.parametrize("env_vars", [{}, CHUNKS7], ids=["tickets", "chunks7"])
def test_a_handle_that_alternates(env_vars):
    """lean, full (a launch with outputs), lean: the three doubles pass between the registers of one body and the record of the other"""
    launches = [("sap_ff", 100, None, ()), ("sap_ff", 100, None, OUTS), ("sap_ff", 100, None, ())]
    alt = drive(make(), launches, env_vars=env_vars)
    full = drive(make(), launches, env_vars=dict(env_vars, **NO_LEAN))
    assert bodies(alt) == ["lean", "full", "lean"] and bodies(full) == ["full"] * 3, (alt["said"], full["said"])
    same_bytes(alt["snap"], full["snap"], "state")
    same_bytes(alt["outs"][1], full["outs"][1], "outputs")


@pytest.mark.parametrize("env_vars", [{}, CHUNKS7], ids=["tickets", "chunks7"])
def test_checkpoint_and_restore_between_launches(env_vars):
    """A checkpoint taken between two lean launches holds no pending entry: a fresh handle that loads it goes on to the same state."""
    with tooling_env(**env_vars):
        a = make()()
        a.run("sap_ff", 100, outputs=(), auto_reset=True)
        saved = a.save_state()
        a.run("sap_ff", 100, outputs=(), auto_reset=True)
        assert "body=lean" in a.last_kernel(), a.last_kernel()
        b = make(seed=SEED + 100)()
        b.load_state(saved)
        b.run("sap_ff", 100, outputs=(), auto_reset=True)
        sa, sb = snapshot(a), snapshot(b)
        a.close()
        b.close()
    same_bytes(sa, sb, "restored")
    with tooling_env(**dict(env_vars, **NO_LEAN)):
        c = make(seed=SEED + 100)()
        c.load_state(saved)
        c.run("sap_ff", 100, outputs=(), auto_reset=True)
        assert "body=full" in c.last_kernel(), c.last_kernel()
        sc = snapshot(c)
        c.close()
    same_bytes(sa, sc, "restored, full body")


# ---------------------------------------------------------------------------------------- rows of a quad
def test_rows_with_different_accept_counts(device_log_in_oracle):
    """Load 1000: most requests are blocked once the spectrum has filled, each row at its own steps."""
    launches = (300, 40, 16)
    lean, full = runs(NSF, 320, 1000, 8, launches, False)
    same_bytes(lean["snap"], full["snap"], "load 1000")
    acc = accepted_per_launch(lean)
    for launch in acc:
        for quad in (launch[:4], launch[4:]):
            assert len(set(quad.tolist())) > 1, acc    # the rows of a quad log different numbers of entries
    assert (acc[0] < 150).all(), acc                   # (blocked requests among the steps)
    against_oracle(NSF, kwargs(load=1000), lean, "sap_ff", launches, (1, 6), "full", fields=())


def test_rows_that_fill_together(device_log_in_oracle):
    """Load 1: every request is accepted, so all rows of every quad reach a full log at the same step."""
    launches = (100, 60)
    lean, full = runs(NSF, 320, 1, 8, launches, False)
    same_bytes(lean["snap"], full["snap"], "load 1")
    assert (accepted_per_launch(lean) == np.array(launches)[:, None]).all(), accepted_per_launch(lean)
    check_graph_stats_moved(lean["snap"])
    against_oracle(NSF, kwargs(load=1), lean, "sap_ff", launches, (0, 7), "full", fields=())


# ---------------------------------------------------------------------------------------- after reset()
@pytest.mark.parametrize("only_episode_counters", [False, True], ids=["full-reset", "episode-reset"])
def test_first_launch_after_reset(only_episode_counters):
    """After a full reset() the statistics start again: g_last_update = 0 meets the log's first entry."""
    snaps = {}
    for body, env_vars in (("lean", {}), ("full", NO_LEAN)):
        with tooling_env(**env_vars):
            env = make()()
            env.run("sap_ff", 100, outputs=(), auto_reset=True)
            env.reset(only_episode_counters=only_episode_counters)
            if not only_episode_counters:
                assert (env.graph_stats()["last_update"] == 0).all()
            env.run("sap_ff", 40, outputs=(), auto_reset=True)
            assert f"body={body}" in env.last_kernel(), env.last_kernel()
            snaps[body] = snapshot(env)
            env.close()
    same_bytes(snaps["lean"], snaps["full"], "after reset")
    check_graph_stats_moved(snaps["lean"])


# ---------------------------------------------------------------------------------------- field widths, words per link
def test_field_widths_on_238_links(device_log_in_oracle):
    """The largest E S the suite runs (ring34: 238 links of 320 slots, paths of up to 14 hops): the sums of the packed entry."""
    launches = (16, 40)
    lean, full = runs(RING34, 320, 300, 3, launches, False)
    same_bytes(lean["snap"], full["snap"], "ring34")
    assert (accepted_per_launch(lean).sum(axis=0) > CAP).all()
    against_oracle(RING34, dict(kwargs(), episode_length=11), lean, "sap_ff", launches, (0, 2), "full", fields=())


@pytest.mark.parametrize("S", [64, 512], ids=["W1", "W8"])
def test_words_per_link(S, device_log_in_oracle):
    """The replay knows no word count, but every instantiation has its own register allocation around it."""
    launches = (16, 40, 100)
    lean, full = runs(NSF, S, 300, B, launches, False)
    same_bytes(lean["snap"], full["snap"], S)
    assert (accepted_per_launch(lean).sum(axis=0) > CAP).all()
    against_oracle(NSF, kwargs(S=S), lean, "sap_ff", launches, (0, B - 1), "full", fields=())
