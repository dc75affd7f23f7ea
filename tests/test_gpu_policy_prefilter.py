"""The longest-run test of the group kernel's later first-fit passes: a first-fit pass after the first looks
only at the paths whose links all have a free run of n slots, from the links' summaries in LDS, and a pass no row has such a path
for is left out.  Results do not change, and every case is held three ways:

1. the state the lean launch leaves equals, byte for byte, the state the same handle leaves when stepped with ``ORLG_NO_LEAN``
   (the full body of the same instantiation: it keeps the summaries and does not run the test),
2. and with ``ORLG_NO_DEFER`` (the plain kind: no summaries, code that is what it was);
3. the full body's ``act_path``, ``act_slot`` and ``accepted`` and the final state equal the CPU oracle's, every environment.

What the cases exercise -- later passes ruled out, kept with and without a window, paths decided by one slot, a middle pass
ruled out before a last one that finds -- is pinned on the CPU by ``test_policy_prefilter.py``."""
import functools

import pytest

import policy_prefilter_reference as ref
from gpu_support import (against_oracle, device_log_fixture, drive, kernel_name, rmsa_env, same_bytes, snapshot,  # noqa: F401
                         tooling_env)

pytestmark = pytest.mark.gpu

NO_LEAN, NO_DEFER, CHUNKS7 = {"ORLG_NO_LEAN": "1"}, {"ORLG_NO_DEFER": "1"}, {"ORLG_GROUP_CHUNKS": "7"}
DECIDED = ("act_path", "act_slot", "accepted")


def maker(name, tmp_path, batch=None):
    topo, kw = ref.case_topology(name, tmp_path), ref.case_kwargs(name)
    return lambda: rmsa_env(topo, batch or ref.CASES[name]["B"], "group", stats_level="full", **kw)


def bodies(run):
    return [s.split("body=")[1].split()[0] if "body=" in s else None for s in run["said"]]


def three_ways(name, tmp_path, batch=None, extra=None):
    """The case's launch four times -- lean, full body, plain kind, full body with the decisions as outputs -- and the checks 1-3."""
    c, extra = ref.CASES[name], extra or {}
    make, B, S = maker(name, tmp_path, batch), batch or ref.CASES[name]["B"], c["S"]
    run = functools.partial(drive, make, [c["steps"]], policy="sap_ff")
    lean = run((), env_vars=extra)
    full = run((), env_vars=dict(extra, **NO_LEAN))
    plain = run((), env_vars=dict(extra, **NO_DEFER))
    out = run(DECIDED, env_vars=extra)
    assert bodies(lean) == ["lean"] and bodies(full) == ["full"] and bodies(out) == ["full"], (lean["said"], full["said"], out["said"])
    assert lean["kernels"] == full["kernels"] == out["kernels"] == [kernel_name("group", S, "full", defer=True)], lean["said"]
    assert plain["kernels"] == [kernel_name("group", S, "full")], plain["said"]
    if extra == CHUNKS7:
        assert "chunks=7" in lean["said"][0] and "chunks=7" in full["said"][0], lean["said"]
    same_bytes(lean["snap"], full["snap"], (name, "lean against the full body"))
    same_bytes(lean["snap"], plain["snap"], (name, "lean against the plain kind"))
    same_bytes(lean["snap"], out["snap"], (name, "lean against the launch with outputs"))
    topo = c["topo"] if not (c["topo"] == "ring" or c["topo"].startswith("grid:")) else ref.case_topology(name, tmp_path)
    against_oracle(topo, ref.case_kwargs(name), out, "sap_ff", c["steps"], range(B), "full", fields=DECIDED)
    assert 0 < out["tr"]["accepted"].mean() < 1
    return lean, out


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_case(name, tmp_path, device_log_in_oracle):
    """NSFNET with two passes at two loads and with three passes, the one-pass controls (NSFNET S = 128, US14 k = 3: the kernel and
    its decisions as before), two many-paths grids, the ring with paths of up to 14 hops, JPN12."""
    three_ways(name, tmp_path)


def test_chunks_rebuild_the_summaries(tmp_path, device_log_in_oracle):
    """seven forced chunks: the summaries the test reads are rebuilt at every ticket, by whichever wave draws it"""
    three_ways("nsf320_load50", tmp_path, extra=CHUNKS7)


def test_partial_last_quad(tmp_path, device_log_in_oracle):
    """B = 18: the last quad has two rows past the batch's end, which must neither keep nor skip a pass for the other two"""
    three_ways("nsf320_load150", tmp_path, batch=18)


def test_checkpoint_mid_run(tmp_path, device_log_in_oracle):
    """A checkpoint between two lean launches, restored into a fresh handle: the summaries are not part of the state, the handle
    that loads it rebuilds them and goes on to the same bytes; and to the oracle's state."""
    name = "nsf320_load50"
    make, c = maker(name, tmp_path), ref.CASES[name]
    a = make()
    a.run("sap_ff", 200, outputs=(), auto_reset=True)
    saved = a.save_state()
    a.run("sap_ff", c["steps"] - 200, outputs=(), auto_reset=True)
    assert "body=lean" in a.last_kernel(), a.last_kernel()
    b = rmsa_env(c["topo"], c["B"], "group", stats_level="full", **dict(ref.case_kwargs(name), seed=ref.SEED0 + 100))
    b.load_state(saved)
    b.run("sap_ff", c["steps"] - 200, outputs=(), auto_reset=True)
    assert "body=lean" in b.last_kernel(), b.last_kernel()
    sa, sb = snapshot(a), snapshot(b)
    a.close()
    b.close()
    same_bytes(sa, sb, "restored")
    against_oracle(c["topo"], ref.case_kwargs(name), dict(snap=sb, tr={}), "sap_ff", c["steps"], range(c["B"]), "full", fields=())


def test_lean_and_full_launches_alternate(tmp_path, device_log_in_oracle):
    """one handle, lean - full (outputs) - lean - full: either body meets the summaries the other one kept"""
    name = "ring_k8_s320"
    launches = [("sap_ff", 100, None, ()), ("sap_ff", 100, None, DECIDED), ("sap_ff", 100, None, ()), ("sap_ff", 100, None, DECIDED)]
    alt = drive(maker(name, tmp_path), launches)
    full = drive(maker(name, tmp_path), launches, env_vars=NO_LEAN)
    plain = drive(maker(name, tmp_path), launches, env_vars=NO_DEFER)
    assert bodies(alt) == ["lean", "full", "lean", "full"] and bodies(full) == ["full"] * 4, (alt["said"], full["said"])
    same_bytes(alt["snap"], full["snap"], "alternating against the full body")
    same_bytes(alt["snap"], plain["snap"], "alternating against the plain kind")
    for k in (1, 3):
        same_bytes(alt["outs"][k], plain["outs"][k], ("outputs of launch", k))
    against_oracle(ref.case_topology(name, tmp_path), ref.case_kwargs(name), dict(snap=alt["snap"], tr={}), "sap_ff", 400,
                   range(ref.CASES[name]["B"]), "full", fields=())
