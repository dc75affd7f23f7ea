"""The lean body's statistics pass at a provision takes a link's seven integers -- free slots, free runs, used runs, first used
slot, end of the last used run, slot 0 free, slot S - 1 free -- from the link's summary, the window and its two neighbouring
slots (group_link_stats, FROMSUM; csrc/orlg_link_summary.h) and rescans the link for its longest free run alone.  The full body
(``ORLG_NO_LEAN``) keeps the full rescan: every case holds the final snapshot -- occupancy, link and graph statistics, counters,
the saved state with its ring -- byte for byte between the two bodies on the same launches, and the first, a middle and the last
environment against the C oracle on the device's logarithm.  The shapes are the smallest at which each case of the arithmetic
occurs; tests/test_provision_summary_args.py asserts on the oracle alone that they reach it."""
import functools

import pytest

from gpu_support import against_oracle, drive, kernel_name, rmsa_env, same_bytes
from provision_summary_cases import B, CASES, CHUNKS, ENVS, LAUNCHES, kwargs

pytestmark = pytest.mark.gpu

NO_LEAN = {"ORLG_NO_LEAN": "1"}


def bodies(run):
    return [s.split("body=")[1].split()[0] if "body=" in s else None for s in run["said"]]


@functools.lru_cache(maxsize=None)
def runs(case):
    """the case's launches on the lean body and on the full body: no outputs, full statistics"""
    name, S, _, policy, chunks = CASES[case]
    extra = {"ORLG_GROUP_CHUNKS": str(CHUNKS)} if chunks else {}
    make = lambda: rmsa_env(name, B, "group", stats_level="full", **kwargs(case))
    lean = drive(make, LAUNCHES, (), policy=policy, env_vars=extra)
    full = drive(make, LAUNCHES, (), policy=policy, env_vars=dict(extra, **NO_LEAN))
    assert bodies(lean) == ["lean"] * len(LAUNCHES) and bodies(full) == ["full"] * len(LAUNCHES), (lean["said"], full["said"])
    assert set(lean["kernels"] + full["kernels"]) == {kernel_name("group", S, "full", defer=True)}, lean["said"]
    if chunks:   # (a launch of 16 steps strides over its quads: no tickets, so no chunks)
        assert all(f"chunks={CHUNKS}" in s for s, n in zip(lean["said"], LAUNCHES) if n > 16), lean["said"]
    return lean, full


@pytest.mark.parametrize("case", sorted(CASES))
def test_lean_provision_equals_full_rescan(case):
    lean, full = runs(case)
    same_bytes(lean["snap"], full["snap"], case)
    assert (lean["snap"]["counters.services_processed"] == sum(LAUNCHES) + 1).all()
    assert (lean["snap"]["counters.services_accepted"] >= 50).all()


@pytest.mark.parametrize("case", sorted(CASES))
def test_lean_provision_equals_oracle(case):
    name, _, _, policy, _ = CASES[case]
    against_oracle(name, kwargs(case), runs(case)[0], policy, LAUNCHES, ENVS, "full", fields=())
