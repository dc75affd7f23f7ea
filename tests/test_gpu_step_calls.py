"""Every step entry point of the RMSA C API on the device, held to the table of ``step_call_reference`` (written from the contract
of ``include/orlg.h``): NSFNET with 320 slots, B = 4, statistics off, on a handle without a gate, a gated one and one whose gate
protects.  Every accepted call of the table's domain and, per entry kind, every distinct refusal goes through the public entry
point (the four plain entries each) with ``n_steps = 1`` (0 for the refusal of ``n_steps``) and a zero action array.  An accepted
call returns ORLG_OK and ``orlg_last_kernel`` names the instantiation the resolved (policy, assign) predicts -- B = 4 stays with
the wave-per-environment kernel, whose key reads STATS, DEFER, GN, CAUSE, ASSIGN, CUT, USAGE, PROTECT --; a refused call returns
the code and the text and leaves the counters and the trace position as they were."""
import numpy as np
import pytest

import gn_protect_reference as pref
from conftest import load_topology
from gpu_support import rmsa_env
from step_call_reference import (DEV_BEST_WINDOW, DEV_MIN_CUT, DEV_MOST_USED, ENTRIES, ENTRY_POINTS, FIRST, HANDLES, OK, SAP_FF, SP_FF,
                                 call_entry, device_cases, expected)

pytestmark = pytest.mark.gpu

B = 4
KW = dict(num_spectrum_resources=320, load=50, mean_service_holding_time=25, episode_length=1000, seed=21, stats_level="counters")


@pytest.fixture(scope="module")
def handles():
    topo = load_topology(pref.NSF)
    gates = {"plain": None, "gated": pref.case_gate(topo, protect=False), "protect": pref.case_gate(topo)}
    envs = {name: rmsa_env(topo, B, gn_gate=gates[name], **KW) for name in HANDLES}
    assert not envs["plain"].gn_gate and not envs["gated"].gn_protect and envs["protect"].gn_protect
    yield envs
    for env in envs.values():
        env.close()


def predicted_kernel(pair, handle, W=5):
    """the wave-per-environment instantiation of a one-step launch without outputs (csrc/orlg_variants.h OrlgWaveKey)"""
    policy, assign = pair
    gn, rule = handle != "plain", assign != FIRST
    name = "orlg_rmsa_kernel_ff" if not gn and not rule and policy in (SP_FF, SAP_FF) else "orlg_rmsa_kernel"
    flags = [False, gn, False, rule, assign == DEV_MIN_CUT, rule and (assign == DEV_MOST_USED or policy == DEV_BEST_WINDOW), handle == "protect"]
    while flags and not flags[-1]:
        flags.pop()
    return f"{name}<{W},0" + "".join(",true" if f else ",false" for f in flags) + ">"


def _state(env):
    return np.stack(list(env.counters().values())).tobytes(), int(env.L.orlg_trace_position(env.h))


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_case_through_the_public_entry_points(handles, entry):
    actions = np.zeros((B, 2), np.int32)
    accepted = refused = 0
    for policy, rule, mode, n_steps, handle in device_cases(entry):
        env = handles[handle]
        code, pair, text = expected(entry, policy, rule, mode, n_steps, handle)
        for name in ENTRY_POINTS[entry]:
            what = (name, policy, rule, mode, n_steps, handle)
            before = None if code == OK else _state(env)
            got = call_entry(env.L, env.h, name, policy, rule, mode, n_steps, actions.ctypes.data)
            assert got == code, (what, got, env.L.orlg_last_error())
            if code == OK:
                assert env.last_kernel().split(" ")[0] == predicted_kernel(pair, handle), (what, env.last_kernel())
                accepted += 1
            else:
                assert text in env.L.orlg_last_error().decode(), (what, env.L.orlg_last_error())
                assert _state(env) == before, what
                refused += 1
    print(entry, accepted, "accepted,", refused, "refused")
    assert accepted and refused
    for env in handles.values():
        env.synchronize()


def test_external_actions_need_an_array(handles):
    """the one check of a resolved call that needs more than the resolver sees: refused before anything is launched"""
    env = handles["plain"]
    before = _state(env)
    for name, policy, rule in (("orlg_step", -1, 0), ("orlg_step_diag", 5, 0), ("orlg_step_assign", 6, 2), ("orlg_step_min_cut", 6, 0),
                               ("orlg_step_window", 6, 100)):
        assert call_entry(env.L, env.h, name, policy, rule, 0, 1, None) == -1
        assert b"external actions need an action array" in env.L.orlg_last_error()
    assert _state(env) == before
