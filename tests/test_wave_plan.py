"""What the host decides about a launch of the wave-per-environment step kernels (csrc/orlg_wave_plan.h), without a device:
``orlg_debug_wave_plan`` takes the launch as the step entries resolve it, a workgroup and the resident workgroups, and returns the
kernel family and key, the workgroup of a launch that keeps bytes behind the wave regions, the grid and the tickets.  The order of
its fields is read from the X-macros next to it, so every value below is asked for by name.

The expected values are those of the arithmetic as it stood inside ``launch_rmsa``, ``mm_geometry`` and ``launch_rmsa_am`` before the
header existed: ``expected_key`` restates the decisions of ``launch_rmsa`` one for one, the literal rows pin what it must say for the
launches the GPU tests name, and the geometry is computed by hand below.

The shape is NSFNET with 320 slots (W = 5) and full statistics: 14 320 B of tables and output pointers, and per wave 880 B of
occupancy, 12 B per queue slot, 2496 B of MT19937 state, 704 + 336 + 96 B of link statistics, histogram (21 bit rates) and span cache,
192 + 128 B of scalars and 1280 B of arrival ring = 6112 + 12 Q bytes.  ``rmsa_create`` picks 8 waves per workgroup for Q = 128 (75 504 B) and for
Q = 1024 (161 520 B).  A queue of more than 4096 slots is refused at create time; the plan is arithmetic, and the two such queues
below only serve to make one wave not fit."""
import ctypes as C
import itertools

import pytest

from gpu_support import LLP, MODE_EPISODE_RESET, MODE_INIT, MODE_STEP, OUT_ACCEPTED, OUT_ASSIGN_BIT, OUT_CAUSE_BIT, OUT_LINK_UTIL, SAP, SP, wave_plan
from optical_rl_gym_amd import _lib

EXTERNAL, BEST_WINDOW = -1, 9   # ORLG_POLICY_EXT, ORLG_POLICY_BEST_WINDOW
FIRST, LAST, MIN_CUT, MOST_USED = 0, 2, 5, 6   # ORLG_ASSIGN_*
KEY = ("kernel", "STATS", "DEFER", "GN", "CAUSE", "ASSIGN", "CUT", "USAGE", "PROTECT")
LDS = 160 * 1024


def test_a_wrong_number_of_inputs_is_refused():
    f = _lib.load().orlg_debug_wave_plan
    f.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    assert f((C.c_int32 * 4)(), 4, (C.c_int32 * 64)(), 64) < 0


# ---------------------------------------------------------------------------------------- the key
def expected_key(policy, K, stats, n_steps, cause, assign, gated, protect):
    """launch_rmsa's decisions for a step of a handle whose gate does not choose the modulation"""
    out_mask = (OUT_CAUSE_BIT if cause else 0) | (OUT_ASSIGN_BIT if assign != FIRST else 0)
    rule = assign != FIRST
    ff = not gated and not cause and not rule and K <= 8 and policy in (SP, SAP)
    df = not gated and stats >= 2 and n_steps >= 16 and out_mask == 0
    usage = rule and (assign == MOST_USED or policy == BEST_WINDOW)
    return dict(kernel="orlg_rmsa_kernel_ff" if ff else "orlg_rmsa_kernel", STATS=stats, DEFER=int(df), GN=int(gated), CAUSE=int(cause),
                ASSIGN=int(rule), CUT=int(rule and assign == MIN_CUT), USAGE=int(usage), PROTECT=int(gated and protect)), out_mask


def test_key_truth_table():
    rows = 0
    for (gated, protect, adaptive), cause, assign, policy, K, n_steps, stats in itertools.product(
            ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1)), (0, 1), (FIRST, LAST, MIN_CUT, MOST_USED), (SP, SAP, LLP, EXTERNAL, BEST_WINDOW),
            (8, 9), (1, 16, 1000), (0, 1, 2)):
        rule = assign != FIRST
        if policy == BEST_WINDOW and (not rule or assign == MIN_CUT):
            continue   # (the route exists under orlg_step_window's rules only)
        if (policy == EXTERNAL and (rule or n_steps != 1)) or (protect and rule) or (gated and (assign == MOST_USED or policy == BEST_WINDOW)):
            continue   # (refused by the step entries)
        if adaptive and (cause or rule):
            continue   # (refused on a handle whose gate chooses the modulation)
        want, out_mask = expected_key(policy, K, stats, n_steps, cause, assign, gated, protect)
        got = wave_plan(policy=policy, K=K, stats_level=stats, n_steps=n_steps, out_mask=out_mask, assign=assign, gated=gated,
                        adaptive=adaptive, protect=protect)
        if adaptive:   # orlg_rmsa_am_kernel whatever the policy
            assert (got["family"], got["kernel"], got["STATS"]) == ("AM", None, stats) and not any(got[f] for f in KEY[2:])
        else:
            assert got["family"] == "PLAIN" and {f: got[f] for f in KEY} == want, (policy, K, stats, n_steps, cause, assign, gated, protect)
        rows += 1
    # per {cause} x {K} x {stats}: (route, rule, n_steps) 3 x 4 x 3 + external + any x 2 x 3 without a gate, 3 x 3 x 3 + external
    # behind one, 3 x 3 + external on a protecting handle; the same 10 without a cause on an adaptive one
    assert rows == 12 * (43 + 28 + 10) + 6 * 10 == 1032


def key(**kw):
    got = wave_plan(**kw)
    return (got["family"], got["kernel"]) + tuple(got[f] for f in KEY[1:])


def test_the_keys_the_gpu_tests_name():
    """(family, kernel, STATS, DEFER, GN, CAUSE, ASSIGN, CUT, USAGE, PROTECT) of the launches test_gpu_kernel_selection and the
    per-feature GPU tests pin by name"""
    R, F = "orlg_rmsa_kernel", "orlg_rmsa_kernel_ff"
    assert key() == ("PLAIN", F, 2, 1, 0, 0, 0, 0, 0, 0)                                  # sap_ff, 1000 steps: <W,2,true> of _ff
    assert key(n_steps=15) == ("PLAIN", F, 2, 0, 0, 0, 0, 0, 0, 0)
    assert key(no_defer=1) == ("PLAIN", F, 2, 0, 0, 0, 0, 0, 0, 0)
    assert key(stats_level=1) == ("PLAIN", F, 1, 0, 0, 0, 0, 0, 0, 0)
    assert key(out_mask=OUT_ACCEPTED) == ("PLAIN", F, 2, 1, 0, 0, 0, 0, 0, 0)
    assert key(out_mask=OUT_LINK_UTIL) == ("PLAIN", F, 2, 0, 0, 0, 0, 0, 0, 0)
    assert key(K=9) == ("PLAIN", R, 2, 1, 0, 0, 0, 0, 0, 0)                               # more than eight paths: the general kernel
    assert key(policy=LLP) == ("PLAIN", R, 2, 1, 0, 0, 0, 0, 0, 0)
    assert key(policy=EXTERNAL, n_steps=1) == ("PLAIN", R, 2, 0, 0, 0, 0, 0, 0, 0)
    assert key(gated=1) == ("PLAIN", R, 2, 0, 1, 0, 0, 0, 0, 0)                           # a gate: no _ff, no DEFER
    assert key(gated=1, out_mask=OUT_CAUSE_BIT) == ("PLAIN", R, 2, 0, 1, 1, 0, 0, 0, 0)
    assert key(gated=1, protect=1) == ("PLAIN", R, 2, 0, 1, 0, 0, 0, 0, 1)
    assert key(protect=1) == ("PLAIN", F, 2, 1, 0, 0, 0, 0, 0, 0)                         # (protection is the gate's)
    assert key(out_mask=OUT_CAUSE_BIT) == ("PLAIN", R, 2, 0, 0, 1, 0, 0, 0, 0)
    assert key(out_mask=OUT_ASSIGN_BIT, assign=LAST) == ("PLAIN", R, 2, 0, 0, 0, 1, 0, 0, 0)
    assert key(out_mask=OUT_ASSIGN_BIT, assign=MIN_CUT) == ("PLAIN", R, 2, 0, 0, 0, 1, 1, 0, 0)
    assert key(out_mask=OUT_ASSIGN_BIT, assign=MOST_USED) == ("PLAIN", R, 2, 0, 0, 0, 1, 0, 1, 0)
    assert key(out_mask=OUT_ASSIGN_BIT, assign=LAST, policy=BEST_WINDOW) == ("PLAIN", R, 2, 0, 0, 0, 1, 0, 1, 0)
    assert key(assign=MOST_USED) == ("PLAIN", F, 2, 1, 0, 0, 0, 0, 0, 0)                  # (without the bit the rule is not read)
    assert key(gated=1, out_mask=OUT_ASSIGN_BIT | OUT_CAUSE_BIT, assign=MIN_CUT) == ("PLAIN", R, 2, 0, 1, 1, 1, 1, 0, 0)
    # orlg_step_max_margin: its own kernel, the classifier its only flag; protection is an argument of the launch
    assert key(gated=1, max_margin=1) == ("MM", None, 2, 0, 0, 0, 0, 0, 0, 0)
    assert key(gated=1, max_margin=1, protect=1, out_mask=OUT_CAUSE_BIT, stats_level=0) == ("MM", None, 0, 0, 0, 1, 0, 0, 0, 0)
    # a gate that chooses the modulation: its own kernel whatever the policy
    assert key(gated=1, adaptive=1, policy=LLP, stats_level=1) == ("AM", None, 1, 0, 0, 0, 0, 0, 0, 0)
    assert key(adaptive=1) == ("PLAIN", F, 2, 1, 0, 0, 0, 0, 0, 0)                        # (the mode is the gate's)
    # the initial and the episode reset: the reset kernel per statistics level, whatever else the parameters carry
    for mode in (MODE_INIT, MODE_EPISODE_RESET):
        for stats in (0, 1, 2):
            for kw in (dict(), dict(gated=1, protect=1), dict(gated=1, adaptive=1), dict(out_mask=OUT_CAUSE_BIT | OUT_ASSIGN_BIT, assign=MIN_CUT)):
                assert key(mode=mode, stats_level=stats, **kw) == ("PLAIN", "orlg_rmsa_reset_kernel", stats, 0, 0, 0, 0, 0, 0, 0)


# ---------------------------------------------------------------------------------------- bytes behind the wave regions
SHARED, USAGE_BYTES = 14320, 256 * 5   # ORLG_USAGE_BYTES(W)
wave_bytes = lambda Q: 6112 + 12 * Q
mm_bytes = lambda Q: (4 * Q + 15) & ~15

# (Q, the handle's waves per workgroup, bytes behind a wave region) -> (waves per workgroup of the launch, its LDS bytes)
GEOMETRY = [
    # the full workgroup fits: 14 320 + 8 x (7648 + 1280) and 14 320 + 8 x (7648 + 512)
    ((128, 8, USAGE_BYTES), (8, 85744)), ((128, 8, mm_bytes(128)), (8, 79600)),
    # fewer waves: 14 320 + 8 x 19 680 = 171 760 > 163 840, 7 fit; 14 320 + 7 x 22 496 = 171 792 >, 6 fit
    ((1024, 8, USAGE_BYTES), (7, 152080)), ((1024, 8, mm_bytes(1024)), (6, 149296)),
    # one wave does not fit: 14 320 + 148 384 + 1280 = 163 984; 14 320 + 128 992 + 40 960 = 184 272
    ((11856, 1, USAGE_BYTES), (0, 163984)), ((10240, 1, mm_bytes(10240)), (0, 184272)),
    # nothing behind the regions: the handle's own workgroup
    ((128, 8, 0), (8, 75504)), ((1024, 8, 0), (8, 161520)), ((11856, 1, 0), (1, 162704)), ((10240, 1, 0), (1, 143312))]


@pytest.mark.parametrize("shape,want", GEOMETRY)
def test_extra_lds_geometry(shape, want):
    (Q, wpb, extra), (wpu, lds) = shape, want
    got = wave_plan(wave_bytes=wave_bytes(Q), extra_per_wave=extra, wpb=wpb, gated=1)
    assert (got["wpu"], got["lds"]) == (wpu, lds)
    assert (lds <= LDS) == (wpu > 0)
    if 0 < wpu < wpb:   # the largest that fits
        assert SHARED + (wpu + 1) * (wave_bytes(Q) + extra) > LDS
    if not wpu:   # refused: no grid
        assert (got["nblocks"], got["ticket_stride"], got["ticket_advance"]) == (0, 0, 0)


# ---------------------------------------------------------------------------------------- the grid and the tickets
@pytest.mark.parametrize("B,wpu,resident,nblocks", [(2047, 8, 256, 256), (2048, 8, 256, 256), (2049, 8, 256, 256), (2041, 8, 256, 256),
                                                    (2040, 8, 256, 255), (64, 8, 256, 8), (65, 8, 256, 9), (1, 8, 256, 1), (64, 7, 256, 10),
                                                    (1792, 7, 256, 256), (1786, 7, 256, 256), (1785, 7, 256, 255), (100000, 1, 512, 512)])
def test_grid(B, wpu, resident, nblocks):
    """ceil(B / waves per workgroup), capped by the resident workgroups: below, at and above resident x wpu"""
    extra = {8: 0, 7: USAGE_BYTES, 1: 0}[wpu]
    Q = {8: 128, 7: 1024, 1: 10240}[wpu]
    got = wave_plan(B=B, resident=resident, wave_bytes=wave_bytes(Q), extra_per_wave=extra, wpb=8 if wpu > 1 else 1)
    assert (got["wpu"], got["nblocks"]) == (wpu, nblocks)


@pytest.mark.parametrize("mode,n_steps,stride,advance", [(MODE_STEP, 1, 1, 0), (MODE_STEP, 16, 1, 0), (MODE_STEP, 17, 0, 4096), (MODE_STEP, 1000, 0, 4096),
                                                         (MODE_INIT, 1, 1, 0), (MODE_INIT, 1000, 1, 0), (MODE_EPISODE_RESET, 17, 1, 0)])
def test_tickets(mode, n_steps, stride, advance):
    """up to 16 steps, and both resets whatever n_steps says: a static stride; longer launches draw tickets and move ticket_base by B"""
    for kw in (dict(), dict(gated=1, max_margin=1), dict(gated=1, adaptive=1)):
        if mode != MODE_STEP and kw:
            continue   # (the MM and AM kernels are launched in step mode only)
        got = wave_plan(mode=mode, n_steps=n_steps, B=4096, **kw)
        assert (got["ticket_stride"], got["ticket_advance"]) == (stride, advance)
