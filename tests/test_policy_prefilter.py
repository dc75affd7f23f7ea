"""What the cases of ``test_gpu_policy_prefilter.py`` exercise, pinned on the CPU oracle (no GPU): the group kernel's first-fit
passes after the first look only at the paths whose links all have a longest free run ml >= n, and a pass without such a path
is left out.  These are conditions on the inputs -- the loads and seeds of
``policy_prefilter_reference.CASES`` were chosen here so that the oracle alone meets them -- and one property of the test itself:
no path with a first fit ever fails it."""
import numpy as np
import pytest

import policy_prefilter_reference as ref

exp = ref.exp
LATER = [n for n, c in ref.CASES.items() if c["passes"] > 1]
ONE_PASS = [n for n, c in ref.CASES.items() if c["passes"] == 1]


def test_shapes(tmp_path):
    """every case has the passes it says: ceil(K / (16 // W))"""
    for name, c in ref.CASES.items():
        topo, W = ref.case_topology(name, tmp_path), exp.words_per_link(c["S"])
        assert -(-topo.k_paths // (16 // W)) == c["passes"], (name, topo.k_paths, W)
    assert sum(c["topo"].startswith("grid:") and c["passes"] >= 3 for c in ref.CASES.values()) == 2
    ring = ref.ring_topology(tmp_path)
    base = int(ring.pair_path_base[0 * ref.RING_N + 14])
    assert [int(h) for h in ring.path_hops[base:base + ref.RING_K]] == ref.RING_HOPS and int(ring.path_hops.max()) == 14


@pytest.mark.parametrize("name", LATER)
def test_case_holds_every_class(name, tmp_path):
    """at least 20 steps each: a later pass ruled out for the row, kept with a window found in it, kept without one"""
    pins, _ = ref.case_pins(name, tmp_path)
    print(name, pins)
    assert pins["ruled_out"] >= 20 and pins["kept_found"] >= 20 and pins["kept_none"] >= 20, (name, pins)
    assert pins["fit_fails_test"] == 0, (name, pins)


@pytest.mark.parametrize("name", ONE_PASS)
def test_controls_have_one_pass(name, tmp_path):
    """all K paths fit in the first pass: the new code is never reached, whatever the links hold"""
    pins, _ = ref.case_pins(name, tmp_path)
    assert pins["later_passes"] == 0 and pins["fit_fails_test"] == 0, (name, pins)


def test_middle_pass_ruled_out_last_pass_finds(tmp_path):
    """three passes (W = 8, two paths per pass): steps whose middle pass is ruled out and whose last pass holds the window"""
    pins, _ = ref.case_pins("nsf512_three_passes", tmp_path)
    assert pins["middle_out_last_found"] >= 5, pins


@pytest.mark.parametrize("name", ["nsf512_three_passes", "grid_k21_s192", "grid_k12_s320"])
def test_quad_skips_a_pass_and_a_later_one_finds(name, tmp_path):
    """at quad level, as the kernel votes: a pass skipped for the whole quad, then a pass that runs and finds a window -- the
    steps a `break` in the place of the `continue` would get wrong.  The three-pass NSFNET shape and both grids hold some (the
    ring, there for its hop layout, has none among its first eight environments and is not asked)."""
    pins, _ = ref.case_pins(name, tmp_path)
    print(name, pins["skip_then_find"])
    assert pins["skip_then_find"] >= 1, (name, pins)


def test_decided_by_one_slot(tmp_path):
    """over the file as a whole: a later-pass path kept by ml == n and one dropped by ml == n - 1 (every case has both)"""
    kept = sum(ref.case_pins(n, tmp_path)[0]["kept_by_ml_eq_n"] for n in LATER)
    dropped = sum(ref.case_pins(n, tmp_path)[0]["dropped_by_ml_eq_n_minus_1"] for n in LATER)
    assert kept >= 1 and dropped >= 1, (kept, dropped)


def test_no_fit_fails_the_test(tmp_path):
    """over every step of every trace: a path with a first fit has ml >= n on all its links, and the oracle's decision is the
    first such path's first fit (oracle_trace asserts the latter step by step)"""
    for name in ref.CASES:
        _, traces = ref.case_pins(name, tmp_path)
        for n, ml, start in traces:
            assert not ((start >= 0) & (ml < n)).any(), name


def test_schedules_on_a_hand_made_step():
    """quad_passes on rows written by hand: K = 5, three paths per pass"""
    def row(n, ml, start):
        return tuple(np.array(v) for v in (n, ml, start))
    found_first = row([4] * 5, [9] * 5, [0, 3, 3, 3, 3])
    blocked_no_candidate = row([4] * 5, [3] * 5, [-1] * 5)
    blocked_candidate = row([4] * 5, [3, 3, 3, 4, 3], [-1] * 5)       # path 3: a run of 4, no common window
    fits_later = row([4] * 5, [3, 3, 3, 3, 7], [-1, -1, -1, -1, 12])
    assert exp.quad_passes([found_first] * 4, 3) == (1, 1, 1)
    assert exp.quad_passes([found_first] * 3 + [blocked_no_candidate], 3) == (2, 1, 0 + 1)
    assert exp.quad_passes([found_first] * 3 + [blocked_candidate], 3) == (2, 2, 1)
    assert exp.quad_passes([blocked_no_candidate] * 3 + [fits_later], 3) == (2, 2, 1)
    assert exp.quad_passes([blocked_no_candidate] * 4, 3) == (2, 1, 0)
    assert exp.row_passes(*blocked_candidate, 3)[0] == [exp.KEPT_NONE] and exp.row_passes(*fits_later, 3) == ([exp.KEPT_FOUND], 1)
    # two paths per pass: the middle pass ruled out, the last one finds
    assert exp.row_passes(*fits_later, 2) == ([exp.RULED_OUT, exp.KEPT_FOUND], 2)
    assert exp.quad_passes([fits_later] * 4, 2) == (3, 2, 1)
