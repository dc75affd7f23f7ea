"""The shapes of tests/test_gpu_provision_summary.py reach what they are there for -- asserted on the CPU oracle alone, so that a
shape that stops doing so is noticed without a GPU.  Every (accepted step, link) of every environment of a case is classified by
``provision_summary_cases.provisions``: the cases of the arithmetic in csrc/orlg_link_summary.h."""
import numpy as np
import pytest

from provision_summary_cases import B, CASES, CHUNKS, ENVS, LAUNCHES, provisions

STEP, LINK, WIN_S, WIN_E, USED_RUNS, FREE_RUNS, A, B_ = range(8)


def rows(case, envs=range(B)):
    return np.concatenate([provisions(case, i)[0] for i in envs])


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_environment_provisions_in_every_launch(case):
    for i in range(B):
        r, accepted = provisions(case, i)
        assert accepted >= 50, (case, i, accepted)
        t0 = 0
        for n in LAUNCHES:
            assert ((r[:, STEP] >= t0) & (r[:, STEP] < t0 + n)).any(), (case, i, n)
            t0 += n


@pytest.mark.parametrize("case", sorted(CASES))
def test_windows_with_no_one_and_two_free_neighbours(case):
    """a + b = 0 (the free run vanishes: F - 1), 1 and 2 (the run is split: F + 1), in the environments held to the oracle too"""
    for envs in (range(B), ENVS):
        r = rows(case, envs)
        ab = r[:, A] + r[:, B_]
        assert all((ab == k).sum() >= 2 for k in range(3)), (case, [int((ab == k).sum()) for k in range(3)])
        # the window joins used runs on both sides (U - 1), and starts at slot 0 (no slot below it)
        assert ((ab == 0) & (r[:, WIN_S] > 0)).any() and (r[:, WIN_S] == 0).any(), case


def test_windows_begin_and_end_on_the_word_boundary():
    r = rows("word_boundary")
    S = CASES["word_boundary"][1]
    assert S == 128
    assert (r[:, WIN_S] == 64).sum() >= 3 and (r[:, WIN_E] == 64).sum() >= 3   # slot s - 1 / slot e is in the other word
    assert ((r[:, WIN_S] < 64) & (r[:, WIN_E] > 64)).sum() >= 20                 # ... and windows over both words
    # a window starting at a multiple of 64 in the five-word shapes too
    for case in ("squeezed", "chunks"):
        q = rows(case)
        assert ((q[:, WIN_S] > 0) & (q[:, WIN_S] % 64 == 0)).any(), case


def test_slot_s_minus_1_is_not_in_the_last_word():
    S = CASES["s400"][1]
    assert (S + 63) // 64 == 7 and (S - 1) >> 6 == 6   # seven words of slots on the eight-word layout
    r = rows("s400")
    assert (r[:, WIN_E] > 384).any()           # windows in the word that holds slot S - 1,
    assert (r[:, WIN_E] == S - 1).any()        # up to the last slot a first fit takes: slot e = S - 1 is the neighbour above
    assert (r[:, WIN_E] < S).all()


def test_links_are_mostly_empty_when_provisioned():
    r = rows("empty_links")
    empty = r[:, USED_RUNS] == 0
    assert empty.mean() > 0.6, empty.mean()
    assert (~empty).sum() >= 100               # ... and not all of them
    # (an empty link has one free run and both neighbours free unless the window starts at slot 0)
    assert (r[empty][:, FREE_RUNS] == 1).all() and (r[empty][:, B_] == 1).all()
    for case in CASES:                         # every case meets an empty link: an environment starts with 22 or 238 of them
        assert (rows(case)[:, USED_RUNS] == 0).any(), case


def test_windows_are_squeezed_between_used_slots():
    r = rows("squeezed")
    ab = r[:, A] + r[:, B_]
    assert (ab == 0).sum() >= 20, int((ab == 0).sum())
    assert ((ab == 0) & (r[:, FREE_RUNS] >= 3)).any()   # a free run vanishes among several
    assert (r[:, USED_RUNS] >= 8).any()


def test_links_of_every_range_of_ids():
    r = rows("many_links")
    assert {int(l) >> 6 for l in r[:, LINK]} == {0, 1, 2, 3}


def test_a_provision_follows_every_chunk_start():
    assert CASES["chunks"][4]
    for i in range(B):
        r, _ = provisions("chunks", i)
        t0 = 0
        for n in LAUNCHES:
            if n > 16:   # (a launch of 16 steps strides over its quads: no tickets, so no chunks)
                steps = -(-n // CHUNKS)
                for c in range(CHUNKS):
                    lo, hi = t0 + c * steps, min(t0 + (c + 1) * steps, t0 + n)
                    assert ((r[:, STEP] >= lo) & (r[:, STEP] < hi)).any(), (i, n, c)
            t0 += n
