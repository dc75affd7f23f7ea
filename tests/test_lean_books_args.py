"""The shapes of tests/test_gpu_lean_books.py reach what they are there for -- asserted on the CPU oracle alone, so that a shape that
stops doing so is noticed without a GPU."""
import functools

import numpy as np

from gpu_support import oracle_env_from_kwargs, topology
from lean_books_cases import B, BOUNDARY_LAUNCHES, CHUNK_STEPS, CHUNKS, EPISODE, LAUNCHES, NSF, RATE_COUNTS, SEED, kwargs, rates


@functools.lru_cache(maxsize=None)
def stepped(seed, steps):
    """one environment of the base case, a step at a time: per step `done` and the services released"""
    o = oracle_env_from_kwargs(topology(NSF), kwargs(seed=seed))
    done, released, running = [], [], o.num_running()
    for _ in range(steps):
        tr = o.run("sap_ff", 1, reset_on_done=True)
        done.append(bool(tr["done"][0]))
        released.append(running + int(tr["accepted"][0]) - o.num_running())
        running = o.num_running()
    o.close()
    return np.array(done), np.array(released)


def test_every_bit_rate_arrives_and_is_accepted():
    for n in RATE_COUNTS:
        for i in range(B):
            o = oracle_env_from_kwargs(topology(NSF), kwargs(seed=SEED + i, bit_rates=rates(n)))
            for steps in LAUNCHES:
                o.run("sap_ff", steps, reset_on_done=True, fields=[])
            hist = o.bit_rate_hist()
            o.close()
            assert len(hist["requested"]) == n
            assert (hist["requested"] >= 1).all() and (hist["provisioned"] >= 1).all(), (n, i, hist)


def test_episodes_end_inside_a_launch_and_on_a_chunks_last_step():
    n = BOUNDARY_LAUNCHES[0]
    assert n == CHUNKS * CHUNK_STEPS and CHUNK_STEPS % (EPISODE - 1) == 0
    for i in range(B):
        done, _ = stepped(SEED + i, n)
        ends = np.flatnonzero(done)
        assert len(ends) >= 2, (i, ends)
        on_boundary = [t for t in ends if (t + 1) % CHUNK_STEPS == 0 and t + 1 < n]   # (the chunk behind it starts from the record)
        inside = [t for t in ends if (t + 1) % CHUNK_STEPS != 0]
        assert on_boundary and inside, (i, ends)


def test_a_step_releases_three_services():
    most = [int(stepped(SEED + i, sum(LAUNCHES))[1].max()) for i in range(B)]
    assert max(most) >= 3, most
