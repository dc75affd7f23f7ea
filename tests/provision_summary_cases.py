"""The shapes of tests/test_gpu_provision_summary.py, in a module of their own so that tests/test_provision_summary_args.py can
hold them to what they are for on the oracle alone, without a GPU.  No test lives here, and nothing here loads the library.

``provisions(case, i)`` steps environment i of a case on the oracle, a step at a time, and says of every (accepted step, link of
its path) what the lean body's statistics pass meets there: the link's used runs before, the window, and whether the slots next
to the window are free -- a and b of csrc/orlg_link_summary.h."""
import functools

import numpy as np

NSF, RING34 = "nsfnet_chen_5-paths_6-modulations", "ring34_3-paths_6-modulations"
SEED = 47
B = 5                        # one full quad, and one quad with three idle rows
ENVS = (0, 2, B - 1)         # the environments held to the oracle: the first, a middle one, the last
EPISODE = 90                 # shorter than the two longer launches: episodes end inside them (the occupancy stays as it is)
LAUNCHES = (16, 100, 300)
CHUNKS = 7                   # ORLG_GROUP_CHUNKS of the case that forces chunks

# name: (topology, slots, load, policy, forced chunks)
CASES = {
    "word_boundary": (NSF, 128, 120, "sap_ff", False),   # two words per link: windows that end or begin exactly at slot 64
    "s400": (NSF, 400, 600, "sp_ff", False),             # the 8-word layout: slot S - 1 sits in word 6, word 7 holds no slot
    "empty_links": (NSF, 320, 2, "sap_ff", False),       # links are mostly empty when provisioned: U == 0
    "squeezed": (NSF, 320, 300, "sap_ff", False),        # windows between used slots: a = b = 0, free runs vanish
    "many_links": (RING34, 100, 60, "sap_ff", False),    # 238 links: link ids of 64 and of 128 and above
    "chunks": (NSF, 320, 300, "sp_ff", True),            # a summary rebuilt at a chunk's start is the next provision's
}


def kwargs(case, seed=SEED):
    _, S, load, _, _ = CASES[case]
    return dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=EPISODE, seed=seed)


@functools.lru_cache(maxsize=None)
def provisions(case, i):
    """One row per (accepted step, link of its path) of environment i over LAUNCHES: step, link, s, e, used runs before, free runs
    before, a, b (int64 [rows, 8]), and the number of accepted steps."""
    from gpu_support import oracle_env_from_kwargs, topology
    name, S, _, policy, _ = CASES[case]
    topo = topology(name)
    o = oracle_env_from_kwargs(topo, kwargs(case), seed=SEED + i)
    rows, accepted = [], 0
    for t in range(sum(LAUNCHES)):
        occ, r = o.available_slots(), o.request()
        path, s = o.policy(policy)
        n = o.number_slots(path) if path >= 0 else 0
        tr = o.run(policy, 1, reset_on_done=True, fields=["accepted", "act_path", "act_slot"])
        if not tr["accepted"][0]:
            continue
        assert (int(tr["act_path"][0]), int(tr["act_slot"][0])) == (path, s)
        accepted += 1
        g = int(topo.pair_path_base[r.src * topo.num_nodes + r.dst]) + path
        for link in topo.path_links[topo.path_link_off[g]:topo.path_link_off[g + 1]]:
            free = occ[link].astype(np.int64)
            assert free[s:s + n].all()   # the window was wholly free
            edges = np.diff(np.concatenate([[1], free, [1]]))   # a used run starts at -1 and ends at +1
            used_runs = int((edges == -1).sum())
            free_runs = int((np.diff(np.concatenate([[0], free, [0]])) == 1).sum())
            a = int(s > 0 and free[s - 1])
            b = int(s + n < S and free[s + n])
            rows.append((t, int(link), s, s + n, used_runs, free_runs, a, b))
    o.close()
    return np.array(rows, np.int64).reshape(-1, 8), accepted
