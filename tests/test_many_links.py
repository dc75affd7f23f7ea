"""Topologies of more than 64 and more than 128 links, what needs no GPU: the figures of the two link lists of our own
(``tests/golden/topology_txt/ring34.txt``, ``ring36.txt``; circulant graphs, ``make_golden.py::circulant``) that the GPU tests of
``test_gpu_many_links.py`` rely on, and the condition under which the two per-step link averages equal the reference's bit for
bit: the link list in graph order (``FrozenTopology.links_in_graph_order``).  The reference's own runs on the two networks join
``test_oracle_golden.py::test_rmsa_trace_bit_exact`` through their names (``rmsa_ring3*.npz``)."""
import numpy as np
import pytest

from conftest import load_golden, load_topology, oracle_env_from_kwargs
from gpu_support import FLOAT_FIELDS, INT_FIELDS

RING34, RING36 = "ring34_3-paths_6-modulations", "ring36_3-paths_6-modulations"
SHUFFLED = "ring34_shuffled_3-paths_6-modulations"
COMMITTED = ("nsfnet_chen_5-paths_6-modulations", "us14_3-paths_6-modulations", "jpn12_3-paths_6-modulations",
             "jpn12_5-paths_6-modulations", "spn_3-paths_6-modulations", RING34, RING36)

# links, path records, most hops, links that some path uses per range of 64 link ids, spectral efficiencies
# (ring34: one of the 1683 records, a third path of 2005 km, is beyond QPSK's 2000 km and has spectral efficiency 1)
FIGURES = {RING34: (238, 1683, 11, [36, 27, 28, 29], (1, 6)),
           RING36: (108, 1890, 14, [53, 38], (1, 6))}


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_fixture_figures(name):
    """What a regenerated link list must not quietly lose: the link counts on both sides of 64 and 128, paths over the links of
    every 64-id range (link ids of 128 and above are read back from a byte), a path of ORLG_MAX_HOPS = 14 hops on ring36."""
    links, records, hops_max, used_per_range, (se_lo, se_hi) = FIGURES[name]
    t = load_topology(name)
    assert t.k_paths == 3
    assert (t.num_links, t.num_paths, int(t.path_hops.max())) == (links, records, hops_max)
    used = np.unique(t.path_links)
    assert np.bincount(used >> 6, minlength=len(used_per_range)).tolist() == used_per_range
    assert (int(t.path_se.min()), int(t.path_se.max())) == (se_lo, se_hi)
    rec = t.packed_path_records()
    assert rec.dtype == np.uint8 and int(rec[:, 2:].max()) == int(t.path_links.max())   # the byte holds every link id
    if name == RING34:
        # 238 links: a partial last group of 4 (lint_stride), of 8 (link_stats_update), of 16 (the group kernel's rows), and
        # numpy's pairwise split 112 + 126 (n // 2 rounded down to a multiple of 8)
        E = t.num_links
        assert (E % 4, E % 8, E % 16) == (2, 6, 14) and (E + 3) & ~3 == 240
        assert (E // 2 - (E // 2) % 8, E - (E // 2 - (E // 2) % 8)) == (112, 126)
        assert int(t.path_links.max()) >= 192
    else:
        from optical_rl_gym_amd.topology import MAX_HOPS
        assert hops_max == MAX_HOPS and 64 < t.num_links <= 128


def test_committed_link_lists_are_in_graph_order():
    for name in COMMITTED:
        assert load_topology(name).links_in_graph_order, name


def test_ring34_shuffled_is_the_same_network():
    a, b = load_topology(RING34), load_topology(SHUFFLED)
    assert not b.links_in_graph_order
    assert a.nodes == b.nodes and a.num_paths == b.num_paths
    assert sorted((x, y, l) for x, y, _, _, l in a.edges) == sorted((x, y, l) for x, y, _, _, l in b.edges)
    assert [e[2] for e in a.edges] != [e[2] for e in b.edges]
    assert np.array_equal(a.path_hops, b.path_hops) and np.array_equal(a.path_length, b.path_length)


def test_link_order_decides_the_last_bits_of_the_link_averages():
    """The reference on ring34 with its link list permuted (``order_ring34_shuffled.npz``: sap_ff, S = 100, load 60, seed 5, 300
    steps).  It takes the two per-step link averages as ``np.mean`` over ``topology.edges()`` (graph order), the oracle -- and the
    kernels held to it -- in link-index order: every other field of the trace equals the recording exactly; the two averages are
    two summation orders of the same E non-negative terms, each within (E - 1) u of the exact sum, plus the division:
    rtol = 2 E 2^-53."""
    z, meta = load_golden("order_ring34_shuffled")
    assert meta["topology"] == SHUFFLED
    topo = load_topology(SHUFFLED)
    assert not topo.links_in_graph_order
    env = oracle_env_from_kwargs(topo, meta["env_kwargs"])
    tr = env.run(meta["policy"], meta["steps"], reset_on_done=meta["reset_on_done"])
    averages = ("avg_link_compactness", "avg_link_utilization")
    for f, g in (("src", "src_id"), ("dst", "dst_id"), ("act_path", "act_path"), ("act_slot", "act_slot")):
        assert np.array_equal(tr[f], z[g]), f
    for f in INT_FIELDS:
        assert np.array_equal(tr[f].astype(np.int64), z[f].astype(np.int64)), f
    for f in FLOAT_FIELDS:
        if f not in averages:
            assert np.array_equal(tr[f], z[f]), f
    rtol = 2 * topo.num_links * 2.0 ** -53
    differ = 0
    for f in averages:
        assert (z[f] >= 0).all()
        np.testing.assert_allclose(tr[f], z[f], rtol=rtol, atol=0, err_msg=f)
        differ += int((tr[f] != z[f]).sum())
    print("steps on which an average differs in its last bits:", differ, "of", 2 * meta["steps"])
    assert differ > 0   # (187 of 600: the order is what this recording is about)
    av = env.available_slots()
    assert np.array_equal(np.packbits(av, axis=1, bitorder="little"), z["final_available_slots"])
    ls = env.link_stats()
    for name in ("utilization", "external_fragmentation", "compactness", "last_update"):
        assert np.array_equal(ls[name], z["final_link_" + name]), name
    env.close()
