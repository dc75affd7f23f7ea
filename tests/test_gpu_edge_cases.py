"""Edge cases of the RMSA path on synthetic topologies (built with the package's own front-end from a link list), device vs
oracle bit for bit: the limits of the lane layout (k * W = 64 with S = 512, many links), a two-node network, slot counts that
are not a multiple of 64, and an over-provisioned queue."""
import numpy as np
import pytest

from gpu_support import compare_with_oracle, device_log_fixture, grid_edges, step_kernel, write_topology  # noqa: F401

# every edge case runs against both step kernels (the four-environments-per-wave kernel carries llp_ff itself since round 2; a shape
# whose four environments do not fit its LDS budget is served by the other one as well)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("step_kernel")]


@pytest.mark.parametrize("policy", ["sap_ff", "llp_ff"])
def test_widest_layout_k8_s512(tmp_path, policy, device_log_in_oracle, step_kernel):
    """k = 8 paths x W = 8 words fill the 64 lanes; 5 x 6 grid with diagonals: 30 nodes, 64 links."""
    pytest.importorskip("networkx")
    from optical_rl_gym_amd.topology_io import topology_from_txt
    rng = np.random.default_rng(3)
    edges = grid_edges(5, 6, rng)
    topo = topology_from_txt(write_topology(tmp_path, "grid30", 30, edges), "grid30", k_paths=8)
    assert topo.num_links == len(edges) and int(topo.path_hops.max()) <= 14
    kw = dict(num_spectrum_resources=512, load=400, mean_service_holding_time=20, episode_length=150, seed=31)
    tr = compare_with_oracle(topo, kw, policy, 400, 3, step_kernel)
    assert 0 < tr["accepted"].mean() < 1  # the load reaches blocking


def test_two_node_network(tmp_path, device_log_in_oracle, step_kernel):
    pytest.importorskip("networkx")
    from optical_rl_gym_amd.topology_io import topology_from_txt
    topo = topology_from_txt(write_topology(tmp_path, "pair", 2, [(1, 2, 300)]), "pair", k_paths=1)
    kw = dict(num_spectrum_resources=64, load=12, mean_service_holding_time=10, episode_length=50, seed=5)
    compare_with_oracle(topo, kw, "sap_ff", 300, 4, step_kernel)


@pytest.mark.parametrize("slots", [65, 100, 191, 320, 384, 400, 448])   # 400 / 448: seven words of slots on the eight-word layout
def test_slot_counts_off_the_word_boundary(tmp_path, slots, device_log_in_oracle, step_kernel):
    pytest.importorskip("networkx")
    from optical_rl_gym_amd.topology_io import topology_from_txt
    rng = np.random.default_rng(slots)
    edges = grid_edges(3, 3, rng)
    topo = topology_from_txt(write_topology(tmp_path, "grid9", 9, edges), "grid9", k_paths=3)
    kw = dict(num_spectrum_resources=slots, load=30 * slots / 100, mean_service_holding_time=15, episode_length=120, seed=slots)
    compare_with_oracle(topo, kw, "sap_ff", 300, 2, step_kernel)
