"""Per-environment traffic without a device: the host arithmetic of ``traffic.py`` (rates, sweep layout), the argument
checks of the batched constructors (raised before the library is loaded) and the per-load Monitor tree."""
import os

import numpy as np
import pytest

FIXTURE_LOADS = (20, 50, 80, 300, 900, 1400, 2400, 3000, 4000)


@pytest.mark.parametrize("load", FIXTURE_LOADS)
@pytest.mark.parametrize("holding", [25, 25.0, 10800.0, 7.3])
def test_per_env_rates_scalar_is_the_scalar_formula(load, holding):
    from optical_rl_gym_amd import traffic
    # batched.py / phy.py (optical_network_env.py:127-129, rmsa_env.py:646-651)
    iat = 1 / float(load / float(holding))
    arrival, hold = 1 / iat, 1 / holding
    a, h = traffic.per_env_rates(5, load, holding)
    assert a.dtype == np.float64 and h.dtype == np.float64 and a.shape == (5,) and h.shape == (5,)
    assert all(x.hex() == float(arrival).hex() for x in a.tolist())
    assert all(x.hex() == float(hold).hex() for x in h.tolist())


def test_per_env_rates_elementwise():
    from optical_rl_gym_amd import traffic
    loads = np.array(FIXTURE_LOADS, np.float64)
    holds = np.linspace(5.0, 10800.0, len(FIXTURE_LOADS))
    a, h = traffic.per_env_rates(len(loads), loads, holds)
    for i in range(len(loads)):
        iat = 1 / float(float(loads[i]) / float(holds[i]))
        assert a[i].hex() == (1 / iat).hex() and h[i].hex() == (1 / float(holds[i])).hex()
    a2, h2 = traffic.per_env_rates(len(loads), list(loads), 25)
    assert np.array_equal(h2, np.full(len(loads), 1 / 25)) and a2[1] == 1 / (1 / (50 / 25.0))


@pytest.mark.parametrize("load,holding", [([1, 2, 3], 25), (np.ones((4, 1)), 25), (50, [25, 25]), ([50, 0, 50, 50], 25),
                                          ([50, -1, 50, 50], 25), ([50, np.nan, 50, 50], 25), (50, np.inf), (50, 0),
                                          (np.inf, 25)])
def test_per_env_rates_rejects(load, holding):
    from optical_rl_gym_amd import traffic
    with pytest.raises(ValueError):
        traffic.per_env_rates(4, load, holding)


def test_load_sweep_layout():
    from optical_rl_gym_amd import traffic
    loads = [1200, 1280, 1360]
    load, seeds, group = traffic.load_sweep(loads, 4, seed=10)
    assert load.shape == seeds.shape == group.shape == (12,)
    assert load.dtype == np.float64 and seeds.dtype == np.uint64 and group.dtype == np.int32
    for g in range(3):
        for r in range(4):
            i = g * 4 + r
            assert load[i] == loads[g] and seeds[i] == 10 + r and group[i] == g
    assert np.array_equal(traffic.load_sweep([5.0], 3)[1], [41, 42, 43])   # optical_network_env.py:266-271: seed None = 41
    for bad in (([], 4), ([1, -2], 4), ([1, 2], 0), ([1, 2], 1.5), (list(range(1, 258)), 1), ([[1, 2]], 2)):
        with pytest.raises(ValueError):
            traffic.load_sweep(*bad)
    assert np.array_equal(traffic.group_loads(load, group, 3), loads)
    with pytest.raises(ValueError):   # a group of two loads has no load to be named after
        traffic.group_loads([20.0, 30.0, 30.0], [0, 0, 1], 2)


def test_check_groups():
    from optical_rl_gym_amd import traffic
    g, n = traffic.check_groups(4, None)
    assert n == 1 and np.array_equal(g, [0, 0, 0, 0])
    g, n = traffic.check_groups(4, [2, 0, 2, 1])
    assert n == 3 and g.dtype == np.int32
    assert traffic.check_groups(4, [0, 0, 1, 1], 256)[1] == 256
    for bad in (([0, 1, 2], None), ([0, 1, 2, 3], 3), ([0, -1, 0, 0], None), ([0, 0, 0, 0], 257), ([0, 0, 0, 300], None)):
        with pytest.raises(ValueError):
            traffic.check_groups(4, *bad)
    with pytest.raises(TypeError):
        traffic.check_groups(4, [0.0, 1.0, 0.0, 1.0])


def test_constructor_errors_come_before_the_library(monkeypatch, nsfnet):
    """Shapes and values of load= / mean_service_holding_time= / groups= are checked before liborlg.so is loaded."""
    from conftest import load_phy_tables, load_topology
    from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedPhyRMSAEnv, BatchedRMSAEnv, _lib, make_sweep

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    kw = dict(num_spectrum_resources=320, mean_service_holding_time=25)
    with pytest.raises(ValueError):
        BatchedRMSAEnv(nsfnet, 4, load=[50, 60, 70], **kw)
    with pytest.raises(ValueError):
        BatchedRMSAEnv(nsfnet, 4, load=[50, 60, 70, np.nan], **kw)
    with pytest.raises(ValueError):
        BatchedRMSAEnv(nsfnet, 4, load=[50, 60, 70, 0], **kw)
    with pytest.raises(ValueError):
        BatchedRMSAEnv(nsfnet, 4, load=50, groups=[0, 1, 2], **kw)
    with pytest.raises(ValueError):
        BatchedRMSAEnv(nsfnet, 4, load=50, groups=[0, 1, 2, 3], num_groups=2, **kw)
    with pytest.raises(ValueError):
        BatchedRMSAEnv(nsfnet, 4, load=50, num_groups=2, **kw)
    with pytest.raises(ValueError):
        BatchedDeepRMSAEnv(nsfnet, 4, mean_service_inter_arrival_time=[0.1, 0.2])
    us14, tables = load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3")
    with pytest.raises(ValueError):
        BatchedPhyRMSAEnv(us14, 4, modulation_level=tables[1], connections_detail=tables[0], gsnr=tables[2],
                          load=[1400, 2400], mean_service_holding_time=25)
    with pytest.raises(ValueError):
        make_sweep("rmsa", nsfnet, loads=[20, -5], seeds_per_load=2, **kw)
    with pytest.raises(ValueError):
        make_sweep("nope", nsfnet, loads=[20], seeds_per_load=2, **kw)
    # valid arguments reach the library
    with pytest.raises(AssertionError, match="library was loaded"):
        BatchedRMSAEnv(nsfnet, 4, load=[50, 60, 70, 80], **kw)


def test_monitor_tree_layout(tmp_path):
    """Synthetic rows of 3 groups: the reference's tree (tests/test_rmsa_threads_us.py:149), header and columns of
    write_monitor_csv, rows in (episode, environment-of-the-group) order."""
    from optical_rl_gym_amd import write_monitor_csv, write_monitor_tree
    from optical_rl_gym_amd.monitor import RMSA_INFO_KEYWORDS
    groups = np.array([2, 0, 1, 0, 2, 2], np.int32)     # scrambled, unequal sizes
    loads = [1200.0, 1280.5, 1360.0]
    B, episodes, L = len(groups), 3, 200
    rows = []
    for ep in range(episodes):
        for i in range(B):
            row = {"r": float(100 * ep + i), "l": L - 1, "t": 0.5 * (ep + 1)}
            row.update({k: (ep + 1) / (i + 2) / (q + 1) for q, k in enumerate(RMSA_INFO_KEYWORDS)})
            rows.append(row)
    paths = write_monitor_tree(str(tmp_path), "sap_ff", rows, groups, loads, L, "RMSA-v0", RMSA_INFO_KEYWORDS, t_start=1.0)
    assert paths == [os.path.join(str(tmp_path), d, "sap_ff.monitor.csv") for d in ("logs_1200_200", "logs_1280.5_200", "logs_1360_200")]
    ref = tmp_path / "one.csv"
    write_monitor_csv(str(ref), rows[:1], "RMSA-v0", RMSA_INFO_KEYWORDS, t_start=1.0)
    ref_lines = ref.read_text().splitlines()
    for g, p in enumerate(paths):
        lines = open(p).read().splitlines()
        assert lines[0] == ref_lines[0] and lines[0].startswith('#{"t_start": 1.0, "env_id": "RMSA-v0"}')
        assert lines[1] == ref_lines[1] == "r,l,t," + ",".join(RMSA_INFO_KEYWORDS)
        members = np.flatnonzero(groups == g)
        assert len(lines) == 2 + episodes * len(members)
        want = [rows[ep * B + i] for ep in range(episodes) for i in members]
        for line, row in zip(lines[2:], want):
            cells = line.split(",")
            assert float(cells[0]) == row["r"] and int(cells[1]) == L - 1 and float(cells[2]) == row["t"]
            assert [float(c) for c in cells[3:]] == [row[k] for k in RMSA_INFO_KEYWORDS]
    with pytest.raises(ValueError):
        write_monitor_tree(str(tmp_path), "x", rows[:-1], groups, loads, L, "RMSA-v0", RMSA_INFO_KEYWORDS)
    with pytest.raises(ValueError):   # two groups of one load would share a file
        write_monitor_tree(str(tmp_path), "x", rows, groups, [1200.0, 1200.0, 1360.0], L, "RMSA-v0", RMSA_INFO_KEYWORDS)


def test_blocking_summary_is_the_per_env_statistic():
    """The grouped reduction's sums give mean and standard error of the per-environment blocking rates."""
    from optical_rl_gym_amd import traffic
    rng = np.random.default_rng(3)
    n, proc = 37, 1000                       # processed counts the pending request (decided: proc - 1)
    acc = rng.integers(600, 999, n)
    row = np.zeros((2, 16), np.int64)
    row[0, 2], row[0, 3], row[0, 9] = n * proc, acc.sum(), n
    row[0, 11] = ((proc - acc) ** 2).sum()
    mean, err = traffic.blocking_summary(row, episode=True)
    rates = (proc - 1 - acc) / (proc - 1)
    assert mean[0] == pytest.approx(rates.mean(), rel=1e-13)
    assert err[0] == pytest.approx(rates.std(ddof=1) / np.sqrt(n), rel=1e-10)
    assert np.isnan(mean[1]) and np.isnan(err[1])      # an empty group
