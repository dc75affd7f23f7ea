"""Valid-action masks for the whole batch (include/orlg.h: orlg_deeprmsa_observation_masked, orlg_action_masks,
orlg_phy_channel_masks): mask[a] = 1 iff the reference's step(a) on the pending request would accept the service.  Every
comparison is exact -- integers and bits, no tolerance: against the oracle step by step, against the outcome of the step itself,
fused launch against separate launch, batched against the single-environment views."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import (DEEPRMSA_NODE_PROBS, deeprmsa_to_rmsa_kwargs, load_golden, load_phy_tables, load_topology,
                      oracle_env_from_kwargs, phy_oracle_from_kwargs)
from gpu_support import check_against_oracles, device_log_fixture, phy_env, unpack  # noqa: F401

pytestmark = pytest.mark.gpu

NSFNET = "nsfnet_chen_5-paths_6-modulations"
RMSA_NSFNET_320 = dict(num_spectrum_resources=320, load=50, mean_service_holding_time=25, episode_length=1000, seed=10)
CONFIG4 = dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, num_spectrum_resources=320,
               node_request_probabilities=DEEPRMSA_NODE_PROBS, episode_length=50)


def _case(name):
    """(topology, device class name, device kwargs, oracle kwargs, j, reward mode, device policy, external policy)"""
    if name == "rmsa_nsfnet_320_load50":
        return load_topology(NSFNET), "BatchedRMSAEnv", dict(RMSA_NSFNET_320), dict(RMSA_NSFNET_320), 1, 0, "sap_ff", "external"
    _, meta = load_golden(name)
    kw = dict(meta["env_kwargs"])
    okw, j = deeprmsa_to_rmsa_kwargs(kw)
    return load_topology(meta["topology"]), "BatchedDeepRMSAEnv", kw, okw, j, 1, "deeprmsa_sap_ff", "deeprmsa_external"


@pytest.mark.parametrize("step_kernel", ["wave", "group"])
@pytest.mark.parametrize("name,allow_rejection", [("deeprmsa_nsfnet_s4_random_j3", False), ("deeprmsa_jpn12_s6_random_j2", False),
                                                  ("deeprmsa_nsfnet_s10_sapff_320_config4", False),
                                                  ("rmsa_nsfnet_320_load50", False), ("deeprmsa_nsfnet_s4_random_j3", True)])
def test_masks_against_the_oracle_step_by_step(name, allow_rejection, step_kernel, device_log_in_oracle):
    import optical_rl_gym_amd as pkg
    topo, cls, kw, okw, j, reward_mode, policy, ext = _case(name)
    kw["allow_rejection"] = allow_rejection
    batch, n_policy, n_ext = 4, 200, 120
    env = getattr(pkg, cls)(topo, batch, step_kernel=step_kernel, **kw)
    oracles = [oracle_env_from_kwargs(topo, okw, seed=okw["seed"] + i, j=j, reward_mode=reward_mode) for i in range(batch)]
    K, S = env.k_paths, env.num_spectrum_resources
    rng = np.random.default_rng(17)
    seen = np.zeros(2, np.int64)
    check_against_oracles(env, oracles, "start")
    for t in range(n_policy + n_ext):
        deep, ff, bits = check_against_oracles(env, oracles, t) if t else (None, None, None)
        if t < n_policy:
            r = env.run(policy, 1, auto_reset=True, outputs=("accepted",))
            for i, o in enumerate(oracles):
                ot = o.run(policy, 1, reset_on_done=True)
                assert r["accepted"][0, i] == ot["accepted"][0], (t, i)
            continue
        # external random actions, so that fragmented states occur: DeepRMSA -- any action; RMSA -- a random path and a random
        # valid start of it (or slot 0 when it has none), i.e. services land in the middle of free runs
        if ext == "deeprmsa_external":
            a = rng.integers(0, K * j + 1, batch).astype(np.int32)
            expect = np.array([a[i] < K * j and deep[i, a[i]] == 1 for i in range(batch)])
        else:
            a = np.zeros((batch, 2), np.int32)
            for i in range(batch):
                p = int(rng.integers(0, K))
                ok = np.flatnonzero(bits[i, p])
                a[i] = (p, int(rng.choice(ok)) if ok.size and rng.random() < 0.9 else int(rng.integers(0, S)))
            expect = np.array([bits[i, a[i, 0], a[i, 1]] == 1 for i in range(batch)])
        r = env.run(ext, 1, actions=a, auto_reset=True, outputs=("accepted",))
        assert np.array_equal(r["accepted"][0].astype(bool), expect), (t, a, r["accepted"][0], expect)   # mask == outcome
        seen[0] += int((~expect).sum()); seen[1] += int(expect.sum())
        for i, o in enumerate(oracles):
            ot = o.run(ext, 1, reset_on_done=True, actions=a[i:i + 1].copy())
            assert r["accepted"][0, i] == ot["accepted"][0], (t, i)
    check_against_oracles(env, oracles, "end")
    assert seen.min() > 0, seen
    for o in oracles:
        o.close()
    env.close()


def test_first_fit_bound_quirk_constructed(device_log_in_oracle):
    """A state, built by external actions on a short spectrum, in which a path's only fit starts at S - n: RMSAEnv.step accepts
    that start, the first-fit loops (range(0, S - n)) never try it.  slots bit set, path_ff 0, step_path_first_fit rejects,
    step([p, S - n]) accepts."""
    from optical_rl_gym_amd import BatchedRMSAEnv
    topo = load_topology(NSFNET)
    S = 16
    # services that practically never leave (holding ~1e6 against one arrival per time unit): the spectrum only fills
    kw = dict(num_spectrum_resources=S, load=1e6, mean_service_holding_time=1e6, episode_length=100000, seed=3,
              bit_rates=[25, 50, 100], queue_capacity=1024)
    env = BatchedRMSAEnv(topo, 1, **kw)
    okw = {k: v for k, v in kw.items() if k != "queue_capacity"}
    o = oracle_env_from_kwargs(topo, okw, seed=3)
    K = env.k_paths
    rng = np.random.default_rng(2)
    found = 0
    for t in range(600):
        ff, bits = env.action_masks("path_ff")[0], unpack(env.action_masks("slots")[0], S)
        _, nslots = env.path_masks(0)
        hit = [p for p in range(K) if bits[p].sum() == 1 and bits[p, S - nslots[p]] == 1]
        if hit:
            p = hit[0]
            n = int(nslots[p])
            assert n == o.number_slots(p) and o.is_path_free(p, S - n, n)
            assert not any(o.is_path_free(p, s, n) for s in range(0, S - n))
            assert ff[p] == 0                                                     # the only fit is the one first fit never tries
            snap = env.save_state()
            r = env.step_path_first_fit(np.array([p], np.int32))
            assert r["accepted"][0] == 0
            env.load_state(snap)
            r = env.step(np.array([[p, S - n]], np.int32))
            assert r["accepted"][0] == 1
            ot = o.run("external", 1, actions=np.array([[p, S - n]], np.int32))
            assert ot["accepted"][0] == 1
            found += 1
            if found == 3:
                break
            continue
        # fill from the bottom: a random path that has a fit, at its lowest valid start
        cands = [p for p in range(K) if bits[p].any()]
        a = np.array([[K, S]], np.int32)
        if cands:
            p = int(rng.choice(cands))
            a = np.array([[p, int(np.flatnonzero(bits[p])[0])]], np.int32)
        r = env.step(a)
        ot = o.run("external", 1, actions=a.copy())
        assert r["accepted"][0] == ot["accepted"][0] == (1 if cands else 0), t
    assert found == 3, found
    o.close()
    env.close()


def test_block_at_slot_zero_quirk_constructed(device_log_in_oracle):
    """A DeepRMSA block that starts at slot 0 encodes its start as 2 (0 - S/2) / S = -1 in the observation -- the value that
    also stands for "no such block".  The mask tells them apart."""
    from optical_rl_gym_amd import BatchedDeepRMSAEnv
    topo = load_topology(NSFNET)
    S, J = 64, 2
    kw = dict(j=J, num_spectrum_resources=S, mean_service_holding_time=1e6, mean_service_inter_arrival_time=1.0,
              episode_length=100000, seed=5, queue_capacity=1024)
    env = BatchedDeepRMSAEnv(topo, 1, **kw)
    okw, j = deeprmsa_to_rmsa_kwargs({k: v for k, v in kw.items() if k != "queue_capacity"})
    o = oracle_env_from_kwargs(topo, okw, seed=5, j=j, reward_mode=1)
    K, N = env.k_paths, topo.num_nodes
    PW, head = 2 * J + 3, 1 + 2 * N
    both = 0
    for t in range(40):
        obs, mask = env.observation(return_mask=True)
        assert np.array_equal(obs[0], o.observation())
        for p in range(K):
            starts, _ = o.available_blocks(p)
            for b in range(J):
                feat = obs[0, head + p * PW + 2 * b]
                assert mask[0, p * J + b] == (b < len(starts))
                if b < len(starts) and starts[b] == 0:
                    assert feat == -1.0 and mask[0, p * J + b] == 1       # a block at slot 0: valid, start feature -1
                    both |= 1
                if b >= len(starts):
                    assert feat == -1.0 and mask[0, p * J + b] == 0       # no block: invalid, start feature -1 as well
                    both |= 2
        # take the LAST block of a path (its second run, if it has one): leaves a block at slot 0 and splits the spectrum
        a = np.array([(t % K) * J + (J - 1 if t % 3 else 0)], np.int32)
        r = env.step_deeprmsa(a)
        ot = o.run("deeprmsa_external", 1, actions=a.copy())
        assert r["accepted"][0] == ot["accepted"][0]
    assert both == 3
    o.close()
    env.close()


@pytest.mark.parametrize("step_kernel", ["wave", "group"])
def test_mask_equals_outcome_at_scale(step_kernel):
    """B = 4096, NSFNET S = 320, j = 3, after 300 SAP-FF steps: for every action the step accepts exactly where the mask is 1.
    Every action column must hold both values, at least 1 % of each, so that the test cannot pass vacuously.

    The load is 14 Erlang (holding 7.5, inter-arrival 7.5 / 14), not configs[3]'s 90: third blocks of the longer paths are scarce
    at high load.  Chosen from the CPU oracle, 1000 seeds x 300 deeprmsa_sap_ff steps, smallest / largest valid fraction over
    the 15 action columns: load 90 -- 0.000 / 0.58 (on the device at B = 4096: 0.0017 / 0.545, three columns under 1 %);
    30 -- 0.015 / 0.80; 20 -- 0.019 / 0.86; 16 -- 0.022 / 0.92; 12 -- 0.024 / 0.96; 8 -- 0.011 / 0.988.  At 12 .. 16 the
    scarcest column is more than five standard deviations of a B = 4096 sample (0.23 %) above 1 % and the fullest as far below
    99 %."""
    from optical_rl_gym_amd import BatchedDeepRMSAEnv
    topo = load_topology(NSFNET)
    B, J = 4096, 3
    env = BatchedDeepRMSAEnv(topo, B, j=J, seed=1000, step_kernel=step_kernel,
                             **dict(CONFIG4, mean_service_inter_arrival_time=7.5 / 14.0))
    env.run("deeprmsa_sap_ff", 300, auto_reset=True)
    K = env.k_paths
    snap = env.save_state()
    obs, mask = env.observation(return_mask=True)
    ff = env.action_masks("path_ff")
    assert mask.shape == (B, K * J) and ff.shape == (B, K)
    print("deeprmsa mask, fraction valid per action:", np.round(mask.mean(axis=0), 4))
    print("path_ff mask, fraction valid per path:", np.round(ff.mean(axis=0), 4))
    for a in range(K * J):
        r = env.step_deeprmsa(np.full(B, a, np.int32), outputs=("accepted",))
        assert np.array_equal(r["accepted"], mask[:, a]), (a, int((r["accepted"] != mask[:, a]).sum()))
        env.load_state(snap)
    for p in range(K):
        r = env.step_path_first_fit(np.full(B, p, np.int32), outputs=("accepted",))
        assert np.array_equal(r["accepted"], ff[:, p]), (p, int((r["accepted"] != ff[:, p]).sum()))
        env.load_state(snap)
    # masks of a loaded state == masks of the state the step kernel left
    assert np.array_equal(env.action_masks("deeprmsa"), mask) and np.array_equal(env.action_masks("path_ff"), ff)
    for name, m in (("deeprmsa", mask), ("path_ff", ff)):
        frac = m.mean(axis=0)
        assert np.all(frac >= 0.01) and np.all(frac <= 0.99), (name, frac)
    env.close()


def test_fused_equals_separate_b32768():
    """The observation of the masked call == the observation of the existing entries byte for byte (f64, f32); the mask of the
    fused call == action_masks("deeprmsa") into pageable, pinned and device buffers.  B = 32 768 with torch device tensors, in a
    child process: torch has to create its HIP context before the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        sys.path[:0] = [%r, %r]
        from conftest import DEEPRMSA_NODE_PROBS, load_topology
        from optical_rl_gym_amd import BatchedDeepRMSAEnv
        B = 32768
        for j, reject in ((1, False), (3, True)):
            env = BatchedDeepRMSAEnv(load_topology("nsfnet_chen_5-paths_6-modulations"), B, num_spectrum_resources=320, j=j,
                                     mean_service_holding_time=7.5, mean_service_inter_arrival_time=1 / 12.0,
                                     node_request_probabilities=DEEPRMSA_NODE_PROBS, episode_length=50, seed=3,
                                     allow_rejection=reject)
            env.run("deeprmsa_sap_ff", 150, auto_reset=True)
            D, M = env.obs_dim, env.k_paths * j + int(reject)
            assert env.mask_dim == M
            ref64, ref32 = env.observation(), env.observation(dtype=np.float32)
            # pageable host buffers
            o64, m_a = env.observation(return_mask=True)
            o32, m_b = env.observation(dtype=np.float32, return_mask=True)
            assert o64.dtype == np.float64 and o32.dtype == np.float32 and m_a.dtype == np.uint8 and m_a.shape == (B, M)
            assert o64.tobytes() == ref64.tobytes() and o32.tobytes() == ref32.tobytes()
            sep = env.action_masks("deeprmsa")
            assert np.array_equal(m_a, sep) and np.array_equal(m_b, sep)
            assert 0 < sep[:, :env.k_paths * j].mean() < 1
            if reject:
                assert np.all(sep[:, -1] == 1)
            # device tensors: observation and mask written in place by one launch
            t64 = torch.full((B, D), 7.0, dtype=torch.float64, device="cuda")
            t32 = torch.full((B, D), 7.0, dtype=torch.float32, device="cuda")
            tm1 = torch.full((B, M), 9, dtype=torch.uint8, device="cuda")
            tm2 = torch.full((B, M), 9, dtype=torch.uint8, device="cuda")
            tms = torch.full((B, M), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r = env.observation(out=t64, mask_out=tm1)
            assert r[0] is t64 and r[1] is tm1
            env.observation(out=t32, mask_out=tm2)
            assert env.action_masks("deeprmsa", out=tms) is tms
            env.synchronize()
            assert t64.cpu().numpy().tobytes() == ref64.tobytes() and t32.cpu().numpy().tobytes() == ref32.tobytes()
            for t in (tm1, tm2, tms):
                assert np.array_equal(t.cpu().numpy(), sep)
            # pinned host buffers: written over the bus, the call does not wait
            p32 = torch.full((B, D), 7.0, dtype=torch.float32).pin_memory()
            pm, pms = torch.full((B, M), 9, dtype=torch.uint8).pin_memory(), torch.full((B, M), 9, dtype=torch.uint8).pin_memory()
            env.observation(out=p32, mask_out=pm)
            env.action_masks("deeprmsa", out=pms)
            env.synchronize()
            assert p32.numpy().tobytes() == ref32.tobytes() and np.array_equal(pm.numpy(), sep) and np.array_equal(pms.numpy(), sep)
            # mixed: device observation, pageable mask
            hm = np.full((B, M), 9, np.uint8)
            t32.fill_(7.0); torch.cuda.synchronize()
            env.observation(out=t32, mask_out=hm)
            env.synchronize()
            assert np.array_equal(hm, sep) and t32.cpu().numpy().tobytes() == ref32.tobytes()
            # the other two masks into device and pinned buffers == pageable
            for kind in ("path_ff", "slots"):
                h = env.action_masks(kind)
                shape, dt = env.action_mask_shape(kind)
                td = torch.zeros(shape, dtype=torch.uint8 if kind == "path_ff" else torch.int64, device="cuda")
                torch.cuda.synchronize()
                if kind == "slots":
                    with np.testing.assert_raises(TypeError):
                        env.action_masks(kind, out=td)                       # int64 is not uint64
                    td = td.view(torch.uint64)
                env.action_masks(kind, out=td)
                env.synchronize()
                got = td.view(torch.int64).cpu().numpy().view(np.uint64) if kind == "slots" else td.cpu().numpy()
                assert np.array_equal(got, h), kind
            env.close()
        print("fused masks ok")
    """) % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "fused masks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _expected_channel_bits(topo, av, src, dst):
    """AND over the links of each candidate path of (src, dst) of available_channels [E, C]"""
    base = int(topo.pair_path_base[src * topo.num_nodes + dst])
    rows = []
    for g in range(base, base + topo.k_paths):
        links = topo.path_links[topo.path_link_off[g]:topo.path_link_off[g + 1]]
        rows.append(np.all(av[links] != 0, axis=0))
    return np.stack(rows).astype(np.uint8)


@pytest.mark.parametrize("case", ["phy_us14_s10_bmfa", "phy_us14_s10_bmfa_groom", "phy_jpn12_s3_bmfa"])
def test_phy_channel_masks_against_the_oracle(case, device_log_in_oracle):
    """US14 load 1400 (grooming off and on) and JPN12, bmfa, 200 steps, 4 environments: channel_masks() == AND over each candidate
    path's links of PhyOracleEnv.available_channels(), after every step."""
    _, meta = load_golden(case)
    topo, tables, kw = load_topology(meta["topology"]), load_phy_tables(meta["tables"]), meta["env_kwargs"]
    if "us14" in case:
        assert kw["load"] == 1400
    batch, C = 4, 268
    env = phy_env(topo, tables, kw, batch)
    assert env.num_channels == C
    oracles = [phy_oracle_from_kwargs(topo, tables, kw, seed=kw["seed"] + i) for i in range(batch)]
    lit = 0
    for t in range(201):
        words = env.channel_masks()
        assert words.shape == (batch, topo.k_paths, env.words_per_link) and words.dtype == np.uint64
        bits = unpack(words, 64 * env.words_per_link)
        assert not bits[..., C:].any()
        for i, o in enumerate(oracles):
            q = o.request()
            want = _expected_channel_bits(topo, o.available_channels(), q.src, q.dst)
            assert np.array_equal(bits[i, :, :C], want), (t, i, np.nonzero(bits[i, :, :C] != want))
            lit += int((want == 0).sum())
        if t == 200:
            break
        r = env.run("bmfa", 1, auto_reset=True, outputs=("accepted",))
        for i, o in enumerate(oracles):
            ot = o.run("bmfa", 1, reset_on_done=True)
            assert r["accepted"][0, i] == ot["accepted"][0], (t, i)
    assert lit > 0
    for o in oracles:
        o.close()
    env.close()


def test_views_agree_with_the_batched_masks():
    """The four single-environment methods == the batched result for B = 1."""
    from optical_rl_gym_amd import DeepRMSAEnv, PathOnlyFirstFitAction, PhyRMSAEnv, RMSAEnv
    topo = load_topology(NSFNET)
    for reject in (False, True):
        d = DeepRMSAEnv(topology=topo, j=3, seed=7, allow_rejection=reject, **CONFIG4)
        for t in range(40):
            d.step(d.action_space.sample())
        m = d.action_masks()
        assert m.dtype == bool and m.shape == (d.action_space.n,) == (5 * 3 + int(reject),)
        assert np.array_equal(m, d._batched.action_masks("deeprmsa")[0].astype(bool))
        if reject:
            assert m[-1]
        d.close()
        e = RMSAEnv(topology=topo, allow_rejection=reject, **RMSA_NSFNET_320)
        w = PathOnlyFirstFitAction(e)
        for t in range(150):
            w.step(t % 5)
        S, k, r = 320, 5, int(reject)
        pm = w.action_masks()
        assert pm.dtype == bool and pm.shape == (k + r,)
        assert np.array_equal(pm, e._batched.action_masks("path_ff")[0].astype(bool))
        for p in range(k):
            assert pm[p] == (w.action(p) != (k, S))                                   # the reference's own loop, on the view
        sm = e.action_masks()
        assert sm.dtype == bool and sm.shape == (k + r, S + r)
        assert np.array_equal(sm[:k, :S], unpack(e._batched.action_masks("slots")[0], S).astype(bool))
        cands = e.k_shortest_paths[e.current_service.source, e.current_service.destination]
        for p in range(k):
            n = e.get_number_slots(cands[p])
            assert np.array_equal(sm[p, :S], [e.is_path_free(cands[p], s, n) for s in range(S)])
        if reject:
            assert sm[k, S] and sm[k].sum() == 1 and sm[:, S].sum() == 1
        e.close()
    _, meta = load_golden("phy_us14_s10_bmfa")
    pairs, mod, gsnr = load_phy_tables(meta["tables"])
    kw = {k: v for k, v in meta["env_kwargs"].items() if k not in ("num_spectrum_resources", "bit_rate_selection")}
    pe = PhyRMSAEnv(topology=load_topology(meta["topology"]), modulation_level=mod, connections_detail=pairs, gsnr=gsnr, **kw)
    pe._batched.run("bmfa", 150)
    pe._sync()
    cm = pe.channel_masks()
    assert cm.dtype == bool and cm.shape == (3, 268) and not cm.all() and cm.any()
    assert np.array_equal(cm, unpack(pe._batched.channel_masks()[0], 268).astype(bool))
    cands = pe.k_shortest_paths[pe.current_service.source, pe.current_service.destination]
    for p in range(3):
        assert np.array_equal(cm[p], [pe.is_channel_free(cands[p], c) for c in range(268)])
    pe.close()
