"""Batched counterpart of ``utils.evaluate_heuristic`` (``utils.py:124-162``) and a writer for the
``stable_baselines3.Monitor`` CSV layout the reference's result folders use
(``examples/phy_frag_rmsa/us-results/logs_1400_200/*.monitor.csv``: a ``#{"t_start": ..., "env_id": ...}`` JSON header
line, then ``r,l,t,<info keywords>`` with one row per episode), so that ``examples/visualize_loads*.ipynb`` can read
results produced on the GPU.
"""
from __future__ import annotations

import json
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import traffic as _traffic

RMSA_INFO_KEYWORDS = ("episode_service_blocking_rate", "service_blocking_rate", "episode_bit_rate_blocking_rate",
                      "bit_rate_blocking_rate")


def write_monitor_csv(path: str, rows: Sequence[Dict], env_id: str, info_keywords: Sequence[str],
                      t_start: Optional[float] = None):
    """``rows``: dicts with r, l, t and the info keywords, one per episode."""
    with open(path, "w") as f:
        f.write("#" + json.dumps({"t_start": time.time() if t_start is None else t_start, "env_id": env_id}) + "\n")
        f.write(",".join(("r", "l", "t") + tuple(info_keywords)) + "\n")
        for row in rows:
            f.write(",".join(repr(float(row[k])) if isinstance(row[k], (float, np.floating)) else str(row[k])
                             for k in ("r", "l", "t") + tuple(info_keywords)) + "\n")


def monitor_tree_path(monitor_dir: str, load, episode_length: int, monitor_name: str) -> str:
    """``{monitor_dir}/logs_{load}_{episode_length}/{monitor_name}.monitor.csv``: the tree of the reference's sweep scripts
    (``tests/test_rmsa_threads_us.py:149``, ``log_dir = "./.../logs_{}_{}/".format(load, episode_length)``)."""
    return os.path.join(monitor_dir, f"logs_{load:g}_{int(episode_length)}", f"{monitor_name}.monitor.csv")


def write_monitor_tree(monitor_dir: str, monitor_name: str, rows: Sequence[Dict], groups, group_loads, episode_length: int,
                       env_id: str, info_keywords: Sequence[str], t_start: Optional[float] = None) -> List[str]:
    """One Monitor CSV per group (= load) of a sweep.  ``rows`` are the rows of :func:`write_monitor_csv` in (episode,
    environment) order for a batch of ``len(groups)`` environments; a group's file keeps that order -- (episode,
    environment-of-the-group).  ``group_loads[g]`` names the folder of group ``g``.  Returns the paths by group (groups
    without environments write nothing and are left out)."""
    groups = np.asarray(groups)
    B = groups.shape[0]
    if B < 1 or len(rows) % B:
        raise ValueError(f"{len(rows)} rows are not whole episodes of {B} environments")
    paths = []
    for g in range(len(group_loads)):
        members = np.flatnonzero(groups == g)
        if members.size == 0:
            continue
        path = monitor_tree_path(monitor_dir, float(group_loads[g]), episode_length, monitor_name)
        if path in paths:
            raise ValueError(f"groups with the same load {group_loads[g]:g} would share {path}")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        mine = [rows[ep * B + int(i)] for ep in range(len(rows) // B) for i in members]
        write_monitor_csv(path, mine, env_id, info_keywords, t_start=t_start)
        paths.append(path)
    return paths


def _by_group_summary(env, grouped: Sequence[np.ndarray]):
    """``by_group`` of the evaluate functions from the grouped reductions taken at the end of every episode."""
    ep = [_traffic.blocking_summary(a, episode=True) for a in grouped]
    al = [_traffic.blocking_summary(a, episode=False) for a in grouped]
    return {"load": _traffic.group_loads(env.loads, env.groups, env.num_groups),
            "num_envs": np.asarray(grouped[0])[:, 9].copy() if grouped else np.zeros(env.num_groups, np.int64),
            "episode_service_blocking_rate": np.stack([m for m, _ in ep]),
            "episode_service_blocking_rate_stderr": np.stack([e for _, e in ep]),
            "service_blocking_rate": np.stack([m for m, _ in al]),
            "service_blocking_rate_stderr": np.stack([e for _, e in al]),
            "counters": np.stack([np.asarray(a) for a in grouped])}


class _Evaluation:
    """What the two evaluate functions share around their episode loops: the check of the groups, the rows of the Monitor
    CSV, the three writers and the return value."""

    def __init__(self, env, info_keywords, monitor_dir, by_group):
        self.env, self.info_keywords, self.by_group = env, info_keywords, by_group
        if monitor_dir is not None or by_group:
            _traffic.group_loads(env.loads, env.groups, env.num_groups)   # (every group one load, before anything runs)
        self.t0 = time.time()
        self.grouped, self.rewards, self.lengths, self.rows = [], [], [], []
        self.infos: Dict[str, List[np.ndarray]] = {k: [] for k in info_keywords}

    def end_of_episode(self):
        """The four blocking rates [B] when an episode has just ended: the Monitor logs the info of the episode's last step,
        built before the next request is generated.  With ``by_group`` the grouped reduction of this moment is kept too."""
        env = self.env
        c = env.counters()
        if self.by_group:
            self.grouped.append(env.reduce_counters(by_group=True))
        return _traffic.blocking_rates(c, env.requests()["bit_rate"].astype(np.int64))

    def add_episode(self, ep_r, ep_l, vals):
        """One row per environment; integer-valued info columns are written as integers."""
        t = time.time() - self.t0
        self.rewards.append(ep_r.copy()); self.lengths.append(ep_l.copy())
        for k in self.info_keywords:
            self.infos[k].append(np.asarray(vals[k]))
        for i in range(self.env.batch_size):
            row = {"r": float(ep_r[i]), "l": int(ep_l[i]), "t": round(t, 6)}
            row.update({k: (int(vals[k][i]) if np.issubdtype(np.asarray(vals[k]).dtype, np.integer) else float(vals[k][i]))
                        for k in self.info_keywords})
            self.rows.append(row)

    def finish(self, env_id, monitor_path, monitor_dir, monitor_name):
        env = self.env
        if monitor_path is not None:
            write_monitor_csv(monitor_path, self.rows, env_id, self.info_keywords, t_start=self.t0)
        if monitor_dir is not None:
            write_monitor_tree(monitor_dir, monitor_name, self.rows, env.groups,
                               _traffic.group_loads(env.loads, env.groups, env.num_groups), env.episode_length, env_id,
                               self.info_keywords, t_start=self.t0)
        out = np.stack(self.rewards), np.stack(self.lengths), {k: np.stack(v) for k, v in self.infos.items()}
        return out + (_by_group_summary(env, self.grouped),) if self.by_group else out


def evaluate_heuristic_batched(env, policy: str, n_eval_episodes: int = 10, monitor_path: Optional[str] = None,
                               env_id: str = "RMSA-v0", info_keywords: Sequence[str] = RMSA_INFO_KEYWORDS,
                               chunk: int = 1000, monitor_dir: Optional[str] = None, monitor_name: Optional[str] = None,
                               by_group: bool = False, gn_rule=None):
    """Run ``n_eval_episodes`` episodes of ``policy`` on every env of a :class:`BatchedRMSAEnv` with the reference
    loop's semantics: ``env.reset()`` (episode counters only) before every episode, step until ``done``.  Returns
    (episode_rewards [episodes, B], episode_lengths [episodes, B], per-episode info arrays); optionally writes one
    Monitor CSV with the rows of env 0, then env 1, ... per episode.

    ``monitor_dir``: one file per group of the handle (a load sweep, ``traffic.load_sweep``) in the reference's tree,
    ``{monitor_dir}/logs_{load:g}_{episode_length}/{monitor_name}.monitor.csv`` (``monitor_name`` defaults to ``policy``).
    ``by_group=True`` adds a fourth return value (whatever the output paths): per group its load and, [episodes, G] each, the
    mean blocking rates with their standard error over the group's seeds, formed from ``reduce_counters(by_group=True)``.
    Both need every group to be one load (``ValueError`` otherwise).  ``gn_rule``: passed on to ``env.run`` (an assignment rule
    behind the GN-model admission check of a ``gn_gate=`` handle)."""
    B = env.batch_size
    ev = _Evaluation(env, info_keywords, monitor_dir, by_group)
    kw = {} if gn_rule is None else {"gn_rule": gn_rule}
    for _ in range(n_eval_episodes):
        env.reset(only_episode_counters=True)
        ep_r = np.zeros(B)
        ep_l = np.zeros(B, np.int64)
        active = np.ones(B, bool)
        # the pending request is already counted, so an episode is episode_length - 1 steps; all envs of
        # a batch share the episode length and therefore finish together
        left = env.episode_length - 1
        while left > 0:
            n = min(left, chunk)
            out = env.run(policy, n, outputs=("reward", "done"), **kw)
            ep_r += out["reward"].sum(axis=0)
            ep_l += n
            left -= n
            active &= ~out["done"][-1].astype(bool)
        assert not active.any(), "episode did not finish on every env"
        ev.add_episode(ep_r, ep_l, ev.end_of_episode())
    return ev.finish(env_id, monitor_path, monitor_dir, monitor_name or policy)


# tests/test_rmsa_threads_us.py:66-69 (the Monitor the reference wraps PhyRMSA-v0 in)
PHY_INFO_KEYWORDS = ("episode_service_blocking_rate", "service_blocking_rate", "episode_bit_rate_blocking_rate",
                     "number_cuts_total", "rss_total_metric", "total_path_length", "num_moves", "num_defrag_cycle",
                     "avrage_gsnr", "average_mod_level", "average_path_index", "path_index", "physical_paths",
                     "num_moves_groom")


def evaluate_phy_heuristic_batched(env, policy: str, n_eval_episodes: int = 10, monitor_path: Optional[str] = None,
                                   env_id: str = "PhyRMSA-v0", info_keywords: Sequence[str] = PHY_INFO_KEYWORDS,
                                   chunk: int = 1000, monitor_dir: Optional[str] = None, monitor_name: Optional[str] = None,
                                   by_group: bool = False):
    """``evaluate_heuristic(env, heuristic, n_eval_episodes)`` (``utils.py:124-162``) for every env of a
    :class:`BatchedPhyRMSAEnv` with a device policy, and the Monitor CSV of the reference's experiment scripts
    (``tests/test_rmsa_threads_us.py:56-126``): one row per episode with the info dict of the episode's LAST step
    (``phy_rmsa_env.py:319-348``).  ``average_mod_level`` is the true mean (the reference's accumulator wraps at 256 under
    NumPy >= 2, SURVEY 8c caveat 2).  Returns (episode_rewards [episodes, B], episode_lengths, info arrays).
    ``monitor_dir`` / ``monitor_name`` / ``by_group``: the per-load tree and the summary, as :func:`evaluate_heuristic_batched`."""
    B = env.batch_size
    ev = _Evaluation(env, info_keywords, monitor_dir, by_group)
    last_outs = ("accepted", "done", "number_cuts_total", "rss_total_metric", "defrag_counters")
    for _ in range(n_eval_episodes):
        env.reset(only_episode_counters=True)
        ep_r = np.zeros(B)
        left = env.episode_length - 1      # the pending request is already counted
        while left > 1:
            n = min(left - 1, chunk)
            ep_r += env.run(policy, n, outputs=("accepted",))["accepted"].sum(axis=0)
            left -= n
        last = env.run(policy, 1, outputs=last_outs)
        ep_r += last["accepted"][0]
        assert last["done"][0].all(), "episode did not finish on every env"
        vals = ev.end_of_episode()
        dc = last["defrag_counters"][0].astype(np.int64)
        vals.update({"number_cuts_total": last["number_cuts_total"][0], "rss_total_metric": last["rss_total_metric"][0],
                     "num_moves": dc[:, 0] / 2 + dc[:, 1], "num_moves_groom": dc[:, 1], "num_defrag_cycle": dc[:, 2]})
        vals.update(env.info())   # the per-episode ratios of the info dict (phy_rmsa_env.py:339-347)
        ev.add_episode(ep_r, np.full(B, env.episode_length - 1, np.int64), vals)
    return ev.finish(env_id, monitor_path, monitor_dir, monitor_name or policy)
