"""Per-environment traffic of a batched handle: load sweeps in one batch.

The reference's experiment scripts are load sweeps -- one process per (load, heuristic), ``range(1200, 1701, 80)`` in
``tests/test_rmsa_threads_us.py:57-60, 132-149``, every load on the same seed, one ``logs_{load}_{episode_length}`` folder
each.  Here the environments of ONE handle carry their own ``load`` / ``mean_service_holding_time`` and a group index (the
load they belong to); the counters come back per group (``reduce_counters(by_group=True)``).

Everything in this module is host arithmetic: importable and testable without a device or the library.
"""
from __future__ import annotations

import numpy as np

MAX_GROUPS = 256   # include/orlg.h: orlg_traffic::num_groups


def _per_env(name, value, batch_size):
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(batch_size, float(a), np.float64)
    if a.shape != (batch_size,):
        raise ValueError(f"{name}: shape {a.shape}, expected a scalar or ({batch_size},)")
    if not np.all(np.isfinite(a)) or not np.all(a > 0):
        raise ValueError(f"{name}: every value must be finite and positive")
    return np.ascontiguousarray(a)


def per_env_rates(batch_size, load, mean_service_holding_time):
    """(arrival_lambda [B], holding_lambda [B]) float64 for scalar or length-B ``load`` / ``mean_service_holding_time``,
    element by element the very operations the scalar constructors perform (``optical_network_env.py:111-129``,
    ``rmsa_env.py:646-651``): ``iat = 1 / (load / holding)``, ``arrival_lambda = 1 / iat``, ``holding_lambda = 1 / holding``
    -- IEEE double divisions, so the same bits as the Python floats of a scalar handle."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    load = _per_env("load", load, batch_size)
    holding = _per_env("mean_service_holding_time", mean_service_holding_time, batch_size)
    iat = 1 / (load / holding)
    arrival_lambda, holding_lambda = 1 / iat, 1 / holding
    if not (np.all(np.isfinite(arrival_lambda)) and np.all(arrival_lambda > 0) and np.all(np.isfinite(holding_lambda))
            and np.all(holding_lambda > 0)):
        raise ValueError("load / mean_service_holding_time give a rate that is not finite and positive")
    return arrival_lambda, holding_lambda


def check_groups(batch_size, groups, num_groups=None):
    """(group [B] int32, num_groups) of a ``groups=`` argument; ``None`` is one group."""
    batch_size = int(batch_size)
    if groups is None:
        if num_groups not in (None, 1):
            raise ValueError("num_groups without groups")
        return np.zeros(batch_size, np.int32), 1
    g = np.asarray(groups)
    if g.shape != (batch_size,):
        raise ValueError(f"groups: shape {g.shape}, expected ({batch_size},)")
    if g.dtype.kind not in "iu":
        raise TypeError(f"groups: dtype {g.dtype}, expected an integer type")
    n = int(g.max()) + 1 if num_groups is None else int(num_groups)
    if n < 1 or n > MAX_GROUPS:
        raise ValueError(f"num_groups {n} not in 1..{MAX_GROUPS}")
    if g.min() < 0 or g.max() >= n:
        raise ValueError(f"groups: every value must lie in 0..{n - 1}")
    return np.ascontiguousarray(g, dtype=np.int32), n


def load_sweep(loads, seeds_per_load, seed=None):
    """(load [B] float64, seeds [B] uint64, group [B] int32) of a sweep, ``B = len(loads) * seeds_per_load``, group-major:
    environment ``g * seeds_per_load + r`` runs ``loads[g]`` on seed ``base + r`` (``base`` = ``seed``, 41 when ``None``:
    ``optical_network_env.py:266-271``).  Every load runs on the SAME seeds -- common random numbers, as the reference's
    scripts use one seed for every load."""
    loads = np.asarray(loads, dtype=np.float64)
    if loads.ndim != 1 or loads.size < 1:
        raise ValueError("loads: a non-empty one-dimensional sequence")
    if loads.size > MAX_GROUPS:
        raise ValueError(f"loads: at most {MAX_GROUPS} loads in one handle")
    if not np.all(np.isfinite(loads)) or not np.all(loads > 0):
        raise ValueError("loads: every value must be finite and positive")
    n = int(seeds_per_load)
    if n < 1 or n != seeds_per_load:
        raise ValueError("seeds_per_load must be a positive integer")
    base = 41 if seed is None else int(seed)
    if base < 0:
        raise ValueError("seed must be >= 0")
    load = np.repeat(loads, n)
    seeds = np.tile(np.arange(n, dtype=np.uint64) + np.uint64(base), loads.size)
    group = np.repeat(np.arange(loads.size, dtype=np.int32), n)
    return load, seeds, group


def group_loads(loads, groups, num_groups):
    """The load of every group, [num_groups] float64 (NaN for an empty group).  ``ValueError`` when a group holds environments
    of different loads: it then has no load to be named after."""
    loads, groups = np.asarray(loads, np.float64), np.asarray(groups)
    out = np.full(int(num_groups), np.nan)
    for g in range(int(num_groups)):
        mine = loads[groups == g]
        if mine.size:
            if not np.all(mine == mine[0]):
                raise ValueError(f"group {g} holds environments of different loads ({mine.min():g} .. {mine.max():g})")
            out[g] = mine[0]
    return out


def blocking_rates(counters, pending_bit_rate):
    """The four blocking rates of the info dict from the counters of ``counters()`` as they stand after a step.  The
    reference builds info BEFORE ``_next_service()`` (``rmsa_env.py:293-335``, ``phy_rmsa_env.py:319-351``); the device step
    has already generated the next request, so the pending request (one service, ``pending_bit_rate``) is taken out of the
    request-side counters again.  Python ints give the reference's own int / int true divisions, int64 arrays the same
    element by element."""
    c = counters
    proc, eproc = c["services_processed"] - 1, c["episode_services_processed"] - 1
    req, ereq = c["bit_rate_requested"] - pending_bit_rate, c["episode_bit_rate_requested"] - pending_bit_rate
    return {"service_blocking_rate": (proc - c["services_accepted"]) / proc,
            "episode_service_blocking_rate": (eproc - c["episode_services_accepted"]) / eproc,
            "bit_rate_blocking_rate": (req - c["bit_rate_provisioned"]) / req,
            "episode_bit_rate_blocking_rate": (ereq - c["episode_bit_rate_provisioned"]) / ereq}


def blocking_summary(grouped, episode=True):
    """Mean service blocking rate per group and its standard error over the group's environments, from one result of
    ``reduce_counters(by_group=True)`` ([G, 16] int64) taken when an episode has just ended -- every environment of a handle
    (all share ``episode_length`` and are stepped together) has processed the same number of services, the last of them the pending request no step has decided yet, which the
    info dict of the reference does not count.  Columns: ``episode=True`` 2, 3, 11, else 0, 1, 10 (include/orlg.h).
    Exact integer sums; only the final quotients are floats.  Returns (mean [G], stderr [G]); NaN where a group is empty
    (stderr also where it has one environment)."""
    a = np.asarray(grouped, dtype=np.int64)
    p, q, s = (2, 3, 11) if episode else (0, 1, 10)
    G = a.shape[0]
    mean, err = np.full(G, np.nan), np.full(G, np.nan)
    for g in range(G):
        n = int(a[g, 9])
        if n < 1:
            continue
        proc = int(a[g, p]) // n - 1                  # decided services per environment
        d1, d2 = int(a[g, p]) - int(a[g, q]), int(a[g, s])   # sums of (processed - accepted) and of its square
        b1, b2 = d1 - n, d2 - 2 * d1 + n              # ... of blocked = processed - accepted - 1
        if proc < 1:
            continue
        mean[g] = b1 / (n * proc)
        if n > 1:
            var = (b2 - b1 * b1 / n) / (n - 1)
            err[g] = np.sqrt(max(var, 0.0) / n) / proc
    return mean, err


def blocking_shares_by_group(cause_counts, groups, num_groups=None, loads=None):
    """Blocking by cause of a load sweep, from the ``"block_cause_counts"`` of one or more launches of a sweep handle
    (``BatchedRMSAEnv.run(..., cause_counts=True)``; sum the arrays of several launches before the call).

    ``cause_counts`` [B, 8] integers, ``groups`` [B] the group of every environment (the handle's ``groups``).  Returns a dict:
    ``counts`` [G, 8] int64, the steps per group and cause (columns: ``BLOCK_CAUSES``, include/orlg.h ``ORLG_CAUSE_*``);
    ``steps`` [G]; ``shares`` [G, 8] float64 = counts / steps, so ``1 - shares[:, 0]`` is the blocking probability and
    ``shares[:, 1:]`` splits it by cause (NaN for a group without a step); ``loads`` [G] where ``loads`` [B] is given and
    every group is one load (:func:`group_loads`; ``ValueError`` otherwise)."""
    c = np.asarray(cause_counts)
    if c.ndim != 2 or c.shape[1] != 8:
        raise ValueError(f"cause_counts: shape {c.shape}, expected (B, 8)")
    if c.dtype.kind not in "iu":
        raise TypeError(f"cause_counts: dtype {c.dtype}, expected an integer type")
    g, n = check_groups(c.shape[0], groups, num_groups)
    counts = np.zeros((n, 8), np.int64)
    np.add.at(counts, g, c.astype(np.int64))
    steps = counts.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        shares = counts / steps[:, None].astype(np.float64)
    out = dict(counts=counts, steps=steps, shares=shares)
    if loads is not None:
        out["loads"] = group_loads(_per_env("loads", loads, c.shape[0]), g, n)
    return out
