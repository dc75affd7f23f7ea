"""``make_sweep``: a load sweep as ONE batched handle (``traffic.load_sweep``)."""
from __future__ import annotations

from . import traffic

_KINDS = ("rmsa", "deeprmsa", "phy")


def make_sweep(kind: str, topology, *, loads, seeds_per_load: int, seed=None, **kwargs):
    """``len(loads) * seeds_per_load`` environments in one handle, group-major: every load on the seeds ``seed`` ..
    ``seed + seeds_per_load - 1``, group ``g`` = ``loads[g]``.  ``kind``: ``"rmsa"`` (:class:`BatchedRMSAEnv`),
    ``"deeprmsa"`` (:class:`BatchedDeepRMSAEnv`; the loads set ``mean_service_inter_arrival_time = holding / load``) or
    ``"phy"`` (:class:`BatchedPhyRMSAEnv`).  The other kwargs are the constructor's."""
    if kind not in _KINDS:
        raise ValueError(f"kind must be one of {_KINDS}, got {kind!r}")
    for k in ("load", "seeds", "groups", "num_groups", "batch_size"):
        if k in kwargs:
            raise ValueError(f"make_sweep sets {k} itself")
    load, seeds, group = traffic.load_sweep(loads, seeds_per_load, seed)
    common = dict(seed=seed, seeds=seeds, groups=group, num_groups=len(loads))
    if kind == "rmsa":
        from .batched import BatchedRMSAEnv
        return BatchedRMSAEnv(topology, load.size, load=load, **common, **kwargs)
    if kind == "phy":
        from .phy import BatchedPhyRMSAEnv
        return BatchedPhyRMSAEnv(topology, load.size, load=load, **common, **kwargs)
    from .batched import BatchedDeepRMSAEnv
    holding = float(kwargs.pop("mean_service_holding_time", 25.0))
    if "mean_service_inter_arrival_time" in kwargs:
        raise ValueError("make_sweep sets mean_service_inter_arrival_time itself")
    return BatchedDeepRMSAEnv(topology, load.size, mean_service_holding_time=holding,
                              mean_service_inter_arrival_time=holding / load, **common, **kwargs)
