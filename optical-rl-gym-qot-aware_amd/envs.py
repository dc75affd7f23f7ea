"""Single-environment gym-style views with the reference's object surface.

``RMSAEnv`` / ``DeepRMSAEnv`` here are drop-ins for ``optical_rl_gym.envs.rmsa_env.RMSAEnv`` and
``optical_rl_gym.envs.deeprmsa_env.DeepRMSAEnv``: same constructor kwargs, ``reset(only_episode_counters=True)``,
``step(action) -> (obs, reward, done, info)`` with the same ``info`` keys, and the attributes / query methods the
reference's heuristic callbacks ``f(env) -> action`` touch (``rmsa_env.py:854-937``, ``deeprmsa_env.py:135-155``).
The environment itself lives on the GPU (a :class:`BatchedRMSAEnv` of batch 1, or one row of a bigger batch);
every query is a read of device state through the C ABI (``orlg_query_path_masks`` computes the path-wide free
bitmaps on the device, this module only slices them).  There is no CPU simulation here.

The heuristics at the bottom are this package's own statements of the reference's policies on that surface;
the reference's functions run unchanged on these classes as well (same names, same attributes).
"""
from __future__ import annotations

import math
from collections import defaultdict
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib, traffic as _traffic
from .batched import DEFAULT_BIT_RATES, BatchedDeepRMSAEnv, BatchedRMSAEnv
from .topology import FrozenTopology, Path, Service

try:  # gym is optional: the reference needs it, this package only mirrors its spaces when present
    import gym as _gym  # type: ignore
except Exception:  # pragma: no cover - gym is not installed in the build image
    try:
        import gymnasium as _gym  # type: ignore
    except Exception:
        _gym = None


class _Space:
    """Minimal stand-in used when neither gym nor gymnasium is importable."""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)
        self._rng = np.random.default_rng()

    def seed(self, seed=None):
        self._rng = np.random.default_rng(seed)

    def sample(self):
        if self.kind == "MultiDiscrete":
            return tuple(int(self._rng.integers(0, n)) for n in self.nvec)
        if self.kind == "Discrete":
            return int(self._rng.integers(0, self.n))
        raise NotImplementedError(self.kind)


def _multi_discrete(nvec):
    if _gym is not None:
        return _gym.spaces.MultiDiscrete(nvec)
    return _Space("MultiDiscrete", nvec=tuple(nvec))


def _discrete(n):
    if _gym is not None:
        return _gym.spaces.Discrete(n)
    return _Space("Discrete", n=n)


def _box(low, high, shape, dtype):
    if _gym is not None:
        return _gym.spaces.Box(low=low, high=high, dtype=dtype, shape=shape)
    return _Space("Box", low=low, high=high, shape=shape, dtype=dtype)


class _LazyGraph(dict):
    """``topology.graph``: static keys plus device-backed ones fetched on access."""

    def __init__(self, static, env):
        super().__init__(static)
        self._env = env

    def __getitem__(self, key):
        if key == "available_slots":
            return self._env._available_slots()
        if key in ("throughput", "compactness", "last_update"):
            return float(self._env._batched.graph_stats()[key][self._env._index])
        return super().__getitem__(key)


class _View:
    """What the single-environment views share (``RMSAEnv`` here, ``PhyRMSAEnv`` in phy_env.py): the mirror of the pending
    request and the parts of the gym surface that do not touch the device."""

    metadata = {"metrics": ["service_blocking_rate", "episode_service_blocking_rate", "bit_rate_blocking_rate",
                            "episode_bit_rate_blocking_rate"]}

    def _service(self, r):
        """The ``Service`` of one row of ``requests()``."""
        nodes = self._ft.nodes
        return Service(int(r["service_id"]), nodes[r["src"]], int(r["src"]), destination=nodes[r["dst"]],
                       destination_id=int(r["dst"]), arrival_time=float(r["arrival_time"]),
                       holding_time=float(r["holding_time"]), bit_rate=int(r["bit_rate"]))

    def observation(self):
        return {"topology": self.topology, "current_service": self.current_service}

    def reward(self):
        return 1 if self.current_service.accepted else 0

    def seed(self, seed=None):
        """``optical_network_env.py:266-271``; see ``BatchedRMSAEnv.reseed`` for why this is refused."""
        raise NotImplementedError(
            "seed() after construction is not reproduced: the reference keeps drawing the BIT RATE from the generator object of "
            "construction time (functools.partial(self.rng.choices, ...)) while the other four draws of a request come from "
            "Random(seed) -- two generators per environment.  Pass seed= to the constructor, or call reseed() on the batched "
            "environment for a fresh generator for all draws (not the reference's stream).")

    def render(self, mode="human"):
        return


class RMSAEnv(_View):
    """Drop-in for ``RMSAEnv`` (``rmsa_env.py:18``) backed by the device path."""

    _batched_cls = BatchedRMSAEnv

    def __init__(self, topology=None, episode_length: int = 1000, load: float = None,
                 mean_service_holding_time: float = None, num_spectrum_resources: int = 100,
                 bit_rate_selection: str = "discrete", bit_rates: Sequence = DEFAULT_BIT_RATES,
                 bit_rate_probabilities=None, node_request_probabilities=None, bit_rate_lower_bound: float = 25.0,
                 bit_rate_higher_bound: float = 100.0, seed: Optional[int] = None, allow_rejection: bool = False,
                 reset: bool = True, channel_width: float = 12.5, device: int = 0, _batched=None, _index: int = 0,
                 trace=None, gn_gate=None, **_ignored):
        # (gn_gate=: the GN-model admission check of BatchedRMSAEnv; info["gn_gsnr_db"] exists only with it)
        # (load / mean_service_holding_time: None = the reference's defaults 10 / 10800.0; trace=: a RequestTrace to replay,
        # which excludes load, mean_service_holding_time and seed -- BatchedRMSAEnv)
        assert bit_rate_selection in ("continuous", "discrete")
        if _batched is None:
            _batched = self._batched_cls(topology, 1, episode_length=episode_length, load=load,
                                         mean_service_holding_time=mean_service_holding_time,
                                         num_spectrum_resources=num_spectrum_resources,
                                         bit_rate_selection=bit_rate_selection, bit_rates=bit_rates,
                                         bit_rate_lower_bound=bit_rate_lower_bound, bit_rate_higher_bound=bit_rate_higher_bound,
                                         bit_rate_probabilities=bit_rate_probabilities,
                                         node_request_probabilities=node_request_probabilities, seed=seed,
                                         allow_rejection=allow_rejection, channel_width=channel_width, device=device,
                                         trace=trace, gn_gate=gn_gate)
        self._init_view(_batched, _index)

    # ------------------------------------------------------------------ plumbing
    def _init_view(self, batched, index):
        self._batched = batched
        self._index = int(index)
        ft: FrozenTopology = batched.topology
        self._ft = ft
        view = ft.view()
        view.graph = _LazyGraph(dict(view.graph, num_spectrum_resources=batched.num_spectrum_resources), self)
        self.topology = view
        self.topology_name = ft.name
        self.k_paths = ft.k_paths
        self.k_shortest_paths = ft.ksp
        self.num_spectrum_resources = batched.num_spectrum_resources
        self.episode_length = batched.episode_length
        self.channel_width = batched.channel_width
        self.allow_rejection = batched.allow_rejection
        self.reject_action = batched.reject_action
        self.bit_rate_selection = getattr(batched, "bit_rate_selection", "discrete")
        if self.bit_rate_selection == "discrete":   # (rmsa_env.py:103-111: the attribute exists in this mode only)
            self.bit_rates = list(batched.bit_rates)
        else:
            self.bit_rate_lower_bound, self.bit_rate_higher_bound = batched.bit_rate_lower_bound, batched.bit_rate_higher_bound
        self.load = batched.load
        self.mean_service_holding_time = batched.mean_service_holding_time
        self.mean_service_inter_arrival_time = batched.mean_service_inter_arrival_time
        self.node_request_probabilities = batched.node_request_probabilities
        self.rand_seed = batched.rand_seed + self._index
        self.j = batched.j
        self.action_space = _multi_discrete((self.k_paths + self.reject_action,
                                             self.num_spectrum_resources + self.reject_action))
        self.observation_space = None
        self.action_space.seed(self.rand_seed)
        self.current_service: Optional[Service] = None
        # bookkeeping the reference keeps beside the simulation (no info key reads it): kept here, on the host, from what a step
        # returns -- rmsa_env.py:185-196 (shape (k + 1, S + 1) at construction), :118-128
        shape = (self.k_paths + 1, self.num_spectrum_resources + 1)
        self.actions_output = np.zeros(shape, dtype=int)
        self.episode_actions_output = np.zeros(shape, dtype=int)
        self.actions_taken = np.zeros(shape, dtype=int)
        self.episode_actions_taken = np.zeros(shape, dtype=int)
        if self.bit_rate_selection == "discrete":
            self.slots_requested_histogram = defaultdict(int)
            self.episode_slots_requested_histogram = defaultdict(int)
            self.slots_provisioned_histogram = defaultdict(int)
            self.episode_slots_provisioned_histogram = defaultdict(int)
        self._sync()
        self._count_request()

    def _count_request(self):
        """``_next_service`` (rmsa_env.py:676-686): the histogram of slots requested, assuming the shortest path."""
        if self.bit_rate_selection == "discrete":
            slots = self.get_number_slots(self._candidates[0])
            self.slots_requested_histogram[slots] += 1
            self.episode_slots_requested_histogram[slots] += 1

    def _reset_bookkeeping(self, only_episode_counters):
        """``reset`` (rmsa_env.py:343-389): the episode arrays are re-created (with the reject action's shape), the pending
        request counted again; the arrays of the whole run are never cleared."""
        shape = (self.k_paths + self.reject_action, self.num_spectrum_resources + self.reject_action)
        self.episode_actions_output = np.zeros(shape, dtype=int)
        self.episode_actions_taken = np.zeros(shape, dtype=int)
        if self.bit_rate_selection == "discrete":
            self.episode_slots_requested_histogram = defaultdict(int)
            self.episode_slots_provisioned_histogram = defaultdict(int)
            if only_episode_counters:
                self.episode_slots_requested_histogram[self.get_number_slots(self._candidates[0])] += 1
        if not only_episode_counters:
            self._count_request()   # (the full reset ends with _next_service)

    def _sync(self):
        """Refresh the host mirror of the pending request, the counters and the per-path masks."""
        b, i = self._batched, self._index
        self.current_service = self._service(b.requests()[i])
        c = b.counters()
        for name, arr in c.items():
            setattr(self, name, int(arr[i]))
        self.current_time = float(b.current_time()[i])
        masks, nslots = b.path_masks(i)
        bits = np.unpackbits(masks.view(np.uint8), axis=-1, bitorder="little")[:, :self.num_spectrum_resources]
        self._path_bits = bits.astype(np.int64)
        self._path_nslots = nslots
        self._candidates = self.k_shortest_paths[self.current_service.source, self.current_service.destination]
        self._avail_cache = None

    def _available_slots(self):
        if self._avail_cache is None:
            self._avail_cache = self._batched.available_slots()[self._index].astype(np.int64)
        return self._avail_cache

    def _bits_of(self, path: Path):
        for idp, p in enumerate(self._candidates):
            if p is path:
                return self._path_bits[idp]
        m, _ = self._batched.path_mask(path.gid, self._index)
        return np.unpackbits(m.view(np.uint8), bitorder="little")[:self.num_spectrum_resources].astype(np.int64)

    # ------------------------------------------------------------------ reference query surface
    def get_number_slots(self, path: Path, se=None) -> int:
        """``rmsa_env.py:708-719`` (plain arithmetic on the pending request).  ``se``: a spectral efficiency in the place of the
        path's own -- the level of a candidate behind a gate that chooses the modulation (not in the reference)."""
        se = path.best_modulation.spectral_efficiency if se is None else int(se)
        return math.ceil(self.current_service.bit_rate / (se * self.channel_width)) + 1

    def is_path_free(self, path: Path, initial_slot: int, number_slots: int) -> bool:
        """``rmsa_env.py:721-734``"""
        if initial_slot + number_slots > self.num_spectrum_resources:
            return False
        return bool(self._bits_of(path)[initial_slot:initial_slot + number_slots].all())

    def get_available_slots(self, path: Path):
        """``rmsa_env.py:745-756``"""
        return self._bits_of(path).copy()

    @staticmethod
    def rle(inarray):
        """``rmsa_env.py:758-772``: (start positions, values, run lengths)."""
        ia = np.asarray(inarray)
        n = len(ia)
        if n == 0:
            return None, None, None
        change = np.flatnonzero(ia[1:] != ia[:-1])
        ends = np.append(change, n - 1)
        lengths = np.diff(np.append(-1, ends))
        starts = np.cumsum(np.append(0, lengths))[:-1]
        return starts, ia[ends], lengths

    def get_available_blocks(self, path: int):
        """``rmsa_env.py:774-804``: first j free runs long enough for the pending request on candidate ``path``."""
        cand = self._candidates[path]
        slots = self.get_number_slots(cand)
        starts, values, lengths = self.rle(self._path_bits[path])
        ok = np.flatnonzero((values == 1) & (lengths >= slots))[: self.j]
        return starts[ok], lengths[ok]

    def _slot_bits(self):
        """[k, S] bool: ``step([p, s])`` would provision (``BatchedRMSAEnv.action_masks("slots")`` of this env)."""
        words = self._batched.action_masks("slots")[self._index]
        bits = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")[:, :self.num_spectrum_resources]
        return bits.astype(bool)

    def action_masks(self, gn=False):
        """Valid actions of ``MultiDiscrete(path, slot)`` for the pending request: bool [k + reject, S + reject], True where
        ``step([p, s])`` would provision the service (``rmsa_env.py:233-260``).  With ``allow_rejection`` the extra row and
        column belong to the explicit rejection ``[k, S]``: only their corner is True.  "The window is free": a GN-model
        admission check (``gn_gate=``) may still refuse it, and ``gn=True`` is refused here; the slot matrix that knows the gate
        is :meth:`admission_slot_masks`."""
        if gn:
            raise ValueError("action_masks(gn=True): there is no slot matrix that knows the GN-model admission check (k * S GSNR "
                             "evaluations per environment); the gated masks are DeepRMSAEnv's and PathOnlyFirstFitAction's")
        k, S, r = self.k_paths, self.num_spectrum_resources, self.reject_action
        m = np.zeros((k + r, S + r), bool)
        m[:k, :S] = self._slot_bits()
        if r:
            m[k, S] = True
        return m

    def admission_slot_masks(self):
        """:meth:`action_masks` under the GN-model admission check of this environment (``gn_gate=``, with ``protect_running`` both
        halves; ``BatchedRMSAEnv.admission_slot_masks``, not in the reference): bool [k + reject, S + reject], True where
        ``step([p, s])`` would be accepted -- the window is free, its GSNR meets the threshold of the path's modulation and no
        running lightpath that shares a link falls below its own.  The rejection's corner as in :meth:`action_masks`."""
        k, S, r = self.k_paths, self.num_spectrum_resources, self.reject_action
        words = self._batched.admission_slot_masks()[self._index]
        m = np.zeros((k + r, S + r), bool)
        m[:k, :S] = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")[:, :S].astype(bool)
        if r:
            m[k, S] = True
        return m

    def qot_audit(self, gate=None):
        """The GN-model audit of this environment's running lightpaths (``BatchedRMSAEnv.qot_audit``; not in the reference): a dict
        -- ``n_running``, ``n_below``, ``worst_rank`` (ints), ``min_margin_db`` (float, NaN when nothing runs) and ``services``, one
        dict per running service in ascending release time: ``path_gid``, ``slot``, ``num_slots``, ``bit_rate``, ``release_time``,
        ``gsnr_db``, ``margin_db``, ``osnr_ase_db``, ``snr_nli_db``.  ``gate``: as there."""
        b, i = self._batched, self._index
        a = b.qot_audit(gate=gate, services=True)
        run = b.running_services()
        n = int(a["n_running"][i])
        names = ("path_gid", "slot", "num_slots", "bit_rate", "release_time")
        return {"n_running": n, "n_below": int(a["n_below"][i]), "worst_rank": int(a["worst_rank"][i]),
                "min_margin_db": float(a["min_margin_db"][i]),
                "services": [dict({k: run[k][i, r].item() for k in names}, **{k: float(a[k][i, r]) for k in b.AUDIT_SERVICE_FIELDS})
                             for r in range(n)]}

    # ------------------------------------------------------------------ gym surface
    def reset(self, only_episode_counters: bool = True):
        """``rmsa_env.py:343-457``"""
        if self._batched.batch_size != 1:
            raise RuntimeError("reset() of a view into a larger batch would reset every env: use the batched API")
        self._batched.reset(only_episode_counters)
        self._sync()
        self._reset_bookkeeping(only_episode_counters)
        return self.observation()

    def _resolved_action(self, action, r):
        """(path, initial_slot) as RMSAEnv.step sees them"""
        return int(action[0]), int(action[1])

    @staticmethod
    def _action_level(action):
        """the se of a (path, slot, se) action, None for every other action (DeepRMSA's and the path-only space's are one integer)"""
        return int(action[2]) if np.ndim(action) == 1 and len(action) == 3 else None

    def _device_step(self, action):
        path, initial_slot = int(action[0]), int(action[1])
        if self._action_level(action) is not None:   # (path, slot, se) behind a gate that chooses the modulation: the device checks the rest
            return self._batched.run("external_am", 1, actions=np.array([[path, initial_slot, int(action[2])]], np.int32),
                                     outputs=("accepted", "done", "reward", "network_compactness",
                                              "network_compactness_difference", "avg_link_compactness",
                                              "avg_link_utilization", "gn_gsnr_db", "gn_se"))
        return self._batched.run("external", 1, actions=np.array([[path, initial_slot]], np.int32),
                                 outputs=("accepted", "done", "reward", "network_compactness",
                                          "network_compactness_difference", "avg_link_compactness",
                                          "avg_link_utilization") + self._gate_outputs())

    def _gate_outputs(self):
        if self._batched.gn_gate is None:
            return ()
        return ("gn_gsnr_db", "gn_neighbour_margin_db") if self._batched.gn_protect else ("gn_gsnr_db",)

    def step(self, action):
        """``rmsa_env.py:222-341`` -> (observation, reward, done, info)"""
        if self._batched.batch_size != 1:
            raise RuntimeError("step() needs a batch-1 environment: use the batched API for B > 1")
        served = self.current_service
        candidates = self._candidates
        r = self._device_step(action)
        served.accepted = bool(r["accepted"][0, 0])
        # rmsa_env.py:226, 261-267, 271, 509: every action counted, the accepted ones again -- and their slots twice (step and
        # _provision_path both add one)
        path, initial_slot = self._resolved_action(action, r)
        self.actions_output[path, initial_slot] += 1
        if served.accepted:
            self.actions_taken[path, initial_slot] += 1
            if self.bit_rate_selection == "discrete":
                se = self._action_level(action)   # (a level of its own: the slots it took are the level's)
                self.slots_provisioned_histogram[self.get_number_slots(candidates[path], se)] += 2
        else:
            self.actions_taken[self.k_paths, self.num_spectrum_resources] += 1
        info = self._info(float(r["network_compactness"][0, 0]), float(r["network_compactness_difference"][0, 0]),
                          float(r["avg_link_compactness"][0, 0]), float(r["avg_link_utilization"][0, 0]))
        if "gn_gsnr_db" in r:   # (a handle with a GN-model admission check: the GSNR it compared, NaN = no check ran)
            info["gn_gsnr_db"] = float(r["gn_gsnr_db"][0, 0])
        if "gn_se" in r:   # (... that chooses the modulation: the level of the candidate it checked, 0 = no check ran)
            info["gn_se"] = int(r["gn_se"][0, 0])
        if "gn_neighbour_margin_db" in r:   # (... that protects its running lightpaths: the neighbour margin, NaN = that check did not run)
            info["gn_neighbour_margin_db"] = float(r["gn_neighbour_margin_db"][0, 0])
        reward = r["reward"][0, 0]
        reward = int(reward) if float(reward).is_integer() else float(reward)
        self._sync()
        self._count_request()
        self._last_served = served
        return self.observation(), reward, bool(r["done"][0, 0]), info

    def _info(self, compactness, compactness_difference, avg_link_compactness, avg_link_utilization):
        """The info dict of ``rmsa_env.py:293-332``: integer ratios from the device counters (Python int
        division, as in the reference), floats from the device statistics."""
        b, i = self._batched, self._index
        c = {k: int(v[i]) for k, v in b.counters().items()}
        nxt_rate = int(b.requests()[i]["bit_rate"])
        info = dict(_traffic.blocking_rates(c, nxt_rate), network_compactness=compactness,
                    network_compactness_difference=compactness_difference)
        # np.mean over the links, evaluated on the device at the reference's point in the step
        info["avg_link_compactness"] = avg_link_compactness
        info["avg_link_utilization"] = avg_link_utilization
        if self.bit_rate_selection != "discrete":   # rmsa_env.py:276, 327: the per-rate keys exist in discrete mode only
            return info
        h = b.bit_rate_hist()
        blocking = {}
        for k, rate in enumerate(self.bit_rates):
            req, prov = int(h["requested"][i, k]) - (1 if rate == nxt_rate else 0), int(h["provisioned"][i, k])
            blocking[rate] = (req - prov) / req if req > 0 else 0.0
        for rate, v in blocking.items():
            info[f"bit_rate_blocking_{rate}"] = v
        info["fairness"] = max(blocking.values()) - min(blocking.values())
        return info

    def close(self):
        if self._batched.batch_size == 1:
            self._batched.close()


class DeepRMSAEnv(RMSAEnv):
    """Drop-in for ``DeepRMSAEnv`` (``deeprmsa_env.py:9``)."""

    _batched_cls = BatchedDeepRMSAEnv

    def __init__(self, topology=None, j: int = 1, episode_length: int = 1000, mean_service_holding_time: float = None,
                 mean_service_inter_arrival_time: float = None, num_spectrum_resources: int = 100,
                 node_request_probabilities=None, seed=None, allow_rejection: bool = False, device: int = 0,
                 _batched=None, _index: int = 0, trace=None, gn_gate=None):
        # (the means: None = the reference's defaults 25.0 / 0.1; trace=: a RequestTrace to replay, which excludes them)
        if _batched is None:
            _batched = BatchedDeepRMSAEnv(topology, 1, j=j, episode_length=episode_length,
                                          mean_service_holding_time=mean_service_holding_time,
                                          mean_service_inter_arrival_time=mean_service_inter_arrival_time,
                                          num_spectrum_resources=num_spectrum_resources,
                                          node_request_probabilities=node_request_probabilities, seed=seed,
                                          allow_rejection=allow_rejection, device=device, trace=trace, gn_gate=gn_gate)
        self._init_view(_batched, _index)
        shape = 1 + 2 * self._ft.num_nodes + (2 * self.j + 3) * self.k_paths
        self.observation_space = _box(-2 ** 30, 2 ** 30, (shape,), np.float64)
        self.action_space = _discrete(self.k_paths * self.j + self.reject_action)
        self.action_space.seed(self.rand_seed)

    def observation(self):
        """``deeprmsa_env.py:60-121`` (built by ``orlg_deeprmsa_obs_kernel``)."""
        return self._batched.observation()[self._index]

    def reward(self):
        return 1 if self.current_service.accepted else -1

    def _device_step(self, action):
        return self._batched.run("deeprmsa_external", 1, actions=np.array([int(action)], np.int32),
                                 outputs=("accepted", "done", "reward", "network_compactness",
                                          "network_compactness_difference", "avg_link_compactness",
                                          "avg_link_utilization", "act_path", "act_slot") + self._gate_outputs())

    def _resolved_action(self, action, r):
        """``deeprmsa_env.py:48-58``: the (route, first slot of the block) the action stands for, (k, S) for a rejection"""
        return int(r["act_path"][0, 0]), int(r["act_slot"][0, 0])

    def _get_route_block_id(self, action: int) -> Tuple[int, int]:
        return action // self.j, action % self.j

    def action_masks(self, gn=False):
        """Valid actions of ``Discrete(k*j + reject)`` for the pending request: bool [k*j + reject], True where ``step(a)``
        would accept the service (the method maskable-PPO implementations look for).  ``gn=True`` (a ``gn_gate=`` environment):
        the mask that knows the GN-model admission check, ``BatchedRMSAEnv.action_masks("deeprmsa_gn")`` -- and, where the gate
        protects the running lightpaths, both halves of it: ``BatchedRMSAEnv.admission_masks("deeprmsa")``."""
        if gn and self._batched.gn_protect:
            return self._batched.admission_masks("deeprmsa")[self._index].astype(bool)
        return self._batched.action_masks("deeprmsa_gn" if gn else "deeprmsa")[self._index].astype(bool)


class SimpleMatrixObservation:
    """``rmsa_env.py:940-971``: observation = one-hot endpoints + the E x S free-slot matrix (built on the device)."""

    def __init__(self, env: RMSAEnv):
        self.env = env
        shape = env.topology.number_of_nodes() * 2 + env.topology.number_of_edges() * env.num_spectrum_resources
        self.observation_space = _box(0, 1, (shape,), np.uint8)
        self.action_space = env.action_space

    def __getattr__(self, name):
        return getattr(self.env, name)

    def observation(self, observation=None):
        return self.env._batched.simple_matrix_observation()[self.env._index]

    def reset(self, **kw):
        self.env.reset(**kw)
        return self.observation()

    def step(self, action):
        _, reward, done, info = self.env.step(action)
        return self.observation(), reward, done, info


class PathOnlyFirstFitAction:
    """``rmsa_env.py:974-1008``: the agent chooses the path, the slot is the first fit (resolved on the device).

    ``assign=`` (not in the reference): another rule of ``ASSIGN_RULES`` picks the slot on the agent's path -- what the device
    policies ``path_{ff_full,lf,bf,ef}_external`` resolve (``BatchedRMSAEnv.run``); the default ``"first"`` is the reference's."""

    assign, policy = "first", "path_ff_external"   # the reference's wrapper

    def __init__(self, env, assign="first"):
        if assign not in _lib.ASSIGN_RULES:
            raise ValueError(f"assign {assign!r}: expected one of {_lib.ASSIGN_RULES}")
        self.assign = assign
        # the device policy that resolves the same actions for a whole batch
        self.policy = "path_ff_external" if assign == "first" else f"path_{_lib._ASSIGN_SUFFIX[assign]}_external"
        self.env = env
        inner = env
        while not isinstance(inner, RMSAEnv):
            inner = inner.env
        self._inner = inner
        self.action_space = _discrete(inner.k_paths + inner.reject_action)
        self.observation_space = getattr(env, "observation_space", None)

    def __getattr__(self, name):
        return getattr(self.env, name)

    def action(self, action) -> Tuple[int, int]:
        e = self._inner
        if self.assign != "first":
            if 0 <= action < e.k_paths:
                path = e.k_shortest_paths[e.current_service.source, e.current_service.destination][action]
                s = assignment_slot(e.get_available_slots(path), e.get_number_slots(path), self.assign)
                if s is not None:
                    return (action, s)
            return (e.topology.graph["k_paths"], e.topology.graph["num_spectrum_resources"])
        if action < e.k_paths:
            path = e.k_shortest_paths[e.current_service.source, e.current_service.destination][action]
            n = e.get_number_slots(path)
            for s in range(0, e.topology.graph["num_spectrum_resources"] - n):
                if e.is_path_free(path, s, n):
                    return (action, s)
        return (e.topology.graph["k_paths"], e.topology.graph["num_spectrum_resources"])

    def action_masks(self, gn=False):
        """Valid paths for the pending request: bool [k + reject], True where ``action(p)`` finds a slot.  ``gn=True`` (a
        ``gn_gate=`` environment): ... and the GN-model admission check admits that window (``"path_ff_gn"``; where the gate
        protects the running lightpaths, both halves of the check: ``BatchedRMSAEnv.admission_masks("path_ff")``).  With
        ``assign=`` another rule: the paths that have a window, ``path_fit_levels() >= 3`` (no mask kernel of its own)."""
        if self.assign != "first":
            if gn:
                raise ValueError("action_masks(gn=True): the assignment rules do not run with a GN-model admission check")
            e = self._inner
            m = np.ones(e.k_paths + e.reject_action, bool)
            m[:e.k_paths] = e._batched.path_fit_levels()[e._index] >= 3
            return m
        if gn and self._inner._batched.gn_protect:
            return self._inner._batched.admission_masks("path_ff")[self._inner._index].astype(bool)
        return self._inner._batched.action_masks("path_ff_gn" if gn else "path_ff")[self._inner._index].astype(bool)

    def step(self, action):
        return self.env.step(self.action(action))

    def reset(self, **kw):
        return self.env.reset(**kw)


# --------------------------------------------------------------------------------------- heuristics
def shortest_path_first_fit(env: RMSAEnv) -> Tuple[int, int]:
    """SP-FF (``rmsa_env.py:854-871``): first fit on the shortest path only; note the exclusive bound."""
    S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
    path = env.k_shortest_paths[env.current_service.source, env.current_service.destination][0]
    n = env.get_number_slots(path)
    for s in range(0, S - n):
        if env.is_path_free(path, s, n):
            return (0, s)
    return (k, S)


def shortest_available_path_first_fit(env: RMSAEnv) -> Tuple[int, int]:
    """SAP-FF (``rmsa_env.py:901-913``)."""
    S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
    for idp, path in enumerate(env.k_shortest_paths[env.current_service.source, env.current_service.destination]):
        n = env.get_number_slots(path)
        for s in range(0, S - n):
            if env.is_path_free(path, s, n):
                return (idp, s)
    return (k, S)


def shortest_available_path_first_fit_gn(env: RMSAEnv) -> Tuple[int, int]:
    """QoT-aware SAP-FF on a ``gn_gate=`` environment (not in the reference): what the device policy ``"sap_ff_gn"`` proposes.
    The first path whose first-fit window the admission check admits (``action_masks("path_ff_gn")`` of this environment); if
    none is admitted, the first path that has a first fit -- the step then refuses it, as the device policy's step is refused;
    if no path has one, the rejection."""
    S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
    mask, gsnr = env._batched.action_masks("path_ff_gn", gsnr_out=True)
    admitted, fits = np.flatnonzero(mask[env._index, :k]), np.flatnonzero(np.isfinite(gsnr[env._index]))
    if fits.size == 0:
        return (k, S)
    idp = int(admitted[0] if admitted.size else fits[0])
    path = env.k_shortest_paths[env.current_service.source, env.current_service.destination][idp]
    n = env.get_number_slots(path)
    for s in range(0, S - n):
        if env.is_path_free(path, s, n):
            return (idp, s)
    return (k, S)


def adaptive_modulation_heuristic(route):
    """A callback ``f(env) -> (path, slot, se)`` for an environment whose gate chooses the modulation
    (``gn_gate=rmsa_gn_gate_parameters(..., modulation="adaptive")``; not in the reference): what the device policies
    ``"sp_ff_am"`` (``route="sp"``) and ``"sap_ff_am"`` (``"sap"``) propose, read from ``BatchedRMSAEnv.modulation_windows``.  The
    paths in scope in order, each with its levels ``M`` down to 1: the first admitted candidate; if none is admitted, the first
    candidate that has a window -- the step then refuses it; if none has one, ``(k, S, 0)``, the rejection."""
    if route not in ("sp", "sap"):
        raise ValueError(f"route {route!r}: expected 'sp' or 'sap'")

    def heuristic(env):
        S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
        slot, _, admitted, _ = env._batched.modulation_windows()
        slot, admitted = slot[env._index], admitted[env._index]
        first = None
        for idp in range(1 if route == "sp" else k):
            for m in range(slot.shape[1], 0, -1):
                if slot[idp, m - 1] >= S:
                    break
                if admitted[idp, m - 1]:
                    return (idp, int(slot[idp, m - 1]), m)
                if first is None:
                    first = (idp, int(slot[idp, m - 1]), m)
        return first if first is not None else (k, S, 0)

    heuristic.__name__ = f"{route}_adaptive_modulation"
    return heuristic


MAX_MARGIN_ROUTES = ("sap", "any")


def max_margin_heuristic(route):
    """A callback ``f(env) -> (path, slot)`` for a ``gn_gate=`` environment (not in the reference): of the windows the
    admission check admits, the one that leaves the most margin (``BatchedRMSAEnv.max_margin_windows``).  ``route``: ``"sap"`` -- the
    first candidate path that has an admitted window, at its best window; ``"any"`` -- the path whose best window has the largest
    margin, the lowest index on ties.  ``(k, S)``, the rejection, if no path has an admitted window."""
    if route not in MAX_MARGIN_ROUTES:
        raise ValueError(f"route {route!r}: expected one of {MAX_MARGIN_ROUTES}")

    def heuristic(env):
        S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
        slots, margin = env._batched.max_margin_windows()
        slots, margin = slots[env._index], margin[env._index]
        has = np.flatnonzero(slots < S)
        if has.size == 0:
            return (k, S)
        idp = int(has[0]) if route == "sap" else int(has[np.argmax(margin[has])])
        return (idp, int(slots[idp]))

    heuristic.__name__ = f"{route}_max_margin"
    return heuristic


def assignment_slot(available, n, rule):
    """The start slot of assignment rule ``rule`` (``ASSIGN_RULES``; include/orlg.h ``ORLG_ASSIGN_*``, not in the reference) for a
    request of ``n`` slots on a path whose availability vector is ``available`` (``get_available_slots``), or None when the path
    has no window.  A window is a start ``s`` in ``0 .. S - n`` inclusive with ``[s, s + n)`` free; ``"first"`` alone keeps the
    reference's bound ``range(0, S - n)``.  A block is a maximal free run (``rmsa_env.py:774-804``)."""
    a = np.asarray(available).astype(bool)
    S = len(a)
    starts, values, lengths = RMSAEnv.rle(a)
    if starts is None:
        return None
    ok = np.flatnonzero(values & (lengths >= n))   # the blocks that hold the request
    if rule == "first":
        for b in ok:
            if starts[b] < S - n:
                return int(starts[b])
        return None
    if ok.size == 0:
        return None
    if rule == "first_full":
        return int(starts[ok[0]])
    if rule == "last":
        return int(starts[ok[-1]] + lengths[ok[-1]] - n)
    if rule == "best":
        return int(starts[ok[np.argmin(lengths[ok])]])   # (argmin: the first of equal lengths, the lowest start)
    if rule == "exact":
        same = ok[lengths[ok] == n]
        return int(starts[same[0] if same.size else ok[0]])
    raise ValueError(f"rule {rule!r}: expected one of {_lib.ASSIGN_RULES}")


def _gn_mode(route, gn):
    """The ``gn=`` argument of the heuristics below, checked."""
    if gn not in (None, "check", "next_path"):
        raise ValueError(f"gn {gn!r}: expected None, 'check' or 'next_path'")
    if gn == "next_path" and route != "sap":
        raise ValueError(f"gn='next_path' goes on to the next candidate path: it needs route 'sap', got {route!r}")
    return gn


def _next_path_action(env, rule):
    """What ``run("sap_<rule>", gn_rule="next_path")`` proposes for the pending request of a ``gn_gate=`` view, read from the
    handle's query ``path_rule_windows(rule)``: the first path whose rule window the admission check admits; none admitted: the
    first path that has a window, which the step then refuses as the device's step is refused; no window: the rejection."""
    S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
    slots, _, admitted = env._batched.path_rule_windows(rule)
    ok, has = np.flatnonzero(admitted[env._index]), np.flatnonzero(slots[env._index] < S)
    if has.size == 0:
        return [k, S]
    idp = int(ok[0] if ok.size else has[0])
    return [idp, int(slots[env._index, idp])]


def assignment_heuristic(route, rule, gn=None):
    """A heuristic ``f(env) -> [path, slot]`` in the drop-in callback shape of ``shortest_available_path_first_fit``: route
    ``"sp"`` (path 0), ``"sap"`` (the first path that has a window) or ``"llp"`` (of the paths that have a window the one with
    the most free slots, strict ``>``; ``rmsa_env.py:854-937``) with assignment rule ``rule`` of ``ASSIGN_RULES`` on it.  Not in
    the reference beyond ``rule="first"``; what the device policies ``{sp,sap,llp}_{ff,ff_full,lf,bf,ef}`` propose, written on
    the view's own ``get_available_slots`` / ``get_number_slots``.

    ``gn=`` (a ``gn_gate=`` view): ``"check"`` -- what ``run(name, gn_rule="check")`` proposes, which is the proposal
    above (the view's step applies the check); ``"next_path"`` (route ``"sap"``, a rule other than ``"first"``) -- what
    ``run(name, gn_rule="next_path")`` proposes, read from the handle's ``path_rule_windows(rule)``."""
    if route not in ("sp", "sap", "llp"):
        raise ValueError(f"route {route!r}: expected 'sp', 'sap' or 'llp'")
    if rule not in _lib.ASSIGN_RULES:
        raise ValueError(f"rule {rule!r}: expected one of {_lib.ASSIGN_RULES}")
    if _gn_mode(route, gn) is not None and rule == "first":
        raise ValueError("gn=: rule 'first' is the reference's first fit (shortest_available_path_first_fit_gn goes on to the next path)")

    def heuristic(env):
        if gn == "next_path":
            return _next_path_action(env, rule)
        S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
        paths = env.k_shortest_paths[env.current_service.source, env.current_service.destination]
        best, action = 0, [k, S]
        for idp, path in enumerate(paths[:1] if route == "sp" else paths):
            available = env.get_available_slots(path)
            s = assignment_slot(available, env.get_number_slots(path), rule)
            if s is None:
                continue
            if route != "llp":
                return [idp, s]
            free = int(np.sum(available))
            if free > best:
                best, action = free, [idp, s]
        return action

    heuristic.__name__ = f"{route}_{rule}"
    return heuristic


def _min_cut_slot(rows, n):
    """The fewest-cuts window of a request of ``n`` slots on a path whose links have the availability ``rows`` [hops, S]
    (``topology.graph["available_slots"]`` rows): ``(cuts, start)`` or None when the path has no window.  A window is a start
    ``s`` in ``0 .. S - n`` inclusive with ``[s, s + n)`` free on every link; its cuts are the links with slot ``s - 1`` and slot
    ``s + n`` both free (slots -1 and S are not); fewest cuts, then lowest start (include/orlg.h ``orlg_step_min_cut``)."""
    rows = np.asarray(rows).astype(bool)
    S = rows.shape[1]
    both = rows.all(axis=0)
    best = None
    for s in range(0, S - n + 1):
        if not both[s:s + n].all():
            continue
        cuts = sum(1 for r in rows if s > 0 and r[s - 1] and s + n < S and r[s + n])
        if best is None or cuts < best[0]:
            best = (cuts, s)
    return best


def min_cut_heuristic(route, gn=None):
    """A heuristic ``f(env) -> [path, slot]`` for ``RMSA-v0`` in the drop-in callback shape of
    ``shortest_available_path_first_fit``: the window with the fewest cuts on route ``"sp"`` (path 0), ``"sap"`` (the first path
    that has a window), ``"llp"`` (of the paths that have a window the one with the most free slots, strict ``>``) or
    ``"min_cut"`` (of all paths the one whose fewest-cuts window has the fewest cuts, ties to the lowest path).  Not in the
    reference for this environment (its ``calculate_r_cut`` belongs to the QoT-aware one); what the device policies
    ``sp_mc`` / ``sap_mc`` / ``llp_mc`` / ``min_cut`` propose, written on what the view exposes: the rows of
    ``topology.graph["available_slots"]``, the link indices along a path's ``node_list`` and ``get_number_slots``.
    ``gn=``: as :func:`assignment_heuristic` (``"next_path"`` reads ``path_rule_windows("min_cut")``)."""
    if route not in ("sp", "sap", "llp", "min_cut"):
        raise ValueError(f"route {route!r}: expected 'sp', 'sap', 'llp' or 'min_cut'")
    _gn_mode(route, gn)

    def heuristic(env):
        if gn == "next_path":
            return _next_path_action(env, "min_cut")
        S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
        paths = env.k_shortest_paths[env.current_service.source, env.current_service.destination]
        avail = env.topology.graph["available_slots"]
        best, action = None, [k, S]
        for idp, path in enumerate(paths[:1] if route == "sp" else paths):
            nodes = path.node_list
            rows = np.asarray([avail[env.topology[nodes[i]][nodes[i + 1]]["index"]] for i in range(len(nodes) - 1)])
            got = _min_cut_slot(rows, env.get_number_slots(path))
            if got is None:
                continue
            if route in ("sp", "sap"):
                return [idp, got[1]]
            rank = int(rows.all(axis=0).sum()) if route == "llp" else -got[0]
            if best is None or rank > best:
                best, action = rank, [idp, got[1]]
        return action

    heuristic.__name__ = f"{route}_min_cut"
    return heuristic


_WINDOW_RULES = ("first_full", "last", "best", "exact", "most_used")


def _window_proposal(available, usage, n, rule):
    """The rule window of a request of ``n`` slots on a path with the availability vector ``available`` (``get_available_slots``)
    and the network's slot usage ``usage`` [S]: ``(rank, start)``, ``rank`` a tuple that is smaller for the better proposal by the
    rule's own order (include/orlg.h ``orlg_step_window``), or None when the path has no window.  A window is a start ``s`` in
    ``0 .. S - n`` inclusive with ``[s, s + n)`` free; a block is a maximal free run."""
    a = np.asarray(available).astype(bool)
    S = len(a)
    best = None
    for s in range(0, S - n + 1):
        if not a[s:s + n].all():
            continue
        lo, hi = s, s + n
        while lo > 0 and a[lo - 1]:
            lo -= 1
        while hi < S and a[hi]:
            hi += 1
        rank = {"first_full": (s,), "last": (-s,), "best": (hi - lo, lo), "exact": (int(hi - lo != n), lo),
                "most_used": (-int(np.sum(usage[s:s + n])), s)}[rule]
        start = s if rule in ("first_full", "last", "most_used") else lo
        if best is None or rank < best[0]:
            best = (rank, start)
    return best


def window_heuristic(route, rule):
    """A heuristic ``f(env) -> [path, slot]`` for ``RMSA-v0`` in the drop-in callback shape of
    ``shortest_available_path_first_fit``: rule ``"first_full"``, ``"last"``, ``"best"``, ``"exact"`` or ``"most_used"`` (the
    window whose slots are occupied on the most links of the whole network, ties to the lowest start) on route ``"sp"`` (path
    0), ``"sap"`` (the first path that has a window), ``"llp"`` (of the paths that have a window the one with the most free
    slots, strict ``>``) or ``"any"`` (every path proposes its rule window; the proposal that ranks best by the rule's own order
    wins, ties to the lowest path).  Not in the reference; what the device policies of ``WINDOW_POLICIES`` and
    ``{sp,sap,llp}_{ff_full,lf,bf,ef}`` propose, written on what the view exposes: ``get_available_slots``,
    ``get_number_slots`` and the rows of ``topology.graph["available_slots"]``."""
    if route not in ("sp", "sap", "llp", "any"):
        raise ValueError(f"route {route!r}: expected 'sp', 'sap', 'llp' or 'any'")
    if rule not in _WINDOW_RULES:
        raise ValueError(f"rule {rule!r}: expected one of {_WINDOW_RULES}")

    def heuristic(env):
        S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
        paths = env.k_shortest_paths[env.current_service.source, env.current_service.destination]
        avail = np.asarray(env.topology.graph["available_slots"])
        usage = avail.shape[0] - avail.astype(np.int64).sum(axis=0)   # links on which the slot is occupied
        best, action = None, [k, S]
        for idp, path in enumerate(paths[:1] if route == "sp" else paths):
            available = env.get_available_slots(path)
            got = _window_proposal(available, usage, env.get_number_slots(path), rule)
            if got is None:
                continue
            if route in ("sp", "sap"):
                return [idp, got[1]]
            rank = (-int(np.sum(available)),) if route == "llp" else got[0]
            if best is None or rank < best:
                best, action = rank, [idp, got[1]]
        return action

    heuristic.__name__ = f"{route}_{rule}_window"
    return heuristic


def least_loaded_path_first_fit(env: RMSAEnv) -> Tuple[int, int]:
    """LLP-FF (``rmsa_env.py:916-937``): among paths with a first fit, the one with most free slots (strict >)."""
    S, k = env.topology.graph["num_spectrum_resources"], env.topology.graph["k_paths"]
    best, action = 0, (k, S)
    for idp, path in enumerate(env.k_shortest_paths[env.current_service.source, env.current_service.destination]):
        n = env.get_number_slots(path)
        for s in range(0, S - n):
            if env.is_path_free(path, s, n):
                free = int(np.sum(env.get_available_slots(path)))
                if free > best:
                    best, action = free, (idp, s)
                break
    return action


def deeprmsa_shortest_path_first_fit(env: DeepRMSAEnv) -> int:
    """``deeprmsa_env.py:135-143``"""
    if not env.allow_rejection:
        return 0
    starts, _ = env.get_available_blocks(0)
    return 0 if len(starts) > 0 else env.k_paths * env.j


def deeprmsa_shortest_available_path_first_fit(env: DeepRMSAEnv) -> int:
    """``deeprmsa_env.py:146-155``"""
    for idp, _ in enumerate(env.k_shortest_paths[env.current_service.source, env.current_service.destination]):
        starts, _ = env.get_available_blocks(idp)
        if len(starts) > 0:
            return idp * env.j
    return env.k_paths * env.j


def random_policy(env):
    return env.action_space.sample()


def evaluate_heuristic(env, heuristic, n_eval_episodes=10, render=False, callback=None, reward_threshold=None,
                       return_episode_rewards=False):
    """``utils.py:124-162``, accepting both 4-tuple (RMSA / DeepRMSA) and 5-tuple (PhyRMSA) steps -- the
    reference's own loop unpacks five values and therefore cannot drive RMSAEnv."""
    episode_rewards, episode_lengths = [], []
    for _ in range(n_eval_episodes):
        env.reset()
        done, episode_reward, episode_length = False, 0.0, 0
        while not done:
            out = env.step(heuristic(env))
            reward, done = out[1], out[2]
            episode_reward += reward
            if callback is not None:
                callback(locals(), globals())
            episode_length += 1
            if render:
                env.render()
        episode_rewards.append(episode_reward)
        episode_lengths.append(episode_length)
    mean_reward, std_reward = np.mean(episode_rewards), np.std(episode_rewards)
    if reward_threshold is not None:
        assert mean_reward > reward_threshold, "Mean reward below threshold: {:.2f} < {:.2f}".format(
            mean_reward, reward_threshold)
    if return_episode_rewards:
        return episode_rewards, episode_lengths
    return mean_reward, std_reward
