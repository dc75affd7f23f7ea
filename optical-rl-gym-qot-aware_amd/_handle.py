"""What the two batched environments share on the host: ``BatchedHandle`` is the base of ``BatchedRMSAEnv`` (batched.py) and
``BatchedPhyRMSAEnv`` (phy.py).  Both C APIs stand on one handle core (``csrc/orlg_host.hip``), so every function that works
on the core exists under both prefixes, ``orlg_`` / ``orlg_phy_``, with one prototype (``_lib.PROTOTYPES``); the base binds
them once per handle and holds everything written against them: lifetime, stream, reset / reseed, the trace position, the
read-backs of requests / counters / time / running services, checkpoints, traffic and the reductions -- and the steps of the
constructor both kinds take.  Buffer checks and ``SweepTraffic`` live here too (batched.py re-exports them).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _lib, trace as _trace, traffic as _traffic
from .topology import FrozenTopology, selection_tables

COUNTER_NAMES = ("services_processed", "services_accepted", "episode_services_processed",
                 "episode_services_accepted", "bit_rate_requested", "bit_rate_provisioned",
                 "episode_bit_rate_requested", "episode_bit_rate_provisioned")

REQUEST_DTYPE = np.dtype([("service_id", np.int32), ("src", np.int32), ("dst", np.int32), ("bit_rate", np.int32),
                          ("arrival_time", np.float64), ("holding_time", np.float64)])


def _ptr(a):
    """Pointer of a numpy array, a torch tensor (host or device) or None."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _dtype_name(a):
    """'int32', 'float64', ... of a numpy array or a torch tensor."""
    return str(a.dtype).replace("torch.", "")


class SweepTraffic:
    """``load=`` / ``mean_service_holding_time=`` / ``groups=`` of a batched constructor.  Scalars without groups: the
    handle is created as ever (``orlg_create`` / ``orlg_phy_create``).  Length-B array-likes, or ``groups=`` (also next to a
    scalar load): the handle is created with ``orlg_traffic`` (include/orlg.h) and the environments carry their own rates.
    ``groups=`` and ``load=`` are independent: a group is any set of environments whose counters are summed together; the
    per-load Monitor tree and summary (monitor.py) need every group to be ONE load and refuse anything else.
    Shapes and values of a per-environment call are checked here, before the library is loaded."""

    def __init__(self, batch_size, load, mean_service_holding_time, groups=None, num_groups=None):
        self.batch_size = int(batch_size)
        self.per_env = np.ndim(load) > 0 or np.ndim(mean_service_holding_time) > 0 or groups is not None
        self._group_given = groups is not None
        if not self.per_env and num_groups not in (None, 1):
            raise ValueError("num_groups without groups")
        if self.per_env:
            self.arrival_lambda, self.holding_lambda = _traffic.per_env_rates(batch_size, load, mean_service_holding_time)
            self.loads = np.broadcast_to(np.asarray(load, np.float64), (self.batch_size,)).copy()
            self.groups, self.num_groups = _traffic.check_groups(batch_size, groups, num_groups)
        else:   # a scalar call: nothing is checked or computed here, the library sees what it always saw
            self.arrival_lambda = self.holding_lambda = None
            self.loads = np.full(max(self.batch_size, 0), float(load), np.float64)
            self.groups, self.num_groups = np.zeros(max(self.batch_size, 0), np.int32), 1

    def _need_rates(self):
        if not self.per_env:
            raise RuntimeError("a handle with scalar rates has no orlg_traffic")

    def largest(self):
        """Index of the environment with the largest offered load (what the library sizes its capacities from)."""
        self._need_rates()
        return int(np.argmax(self.arrival_lambda / self.holding_lambda))

    def struct(self):
        """The ``orlg_traffic`` of the handle (the arrays stay referenced by this object)."""
        self._need_rates()
        t = _lib.Traffic()
        t.arrival_lambda = self.arrival_lambda.ctypes.data_as(C.c_void_p)
        t.holding_lambda = self.holding_lambda.ctypes.data_as(C.c_void_p)
        t.group = self.groups.ctypes.data_as(C.c_void_p) if self._group_given else None
        t.num_groups = self.num_groups
        return t


def _check_buffer(name, a, shape, dtype):
    """A caller-supplied array the library reads or writes through a raw pointer: shape, dtype and layout must be exactly
    what the C ABI expects (a wrong dtype would be reinterpreted, a short array overrun)."""
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(a.shape)}, expected {tuple(shape)}")
    if _dtype_name(a) != str(np.dtype(dtype)):
        raise TypeError(f"{name}: dtype {_dtype_name(a)}, expected {np.dtype(dtype)}")
    contiguous = a.is_contiguous() if hasattr(a, "is_contiguous") else a.flags["C_CONTIGUOUS"]
    if not contiguous:
        raise ValueError(f"{name}: must be C-contiguous")
    if not hasattr(a, "data_ptr") and not a.flags["WRITEABLE"] and name.startswith("out"):
        raise ValueError(f"{name}: read-only array")
    return a


def _output_names(outputs, out):
    """The per-step outputs of a ``run``: those named, then those ``out`` brings a buffer for."""
    return list(outputs) + [k for k in (out or {}) if k not in outputs]


class BatchedHandle:
    """Base of the two batched environments.  ``PREFIX`` is the variant's symbol prefix; ``self._c.<name>`` is the library's
    ``PREFIX + name``, resolved once per handle for every name of ``SHARED_CALLS`` (nothing is looked up by string per call:
    ``run`` is on an agent loop's path).  A method of this class may call only what ``SHARED_CALLS`` lists, i.e. what both
    prefixes have; a function of one kind only (``orlg_launch_info``, ``orlg_phy_get_episode_stats``) stays in its class."""

    PREFIX = None
    SHARED_CALLS = ("create", "create_traffic", "create_trace", "destroy", "set_stream", "synchronize", "last_kernel", "reset",
                    "reseed", "trace_length", "trace_position", "get_requests", "get_counters", "get_current_time",
                    "get_num_running", "get_occupancy", "words_per_link", "state_size", "save_state", "load_state",
                    "get_traffic", "reduce_counters", "reduce_counters_grouped")

    # ------------------------------------------------------------------ the constructor's shared steps
    def _init_traffic_kwargs(self, trace, load, mean_service_holding_time, seed, seeds):
        """trace=: the handle replays a RequestTrace (trace.py) instead of generating its traffic; the arguments that describe
        generated traffic cannot be passed with it.  Returns (load, mean_service_holding_time) with the reference's defaults
        (``rmsa_env.py:31-32``)."""
        _trace.check_trace_kwargs(trace, dict(load=load, mean_service_holding_time=mean_service_holding_time, seed=seed,
                                              seeds=seeds))
        self.trace = trace
        return (10 if load is None else load,
                10800.0 if mean_service_holding_time is None else mean_service_holding_time)

    def _open(self, topology, batch_size, episode_length, load, mean_service_holding_time, bit_rates, continuous,
              bit_rate_probabilities, node_request_probabilities, seed, groups, num_groups):
        """Traffic, topology and trace are checked, THEN the library is loaded and bound; then the attributes and the
        selection tables both kinds have.  Returns (src_cum, dst_cum, bit_rate_cum)."""
        trace = self.trace
        # load= / mean_service_holding_time= may be length-B array-likes (a load sweep in one handle, traffic.py); with a trace
        # groups= stays: it feeds reduce_counters(by_group=True)
        self.traffic = SweepTraffic(batch_size, load, mean_service_holding_time, None if trace is not None else groups,
                                    None if trace is not None else num_groups)
        self.topology = t = FrozenTopology.from_graph(topology)
        if trace is not None:   # checked before the library is loaded: the rules of orlg_create_trace / orlg_phy_create_trace
            self.trace = trace = trace.for_batch(batch_size)
            trace.validate(num_nodes=t.num_nodes, **({"bit_rate_bounds": (bit_rates[0], bit_rates[-1])}
                                                     if continuous else {"bit_rates": list(bit_rates)}))
            self.traffic.groups, self.traffic.num_groups = _trace.trace_groups(batch_size, groups, num_groups)
            self._trace_groups = groups is not None
        self.L = _lib.load()
        self._c = SimpleNamespace(**{name: getattr(self.L, self.PREFIX + name) for name in self.SHARED_CALLS})
        self.batch_size = int(batch_size)
        self.episode_length = int(episode_length)
        self.k_paths = t.k_paths
        self.bit_rates = [int(b) for b in bit_rates]
        # optical_network_env.py:111-129
        self.load = load
        self.mean_service_holding_time = mean_service_holding_time
        if self.traffic.per_env:
            self.mean_service_inter_arrival_time = 1 / self.traffic.arrival_lambda
        else:
            self.mean_service_inter_arrival_time = 1 / float(load / float(mean_service_holding_time))
        self.loads, self.groups, self.num_groups = self.traffic.loads, self.traffic.groups, self.traffic.num_groups
        self.node_request_probabilities, src_cum, dst_cum, br_cum = selection_tables(
            node_request_probabilities, bit_rate_probabilities, t.num_nodes, self.bit_rates)
        self.rand_seed = 41 if seed is None else int(seed)  # optical_network_env.py:266-271
        self._keep = []
        return src_cum, dst_cum, None if continuous else br_cum   # (NULL: rng.randint, include/orlg.h)

    def _keep_array(self, a, dt):
        """Pointer of ``a`` as a contiguous array of ``dt`` that lives as long as the handle."""
        a = np.ascontiguousarray(a, dtype=dt)
        self._keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    def _topology_struct(self):
        t, ct = self.topology, _lib.Topology()
        ct.num_nodes, ct.num_links, ct.k_paths, ct.num_paths = t.num_nodes, t.num_links, t.k_paths, t.num_paths
        for name, dt in (("pair_path_base", np.int32), ("pair_path_count", np.int32), ("path_hops", np.int32),
                         ("path_se", np.int32), ("path_length", np.float64), ("path_link_off", np.int32),
                         ("path_links", np.int32)):
            setattr(ct, name, self._keep_array(getattr(t, name), dt))
        return ct

    def _fill_traffic(self, cc, src_cum, dst_cum, br_cum):
        """The fields both config structs have: the rates of ``expovariate(1 / mean)`` (``rmsa_env.py:646-651``) and the
        three cumulative tables."""
        if self.traffic.per_env:   # (ignored by the create_traffic functions; the pair of the largest load, for the record)
            cc.arrival_lambda = self.traffic.arrival_lambda[self.traffic.largest()]
            cc.holding_lambda = self.traffic.holding_lambda[self.traffic.largest()]
        else:
            cc.arrival_lambda = 1 / self.mean_service_inter_arrival_time
            cc.holding_lambda = 1 / self.mean_service_holding_time
        cc.bit_rates = self._keep_array(self.bit_rates, np.int32)
        cc.bit_rate_cum = None if br_cum is None else self._keep_array(br_cum, np.float64)
        cc.src_cum = self._keep_array(src_cum, np.float64)
        cc.dst_cum = self._keep_array(dst_cum, np.float64)

    def _create(self, ct, cc, seeds, device):
        """``create_trace`` / ``create_traffic`` / ``create`` of the variant: sets ``self.h``, ``self.device`` and
        ``self.words_per_link``."""
        seeds_ptr = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            if seeds.shape != (self.batch_size,):
                raise ValueError(f"seeds: shape {seeds.shape}, expected ({self.batch_size},)")
            seeds_ptr = seeds.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        head = (C.byref(ct), C.byref(cc), self.batch_size)
        if self.trace is not None:
            ts = self.trace.struct(self.groups if self._trace_groups else None, self.num_groups)
            _lib.check(self._c.create_trace(*head, int(device), C.byref(ts), C.byref(h)))
        elif self.traffic.per_env:
            tr = self.traffic.struct()
            _lib.check(self._c.create_traffic(*head, seeds_ptr, C.c_uint64(self.rand_seed), int(device), C.byref(tr),
                                              C.byref(h)))
        else:
            _lib.check(self._c.create(*head, seeds_ptr, C.c_uint64(self.rand_seed), int(device), C.byref(h)))
        self.h = h
        self.device = int(device)
        self.words_per_link = self._c.words_per_link(self.h)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "h", None):
            self._c.destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """Run on an existing HIP stream, e.g. ``torch.cuda.current_stream().cuda_stream``."""
        _lib.check(self._c.set_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def synchronize(self):
        _lib.check(self._c.synchronize(self.h))

    def last_kernel(self) -> str:
        """Name, template arguments and launch shape of the kernel behind the last ``run`` / ``reset``."""
        buf = C.create_string_buffer(160)
        _lib.check(self._c.last_kernel(self.h, buf, 160))
        return buf.value.decode()

    # ------------------------------------------------------------------ stepping
    def reset(self, only_episode_counters: bool = True):
        _lib.check(self._c.reset(self.h, 1 if only_episode_counters else 0))

    def reseed(self, seed=None, seeds=None):
        """A fresh ``random.Random`` for every environment -- ``seeds[i]`` if given, else ``seed + i`` (the constructor's
        convention) -- and nothing else changes: the pending requests stay, the next arrivals are the new generators' first
        draws.  NOT the reference's ``seed()``: there the bit-rate draw stays bound to the generator object of construction time
        (``functools.partial(self.rng.choices, ...)``, ``rmsa_env.py:109-111``), so after ``env.seed(s)`` the reference takes
        inter-arrival time, holding time, source and destination from ``Random(s)`` and the bit rate from the OLD generator
        (pinned by ``tests/golden/seed_rmsa_nsfnet_s10.npz``); here all five draws come from the new one.  A handle that
        replays a trace has no generator: ``ValueError``."""
        if self.trace is not None:
            raise ValueError("a handle that replays a trace has no generator to seed")
        if seeds is not None:
            sa = np.ascontiguousarray(seeds, np.uint64)
            if sa.shape != (self.batch_size,):
                raise ValueError(f"seeds: shape {sa.shape}, expected ({self.batch_size},)")
            _lib.check(self._c.reseed(self.h, _ptr(sa), 0))
        else:
            _lib.check(self._c.reseed(self.h, None, int(41 if seed is None else seed)))

    @property
    def trace_length(self) -> int:
        """Requests per environment of the handle's trace, 0 for a handle that generates its traffic."""
        return int(self._c.trace_length(self.h))

    @property
    def trace_position(self) -> int:
        """Requests drawn so far (the same for every environment): 1 after a full reset, + 1 per step."""
        return int(self._c.trace_position(self.h))

    def _step_outputs(self, names, n_steps, out, dtypes, shapes, io=None):
        """The per-step arrays of a ``run``, name -> [n_steps, B] + ``shapes.get(name, ())`` of ``dtypes[name]``: the
        caller's buffer from ``out`` where it brings one (checked: the library writes through its raw pointer), else a new numpy
        array.  With ``io`` every array's pointer goes into the field of its name."""
        res = {}
        for name in names:
            if name not in dtypes:
                raise KeyError(f"unknown step output {name!r}")
            shape = (n_steps, self.batch_size) + shapes.get(name, ())
            if out is not None and name in out:
                res[name] = _check_buffer(f"out[{name!r}]", out[name], shape, dtypes[name])
            else:
                res[name] = np.zeros(shape, dtype=dtypes[name])
            if io is not None:
                setattr(io, name, _ptr(res[name]))
        return res

    # ------------------------------------------------------------------ state read-back
    def _read(self, call, shape, dtype):
        a = np.zeros(shape, dtype)
        _lib.check(call(self.h, _ptr(a)))
        return a

    def requests(self):
        return self._read(self._c.get_requests, self.batch_size, REQUEST_DTYPE)

    def counters(self):
        a = self._read(self._c.get_counters, (self.batch_size, 8), np.int64)
        return {n: a[:, i].copy() for i, n in enumerate(COUNTER_NAMES)}

    def current_time(self):
        return self._read(self._c.get_current_time, self.batch_size, np.float64)

    def num_running(self):
        return self._read(self._c.get_num_running, self.batch_size, np.int32)

    def _occupancy_words(self):
        """[B, E, W] uint64, bit ``s`` of word ``w`` set = slot / channel ``64 w + s`` of the link is free."""
        return self._read(self._c.get_occupancy, (self.batch_size, self.topology.num_links, self.words_per_link), np.uint64)

    def save_state(self):
        """Snapshot of the complete simulation state of the batch (a uint8 array): checkpoint / resume, env cloning."""
        n = self._c.state_size(self.h)
        if n < 0:
            _lib.check(int(n))
        buf = np.empty(int(n), np.uint8)
        _lib.check(self._c.save_state(self.h, _ptr(buf)))
        return buf

    def load_state(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        assert buf.size == self._c.state_size(self.h), "snapshot of a differently configured batch"
        _lib.check(self._c.load_state(self.h, _ptr(buf)))

    def traffic_rates(self):
        """(arrival_lambda [B], holding_lambda [B], group [B]) as the handle holds them."""
        B = self.batch_size
        a, h, g = np.zeros(B), np.zeros(B), np.zeros(B, np.int32)
        _lib.check(self._c.get_traffic(self.h, _ptr(a), _ptr(h), _ptr(g)))
        return a, h, g

    def reduce_counters(self, by_group: bool = False):
        """Summed counters of this shard (raises if a release queue overflowed): the vector a
        multi-GPU job all-reduces.  ``by_group=True``: the sums per group of environments instead, [G, 16] int64 --
        columns 0..9 as the vector, 10 / 11 the sums of (processed - accepted)^2, all-time / episode (include/orlg.h)."""
        if by_group:
            return self._read(self._c.reduce_counters_grouped, (self.num_groups, 16), np.int64)
        a = self._read(self._c.reduce_counters, 16, np.int64)
        d = {n: int(a[i]) for i, n in enumerate(COUNTER_NAMES)}
        d["episodes_done"], d["num_envs"] = int(a[8]), int(a[9])
        return d, a
