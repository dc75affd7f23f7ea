"""BatchedPhyRMSAEnv: B independent QoT-aware environments (``PhyRMSAEnv``, ``phy_rmsa_env.py:20``) on one
MI355X: physical layer and virtual ("grooming") layer.  Constructor kwargs are the reference's
(``phy_rmsa_env.py:30-58``); ``modulation_level`` / ``gsnr`` are the ``(pairs, channels, k)`` tables and
``connections_detail`` the table's (source, destination) node numbers per row (an ``[rows, 2]`` int array, or the
reference's MATLAB object array).

Device policies (``run(policy, ...)``): ``bmfa`` / ``bmfa_rss`` (``phy_rmsa_env.py:1375,1441``; they consult the
virtual layer only when ``grooming=True``), ``sapff`` / ``bmff`` / ``sapbm`` / ``faff`` / ``faff_rss``
(``:1676,1317,1254,1508,1572``; they always try ``use_existing_channels`` first, like the reference) and ``external``.  ``defrag_period`` / ``number_moves`` / ``metric``
switch on the periodic defragmentation (``phy_rmsa_env.py:355-417``), run inside the step kernel.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._handle import BatchedHandle, _check_buffer, _output_names, _ptr

PHY_DEFAULT_BIT_RATES = (100, 200, 300, 400, 500, 600)  # phy_rmsa_env.py:38

EPISODE_STATS_DTYPE = np.dtype([("total_path_length", np.float64), ("total_gsnr", np.float64),
                                ("total_path_index", np.int64), ("total_modulation_level", np.int64),
                                ("channels_accepted", np.int64), ("physical_services_accepted", np.int64),
                                ("episodes_done", np.int64), ("queue_overflow", np.int64),
                                ("counted_moves", np.int64), ("counted_moves_groom", np.int64),
                                ("counted_defrag_cycles", np.int64)])


def _pairs_from_connections_detail(cd):
    cd = np.asarray(cd)
    if cd.dtype == object:  # scipy.io.loadmat cell array: column 0 / 1 hold 1x1 arrays
        return np.array([[int(np.asarray(r[0]).ravel()[0]), int(np.asarray(r[1]).ravel()[0])] for r in cd], np.int32)
    return np.ascontiguousarray(cd[:, :2], dtype=np.int32)


# the last 16 bytes of a continuous handle's saved state (orlg_phy_api.hip, ORLG_PHY_CONT_TAG0 / 1)
_CONT_STATE_TAG = np.array([0x796870206772726F, 0x34366620746E6F63], "<u8").view(np.uint8)


def _integral_bound(name, v):
    """rng.randint(lower, higher) takes integral values only (Python 3.10 accepts integral floats such as the reference's
    defaults 25.0 / 100.0)."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an integral number, got {v!r}") from None
    if not np.isfinite(f) or f != int(f):
        raise ValueError(f"{name} must be an integral number, got {v!r}")
    return int(f)


def continuous_bit_rate_bounds(bit_rate_selection, bit_rate_lower_bound, bit_rate_higher_bound, defrag_period):
    """The checks of ``phy_rmsa_env.py:79-86`` on the bit-rate kwargs, without a device: None for ``"discrete"``, else the
    integral (lower, higher) of ``rng.randint``."""
    if bit_rate_selection not in ("discrete", "continuous"):
        raise ValueError(f"bit_rate_selection must be 'discrete' or 'continuous', got {bit_rate_selection!r}")
    if bit_rate_selection == "discrete":
        return None
    lo = _integral_bound("bit_rate_lower_bound", bit_rate_lower_bound)
    hi = _integral_bound("bit_rate_higher_bound", bit_rate_higher_bound)
    if lo < 0 or hi < lo:
        raise ValueError(f"continuous bit rates need 0 <= bit_rate_lower_bound <= bit_rate_higher_bound, got {lo}..{hi}")
    if hi > 100 * _lib.PHY_MAX_CHANNELS:
        raise ValueError(f"bit_rate_higher_bound {hi} needs more than {_lib.PHY_MAX_CHANNELS} channels of 100 Gb/s")
    if defrag_period:
        raise ValueError("the periodic defragmentation (defrag_period) is not supported with continuous bit rates")
    return lo, hi


def encode_channels(selected_channels, out_row):
    """The reference's ``selected_channels`` tuples ``(channel, used, free, capacity, virtual)`` (``phy_rmsa_env.py:
    1364-1366``) -> one ``act_channels`` row: channel | used << 9 (``used`` in 100 Gb/s units; bare ints = whole channel)."""
    out_row[:] = -1
    for q, c in enumerate(selected_channels):
        if isinstance(c, (tuple, list, np.ndarray)):
            out_row[q] = int(c[0]) | (int(round(float(c[1]))) << 9 if len(c) > 1 else 0)
        else:
            out_row[q] = int(c)
    return out_row


def encode_shares(selected_channels, out_row):
    """Continuous bit rates: the tuples' float64 (used, free) fields -> one ``act_share`` row [14, 2] (0 padded)."""
    out_row[:] = 0.0
    for q, c in enumerate(selected_channels):
        out_row[q, 0], out_row[q, 1] = float(c[1]), float(c[2])
    return out_row


# per-step outputs wider than [n_steps, B]; the float64 shares of a continuous handle leave through orlg_phy_step_ex's own
# arguments, not through the orlg_phy_step_io
_STEP_IO_SHAPES = {"request": (4,), "channels": (_lib.PHY_MAX_CHANNELS,), "channels_used": (_lib.PHY_MAX_CHANNELS,),
                   "defrag_counters": (3,), "channels_used_f64": (_lib.PHY_MAX_CHANNELS,),
                   "channels_free_f64": (_lib.PHY_MAX_CHANNELS,)}
_F64_OUTPUTS = {"channels_used_f64": "float64", "channels_free_f64": "float64"}


class BatchedPhyRMSAEnv(BatchedHandle):
    PREFIX = "orlg_phy_"

    def __init__(self, topology, batch_size: int, *, modulation_level, connections_detail, gsnr,
                 episode_length: int = 1000, load: float = None, mean_service_holding_time: float = None,
                 bit_rates: Sequence[int] = PHY_DEFAULT_BIT_RATES, bit_rate_probabilities=None,
                 node_request_probabilities=None, seed: Optional[int] = None, seeds=None,
                 allow_rejection: bool = False, number_spectrum_channels: int = 80,
                 number_spectrum_channels_s_band: int = 108, l_band: bool = True, s_band: bool = True,
                 defrag_period=None, number_moves=None, metric: str = "cut", grooming: bool = False,
                 queue_capacity: int = 0, channel_state_capacity: int = 0, defrag_capacity: int = 0, device: int = 0,
                 gn_gate=None, bit_rate_selection: str = "discrete", bit_rate_lower_bound=25.0,
                 bit_rate_higher_bound=100.0, groups=None, num_groups=None, trace=None, **_ignored):
        load, mean_service_holding_time = self._init_traffic_kwargs(trace, load, mean_service_holding_time, seed, seeds)
        if defrag_period and number_moves is None:
            raise ValueError("defrag_period needs number_moves (the reference compares against it, phy_rmsa_env.py:358)")
        # bit_rate_selection="continuous" (phy_rmsa_env.py:79-86, 114-134): rng.randint(lower, higher) per request, checked
        # before the library is loaded
        bounds = continuous_bit_rate_bounds(bit_rate_selection, bit_rate_lower_bound, bit_rate_higher_bound, defrag_period)
        self.bit_rate_selection = bit_rate_selection
        self.continuous = bounds is not None
        if self.continuous:
            self.bit_rate_lower_bound, self.bit_rate_higher_bound = bounds
            bit_rates = range(bounds[0], bounds[1] + 1)
            bit_rate_probabilities = None
        tables = self._open(topology, batch_size, episode_length, load, mean_service_holding_time, bit_rates,
                            self.continuous, bit_rate_probabilities, node_request_probabilities, seed, groups, num_groups)
        t = self.topology
        self.allow_rejection = bool(allow_rejection)
        # optical_network_env.py:78-102
        if s_band:
            self.num_channels = 2 * number_spectrum_channels + number_spectrum_channels_s_band
        elif l_band:
            self.num_channels = 2 * number_spectrum_channels
        else:
            self.num_channels = number_spectrum_channels
        mod = np.ascontiguousarray(modulation_level, dtype=np.uint8)
        gs = np.ascontiguousarray(gsnr, dtype=np.float64)
        assert mod.shape == gs.shape and mod.shape[1] >= self.num_channels
        if mod.shape[1] != self.num_channels:
            mod, gs = np.ascontiguousarray(mod[:, :self.num_channels]), np.ascontiguousarray(gs[:, :self.num_channels])
        pairs = _pairs_from_connections_detail(connections_detail)
        adj_off, adj_link, adj_weight = t.cut_adjacency()

        keep = self._keep_array
        cc = _lib.PhyConfig()
        cc.num_channels, cc.episode_length, cc.num_bit_rates = self.num_channels, self.episode_length, len(self.bit_rates)
        cc.k_table, cc.num_table_rows, cc.queue_capacity = mod.shape[2], mod.shape[0], int(queue_capacity)
        cc.grooming, cc.channel_state_capacity = (1 if grooming else 0), int(channel_state_capacity)
        self.grooming = bool(grooming)
        cc.defrag_period, cc.number_moves = int(defrag_period or 0), int(number_moves or 0)
        cc.defrag_metric, cc.defrag_capacity = (0 if metric == "cut" else 1), int(defrag_capacity)
        self.defrag_period, self.number_moves, self.metric = defrag_period, number_moves, metric
        self._fill_traffic(cc, *tables)
        cc.pair_table_row = keep(t.pair_table_rows(pairs), np.int32)
        cc.modulation_level = keep(mod, np.uint8)
        cc.gsnr = keep(gs, np.float64)
        cc.adj_off, cc.adj_link, cc.adj_weight = keep(adj_off, np.int32), keep(adj_link, np.int32), keep(adj_weight, np.int32)
        # the cut metric as byte dot products over per-node free degrees (networks of at most 16 nodes); ORLG_PHY_NODEVEC=0
        # keeps the adjacency-list evaluation (identical results: tests/test_gpu_phy.py runs both)
        nv = t.cut_node_tables() if os.environ.get("ORLG_PHY_NODEVEC", "1") != "0" else None
        if nv is not None:
            cc.path_node_weights, cc.node_degree = keep(nv[0], np.uint8), keep(nv[1], np.uint8)
            cc.link_ends = keep(np.asarray(t.link_ends, np.int32).reshape(-1, 2), np.int32)
        # GN-model admission check of the chosen channels (osnr.gn_gate_parameters; not in the reference: include/orlg.h)
        self.gn_gate = gn_gate
        if gn_gate is not None:
            gg = _lib.GnGate()
            gg.launch_power_w = float(gn_gate["launch_power_w"])
            gg.channel_bandwidth_hz = float(gn_gate["channel_bandwidth_hz"])
            gg.attenuation_normalized = float(gn_gate["attenuation_normalized"])
            gg.noise_figure = float(gn_gate["noise_figure"])
            cf = np.ascontiguousarray(gn_gate["channel_center_frequency_hz"], np.float64)
            ns, sl = np.ascontiguousarray(gn_gate["link_num_spans"], np.int32), np.ascontiguousarray(gn_gate["link_span_length_km"], np.float64)
            if cf.shape != (self.num_channels,) or ns.shape != (t.num_links,) or sl.shape != (t.num_links,):
                raise ValueError("gn_gate: channel_center_frequency_hz [num_channels], link_num_spans / link_span_length_km [num_links]")
            gg.channel_center_frequency_hz, gg.link_num_spans, gg.link_span_length_km = keep(cf, np.float64), keep(ns, np.int32), keep(sl, np.float64)
            thr = np.ascontiguousarray(gn_gate["thresholds_db"], np.float64)
            gg.thresholds_db, gg.num_thresholds = keep(thr, np.float64), len(thr)
            self._keep.append(gg)
            cc.gn_gate = C.cast(C.pointer(gg), C.c_void_p)
        self._create(self._topology_struct(), cc, seeds, device)
        self.node_vectors = bool(self.L.orlg_phy_node_vectors(self.h))   # cut metric through node-degree vectors (include/orlg.h)

    def run(self, policy: str, n_steps: int = 1, *, act_path=None, act_channels=None, act_share=None,
            auto_reset: bool = False, outputs: Sequence[str] = (), out=None, cause_counts=None):
        """``n_steps`` x (policy -> PhyRMSAEnv.step).  ``policy='external'``: ``act_path`` [B] int32 (-2 = blocked,
        0..k-1 physical, 20 + k-path virtual layer) and ``act_channels`` [B, 14] int16 (-1 padded; entry = channel |
        used << 9, see :func:`encode_channels`).  Returns the requested per-step arrays [n_steps, B(, ...)]; ``out`` may
        supply preallocated numpy arrays or torch tensors by name (device tensors are written without staging).

        Continuous bit rates: external actions also need ``act_share`` [B, 14, 2] float64, the (used, free) fields of the
        tuples (:func:`encode_shares`); the outputs ``channels_used_f64`` / ``channels_free_f64`` [n_steps, B, 14] hold the
        chosen channels' float64 shares (``channels_used`` is 0 on such a handle).

        ``cause_counts`` / the output ``"block_cause"`` belong to the slot-based environments (``BatchedRMSAEnv.run``): channel
        allocation is not contiguous here, and the taxonomy of contiguous windows does not apply."""
        if (cause_counts is not None and cause_counts is not False) or "block_cause" in _output_names(outputs, out):
            raise ValueError("the blocking cause (block_cause, cause_counts) is defined for BatchedRMSAEnv / BatchedDeepRMSAEnv: "
                             "the QoT-aware environment allocates non-contiguous channels")
        B = self.batch_size
        io = _lib.PhyStepIO()
        names = _output_names(outputs, out)
        f64 = [n for n in names if n in _F64_OUTPUTS]
        if f64 and not self.continuous:
            raise KeyError(f"step output {f64[0]!r} belongs to handles with continuous bit rates")
        res = self._step_outputs(f64, n_steps, out, _F64_OUTPUTS, _STEP_IO_SHAPES)
        fptr = {name: _ptr(a) for name, a in res.items()}
        res.update(self._step_outputs([n for n in names if n not in f64], n_steps, out, _lib.PHY_STEP_IO_DTYPES,
                                      _STEP_IO_SHAPES, io))
        ap = ac = None
        if policy == "external":
            if act_path is None or act_channels is None:
                raise ValueError("policy 'external' needs act_path and act_channels")
            # host arrays: integers only (as BatchedRMSAEnv.run), and every value must survive the cast to the ABI's types --
            # a float or an out-of-range entry is refused, not truncated or wrapped
            def _as(name, a, dt):
                a = np.asarray(a)
                if a.dtype.kind not in "iu":
                    raise TypeError(f"{name} must be an integer array, got {a.dtype}")
                info = np.iinfo(dt)
                if a.size and (a.min() < info.min or a.max() > info.max):
                    raise ValueError(f"{name} has values outside {np.dtype(dt).name}")
                return np.ascontiguousarray(a, dt)
            if not hasattr(act_path, "data_ptr"):
                act_path = _as("act_path", act_path, np.int32)
            if not hasattr(act_channels, "data_ptr"):
                act_channels = _as("act_channels", act_channels, np.int16)
            _check_buffer("act_path", act_path, (B,), np.int32)
            _check_buffer("act_channels", act_channels, (B, _lib.PHY_MAX_CHANNELS), np.int16)
            ap, ac = _ptr(act_path), _ptr(act_channels)
        if not self.continuous:
            if act_share is not None:
                raise ValueError("act_share belongs to handles with continuous bit rates")
            _lib.check(self.L.orlg_phy_step(self.h, _lib.PHY_POLICIES[policy], int(n_steps), ap, ac,
                                            1 if auto_reset else 0, C.byref(io)))
            return res
        sp = None
        if policy == "external":
            if act_share is None:
                raise ValueError("policy 'external' with continuous bit rates needs act_share (the tuples' float64 used, free)")
            if not hasattr(act_share, "data_ptr"):
                act_share = np.ascontiguousarray(act_share, np.float64)
            _check_buffer("act_share", act_share, (B, _lib.PHY_MAX_CHANNELS, 2), np.float64)
            sp = _ptr(act_share)
        _lib.check(self.L.orlg_phy_step_ex(self.h, _lib.PHY_POLICIES[policy], int(n_steps), ap, ac, sp,
                                           1 if auto_reset else 0, C.byref(io), fptr.get("channels_used_f64"),
                                           fptr.get("channels_free_f64")))
        return res

    def episode_stats(self):
        return self._read(self.L.orlg_phy_get_episode_stats, self.batch_size, EPISODE_STATS_DTYPE)

    def info(self):
        """The per-episode ratios of the info dict (``phy_rmsa_env.py:339-347``) for every env."""
        s = self.episode_stats()
        phys, chans = s["physical_services_accepted"], s["channels_accepted"]
        return {"total_path_length": s["total_path_length"] / (phys + 1),
                "avrage_gsnr": s["total_gsnr"] / (chans + 1),
                "average_mod_level": s["total_modulation_level"] / (chans + 1),
                "average_path_index": s["total_path_index"] / (phys + 1),
                "path_index": s["total_path_index"], "physical_paths": phys}

    def available_channels(self):
        """topology.graph["available_channels"] for every env: [B, E, C] uint8 (1 = free)."""
        bits = np.unpackbits(self._occupancy_words().view(np.uint8), axis=-1, bitorder="little")
        return bits.reshape(self.batch_size, self.topology.num_links, -1)[:, :, :self.num_channels]

    def channel_masks(self, out=None):
        """``is_channel_free(path_p, c)`` (``phy_rmsa_env.py:1029-1035``) for the k candidate paths of every env's pending
        request: [B, k, W] uint64, bit ``c`` of word ``w`` = channel ``64 w + c`` is dark on every link of the path; bits at
        and beyond the channel count are 0.  ``out`` may be a numpy array or a torch tensor (device and pinned host tensors
        are written in place).  Modulation levels, the bit rate and the virtual layer are not looked at."""
        shape = (self.batch_size, self.k_paths, self.words_per_link)
        if out is None:
            out = np.zeros(shape, np.uint64)
        else:
            _check_buffer("out", out, shape, np.uint64)
        _lib.check(self.L.orlg_phy_channel_masks(self.h, _ptr(out)))
        return out

    def channel_state(self, env_index: int = 0):
        """``env.channel_state`` of one env (``phy_rmsa_env.py:117-125``): dict (src_id, dst_id, k-path) -> list of
        (channel, used, free, capacity) tuples in list order (100 Gb/s units); empty lists are omitted."""
        t = self.topology
        lists = t.num_nodes * t.num_nodes * t.k_paths
        cap = self.L.orlg_phy_channel_state_capacity(self.h)
        ent = np.zeros((lists, cap), np.uint32)
        n = np.zeros(lists, np.uint8)
        rc = self.L.orlg_phy_get_channel_state(self.h, int(env_index), _ptr(ent), _ptr(n))
        if rc < 0:
            _lib.check(rc)
        out = {}
        if self.continuous:   # float64 (used, free): the reference's tuples hold floats in this mode
            ent = np.zeros((lists, cap, 4), np.float64)
            rc = self.L.orlg_phy_get_channel_state_f64(self.h, int(env_index), _ptr(ent), _ptr(n))
            if rc < 0:
                _lib.check(rc)
            for key in np.nonzero(n)[0]:
                s, rem = divmod(int(key), t.num_nodes * t.k_paths)
                d, k = divmod(rem, t.k_paths)
                out[(s, d, k)] = [(int(x[0]), float(x[1]), float(x[2]), int(x[3])) for x in ent[key, :n[key]]]
            return out
        for key in np.nonzero(n)[0]:
            e = ent[key, :n[key]].astype(np.int64)
            s, rem = divmod(int(key), t.num_nodes * t.k_paths)
            d, k = divmod(rem, t.k_paths)
            out[(s, d, k)] = [(int(x & 0x1ff), int((x >> 9) & 0x1f), int((x >> 14) & 0x1f), int((x >> 19) & 0x1f)) for x in e]
        return out

    def load_state(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        tagged = buf.size >= 16 and np.array_equal(buf[-16:], _CONT_STATE_TAG)
        if self.continuous or tagged:   # a snapshot of the other bit-rate mode is refused (ORLG_ERR_INVALID)
            _lib.check(self.L.orlg_phy_load_state_checked(self.h, _ptr(buf), C.c_int64(buf.size)))
            return
        super().load_state(buf)
