"""GN-model GSNR admission check on the device (``examples/calculate_osnr.py:9-56``): ``gn_osnr(batch)``.

``batch`` is a dict of flat arrays (see ``include/orlg.h`` ``orlg_osnr_batch``); :func:`flatten_checks` builds it from
reference-style objects (``current_service.path.links``, ``link.spans``, ``running_services``).  The modulation-format
thresholds the QoT tables were built with are in :data:`TABLE_THRESHOLDS_DB`.
"""
import ctypes as C

import numpy as np

from . import _lib

FIELDS = (("check_link_off", np.int32), ("link_span_off", np.int32), ("link_svc_off", np.int32),
          ("bandwidth", np.float64), ("center_frequency", np.float64), ("launch_power", np.float64),
          ("span_length_km", np.float64), ("span_attenuation", np.float64), ("span_noise_figure", np.float64),
          ("svc_bandwidth", np.float64), ("svc_center_frequency", np.float64), ("svc_se", np.int32),
          ("svc_is_self", np.uint8))

# Modulation_connection == #{t in T : GSNR >= t} for the shipped US14 / JPN12 tables: open intervals
TABLE_THRESHOLDS_DB = ((3.940023, 3.941195), (6.951155, 6.951439), (11.048567, 11.048630), (13.484332, 13.484535),
                       (16.416199, 16.416316), (19.280312, 19.280709))


class OsnrBatch(C.Structure):
    _fields_ = [("num_checks", C.c_int32), ("num_links", C.c_int32), ("num_spans", C.c_int32), ("num_services", C.c_int32)] + \
               [(n, C.c_void_p) for n, _ in FIELDS]


def validate_batch(batch):
    """Raise ``ValueError`` for a batch the kernel must not be given (the caller's contract of ``orlg_gn_osnr`` in
    ``include/orlg.h``): the device follows the offsets without checking them, and the routine is undefined for an interferer
    on the service's own frequency (division by ``|f - fc| = 0``), for two own entries in one list and for a spectral
    efficiency outside the six the modulation-factor table has.  Pure numpy: runs before the library is loaded."""
    a = {name: np.asarray(batch[name]) for name, _ in FIELDS}
    for name in a:
        if a[name].ndim != 1:
            raise ValueError(f"{name} must be one-dimensional, got shape {a[name].shape}")
    for fam in (("bandwidth", "center_frequency", "launch_power"), ("span_length_km", "span_attenuation", "span_noise_figure"),
                ("svc_bandwidth", "svc_center_frequency", "svc_se", "svc_is_self"), ("link_span_off", "link_svc_off")):
        sizes = {n: a[n].size for n in fam}
        if len(set(sizes.values())) != 1:
            raise ValueError("arrays of one family differ in length: " + ", ".join(f"{n}={s}" for n, s in sizes.items()))
    num_links = a["link_span_off"].size - 1
    if num_links < 0:
        raise ValueError("link_span_off and link_svc_off are empty: offset arrays hold one entry more than they have ranges")
    if a["check_link_off"].size != a["bandwidth"].size + 1:
        raise ValueError(f"check_link_off has {a['check_link_off'].size} entries for {a['bandwidth'].size} checks: "
                         "offset arrays hold one entry more than they have ranges")
    for name, end, what in (("check_link_off", num_links, "links"), ("link_span_off", a["span_length_km"].size, "spans"),
                            ("link_svc_off", a["svc_bandwidth"].size, "list entries")):
        off = a[name].astype(np.int64)
        if off[0] != 0:
            raise ValueError(f"{name} does not start at 0 (starts at {off[0]})")
        if np.any(np.diff(off) < 0):
            raise ValueError(f"{name} does not ascend (at index {int(np.argmax(np.diff(off) < 0)) + 1})")
        if off[-1] != end:
            raise ValueError(f"{name} ends at {off[-1]}, not at the number of {what} ({end})")
    own = a["svc_is_self"] != 0
    se = a["svc_se"]
    bad = ~own & ((se < 1) | (se > 6))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"svc_se outside 1..6: svc_se[{i}] = {se[i]}")
    svc_off = a["link_svc_off"].astype(np.int64)
    own_before = np.concatenate(([0], np.cumsum(own)))
    own_per_link = own_before[svc_off[1:]] - own_before[svc_off[:-1]]
    if np.any(own_per_link > 1):
        l = int(np.argmax(own_per_link > 1))
        raise ValueError(f"more than one self entry in the list of link {l} ({int(own_per_link[l])})")
    link_of_svc = np.repeat(np.arange(num_links), np.diff(svc_off))
    check_of_link = np.repeat(np.arange(a["bandwidth"].size), np.diff(a["check_link_off"].astype(np.int64)))
    same = ~own & (a["svc_center_frequency"] == a["center_frequency"][check_of_link[link_of_svc]])
    if same.any():
        i = int(np.argmax(same))
        raise ValueError(f"a non-self entry sits on the center_frequency of its check: svc_center_frequency[{i}] = "
                         f"{a['svc_center_frequency'][i]} (link {int(link_of_svc[i])}, check {int(check_of_link[link_of_svc[i]])})")


def gn_osnr(batch, device: int = 0, stream_ptr=None):
    """GSNR [dB] per admission check; numpy arrays in, numpy array out (computed on the GPU).  A malformed batch
    (:func:`validate_batch`) raises ``ValueError`` before anything is launched."""
    validate_batch(batch)
    L = _lib.load()
    L.orlg_gn_osnr.argtypes = [C.POINTER(OsnrBatch), C.c_void_p, C.c_int32, C.c_void_p]
    b = OsnrBatch()
    keep = []
    for name, dt in FIELDS:
        a = np.ascontiguousarray(batch[name], dtype=dt)
        keep.append(a)
        setattr(b, name, a.ctypes.data_as(C.c_void_p))
    b.num_checks = len(batch["bandwidth"])
    b.num_links = len(batch["link_span_off"]) - 1
    b.num_spans = len(batch["span_length_km"])
    b.num_services = len(batch["svc_bandwidth"])
    out = np.zeros(b.num_checks)
    _lib.check(L.orlg_gn_osnr(C.byref(b), out.ctypes.data_as(C.c_void_p), int(device),
                              C.c_void_p(stream_ptr) if stream_ptr else None))
    return out


def modulation_level_from_gsnr(gsnr_db, thresholds=None):
    """Number of thresholds met = table modulation level (0 = unusable)."""
    t = np.array([0.5 * (a + b) for a, b in (thresholds or TABLE_THRESHOLDS_DB)])
    return (np.asarray(gsnr_db)[..., None] >= t).sum(axis=-1).astype(np.uint8)


def gn_gate_parameters(topology, num_channels=268, *, launch_power_dbm=0.0, channel_spacing_hz=50e9,
                       first_center_frequency_hz=184.5e12, max_span_length_km=80.0, attenuation_db_km=0.2,
                       noise_figure_db=4.5, thresholds_db=None):
    """Parameters of the GN-model admission check of ``BatchedPhyRMSAEnv(..., gn_gate=...)`` (``include/orlg.h``
    ``orlg_gn_gate``): a plain dict of numbers / arrays, physical defaults of ``examples/create_topology_gn.py``.

    * spans: ``int(length // 80) + 1`` equal spans per link (``create_topology_gn.py:122-125``), 0.2 dB/km, NF 4.5 dB;
      ``attenuation_normalized = att_dB_km / (2 * 10 * log10(e) * 1e3)`` [1/m] and ``noise_figure = 10 ** (NF_dB / 10)`` are
      the conventions stated for the stand-alone routine (the reference leaves them undefined);
    * channels: a uniform grid ``f0 + index * spacing``, every channel ``spacing`` wide (L, C, S bands = 268 channels);
    * thresholds: the GSNR levels the shipped QoT tables were built with (midpoints of :data:`TABLE_THRESHOLDS_DB`).
    """
    from .topology import FrozenTopology
    t = FrozenTopology.from_graph(topology)
    lengths = np.array([float(e[4]) for e in t.edges], np.float64)[np.argsort([int(e[2]) for e in t.edges])]
    nspans = (lengths // max_span_length_km).astype(np.int32) + 1
    thr = thresholds_db if thresholds_db is not None else [0.5 * (a + b) for a, b in TABLE_THRESHOLDS_DB]
    return {
        "launch_power_w": 1e-3 * 10 ** (launch_power_dbm / 10.0),
        "channel_bandwidth_hz": float(channel_spacing_hz),
        "attenuation_normalized": attenuation_db_km / (2 * 10 * np.log10(np.e) * 1e3),
        "noise_figure": 10 ** (noise_figure_db / 10.0),
        "channel_center_frequency_hz": first_center_frequency_hz + channel_spacing_hz * np.arange(num_channels, dtype=np.float64),
        "link_num_spans": nspans,
        "link_span_length_km": lengths / nspans,
        "thresholds_db": np.asarray(sorted(thr), np.float64),
    }


def rmsa_gn_gate_parameters(topology, *, launch_power_dbm_per_50ghz=0.0, frequency_start_hz=191.7e12, channel_width=12.5,
                            max_span_length_km=80.0, attenuation_db_km=0.2, noise_figure_db=4.5, thresholds_db=None, protect_running=False,
                            modulation="path"):
    """Parameters of the GN-model admission check of ``BatchedRMSAEnv(..., gn_gate=...)`` / ``BatchedDeepRMSAEnv``
    (``include/orlg.h`` ``orlg_rmsa_gn_gate``): a plain dict of numbers / arrays.

    * slot grid: slot width ``channel_width`` GHz, lower edge of slot 0 at ``frequency_start_hz``; a service on the window
      ``[s, s + n)`` is ``n`` slots wide around ``frequency_start_hz + (s + n / 2) * width``;
    * launch power: a constant power spectral density, ``launch_power_dbm_per_50ghz`` dBm in every 50 GHz --
      ``1e-3 * 10 ** (dBm / 10) / 50e9`` W/Hz;
    * spans, attenuation, noise figure and the default thresholds: the conventions of :func:`gn_gate_parameters`;
    * ``protect_running=True`` adds the key ``"protect_running"``: the gate also refuses a candidate that would push a running
      lightpath on a shared link below the threshold of its modulation (``orlg_set_gn_protect``).  Without it the
      dict has exactly the eight keys above.
    * ``modulation="adaptive"`` adds the key ``"modulation"``: the gate reads ``thresholds_db`` as the reference's ``modulation_level``
      table reads a GSNR -- level ``m`` = spectral efficiency ``m`` needs ``thresholds_db[m - 1]`` -- and the policies of
      ``ADAPTIVE_POLICIES`` run a service at the highest level its GSNR meets (``orlg_set_gn_modulation``).  The
      default ``"path"``: every service runs at its path's reach-table spectral efficiency, and the dict has no such key.
    """
    if modulation not in ("path", "adaptive"):
        raise ValueError(f"modulation {modulation!r}: expected 'path' or 'adaptive'")
    from .topology import FrozenTopology
    t = FrozenTopology.from_graph(topology)
    lengths = np.array([float(e[4]) for e in t.edges], np.float64)[np.argsort([int(e[2]) for e in t.edges])]
    nspans = (lengths // max_span_length_km).astype(np.int32) + 1
    thr = thresholds_db if thresholds_db is not None else [0.5 * (a + b) for a, b in TABLE_THRESHOLDS_DB]
    g = {
        "launch_power_density_w_hz": 1e-3 * 10 ** (launch_power_dbm_per_50ghz / 10.0) / 50e9,
        "frequency_start_hz": float(frequency_start_hz),
        "slot_width_hz": float(channel_width) * 1e9,
        "attenuation_normalized": attenuation_db_km / (2 * 10 * np.log10(np.e) * 1e3),
        "noise_figure": 10 ** (noise_figure_db / 10.0),
        "link_num_spans": nspans,
        "link_span_length_km": lengths / nspans,
        "thresholds_db": np.asarray(sorted(thr), np.float64),
    }
    if protect_running:
        g["protect_running"] = True
    if modulation == "adaptive":
        g["modulation"] = "adaptive"
    return g


RMSA_GN_GATE_SCALARS = ("launch_power_density_w_hz", "frequency_start_hz", "slot_width_hz", "attenuation_normalized", "noise_figure")


def check_rmsa_gn_gate(gate, topology, step_kernel="auto"):
    """The rules of ``orlg_set_gn_gate`` as ``ValueError``s, before the library is loaded: returns the gate as a dict of floats
    and contiguous arrays."""
    from .topology import FrozenTopology
    if step_kernel == "group":
        raise ValueError("gn_gate: the admission check is served by the wave-per-environment kernel, not by step_kernel='group'")
    t = FrozenTopology.from_graph(topology)
    g = {}
    for name in RMSA_GN_GATE_SCALARS:
        v = float(gate[name])
        if not np.isfinite(v) or not v > 0:
            raise ValueError(f"gn_gate: {name} must be finite and positive, got {v}")
        g[name] = v
    g["link_num_spans"] = ns = np.ascontiguousarray(gate["link_num_spans"], np.int32)
    g["link_span_length_km"] = sl = np.ascontiguousarray(gate["link_span_length_km"], np.float64)
    g["thresholds_db"] = thr = np.ascontiguousarray(gate["thresholds_db"], np.float64)
    if ns.shape != (t.num_links,) or sl.shape != (t.num_links,):
        raise ValueError(f"gn_gate: link_num_spans / link_span_length_km must have shape ({t.num_links},), got {ns.shape} / {sl.shape}")
    if (ns < 1).any() or not np.isfinite(sl).all() or (sl <= 0).any():
        raise ValueError("gn_gate: link_num_spans must be >= 1 and link_span_length_km finite and positive")
    if thr.ndim != 1 or thr.size < 1 or not np.isfinite(thr).all():
        raise ValueError("gn_gate: thresholds_db must be a non-empty one-dimensional array of finite values")
    se_max = int(np.max(t.path_se))
    if se_max > thr.size:
        raise ValueError(f"gn_gate: a path has spectral efficiency {se_max}, thresholds_db has {thr.size} entries")
    if gate.get("protect_running"):   # (carried only when asked for)
        g["protect_running"] = True
    mode = gate.get("modulation", "path")
    if mode not in ("path", "adaptive"):
        raise ValueError(f"gn_gate: modulation {mode!r}: expected 'path' or 'adaptive'")
    if mode == "adaptive":   # the rules of orlg_set_gn_modulation
        from ._lib import MAX_ADAPTIVE_PATHS, MAX_MODULATION_LEVELS
        if g.get("protect_running"):
            raise ValueError("gn_gate: modulation='adaptive' with protect_running: the modulation is not chosen behind the check of the "
                             "running lightpaths yet")
        if thr.size > MAX_MODULATION_LEVELS:
            raise ValueError(f"gn_gate: modulation='adaptive' with {thr.size} thresholds: the levels are spectral efficiencies "
                             f"1..{MAX_MODULATION_LEVELS}, where the modulation factors of the GN model end")
        if t.num_paths >= MAX_ADAPTIVE_PATHS:
            raise ValueError(f"gn_gate: modulation='adaptive' on a topology with {t.num_paths} path records: a service's level takes 3 "
                             f"bits of its descriptor's path field, which leaves room for {MAX_ADAPTIVE_PATHS - 1}")
        g["modulation"] = "adaptive"
    return g
