"""The CPU restatement of the GN-model audit of the running lightpaths (``include/orlg.h`` ``orlg_gn_audit``): for every
running service one check of ``oracle.gn_osnr`` over the links of its own path, its interferers per link the OTHER running services
whose path holds the link, in rank order (ascending release time).  The ASE and NLI parts are restated in NumPy with the oracle's
expressions (``examples/calculate_osnr.py:24-53``).  Helper module of ``test_gn_audit_args.py`` and ``test_gpu_gn_audit.py``; nothing
here touches a GPU.

A service is ``(links of its path in order, first slot, number of slots, spectral efficiency)``.
"""
import functools
import math

import numpy as np

import gn_protect_reference as pref
import oracle as orc
from conftest import load_topology
from gpu_support import device_log_in_oracle

B = pref.B
CHECKPOINTS = (0, 1, 2, 50, 200, 400, 600)
# the cases of the issue: gn_protect_reference.CASES' topologies, shapes, loads, policies and seeds
CASES = ("nsfnet_s100_l20_spff", "nsfnet_s320_l150_sapff", "jpn12_s320_l150_sapff", "ring34_s320_l300_llpff", "ring36_s512_l500_sapff")
LOADED_CASES = CASES[1:]
# a case's environments run on its seed + 0 .. 7: gn_protect_reference's seed, but ring36 moved from 11 to 22 -- with the device's
# logarithm its seed 18 audits a margin 7.2e-5 dB from zero (protecting handle, step 200), inside the 1e-4 dB the comparison of
# n_below needs (test_gn_audit_args.py asserts that none is)
SEEDS = dict({case: pref.CASES[case]["seed"] for case in CASES}, ring36_s512_l500_sapff=22)
PHI_MOD = (1, 1, 2 / 3, 17 / 25, 69 / 100, 13 / 21)


def audit(services, gate, topo=None):
    """dict(gsnr_db, margin_db, osnr_ase_db, snr_nli_db: [n] float64, n_running, n_below, min_margin_db, worst_rank) of the
    services, a list of (links, s, n, se) in rank order, under `gate`.  `topo` is not needed: a service carries its links."""
    g = gate
    D, f0, dens = g["slot_width_hz"], g["frequency_start_hz"], g["launch_power_density_w_hz"]
    att, nf = g["attenuation_normalized"], g["noise_figure"]
    n_svc = len(services)
    bw = np.array([n * D for _, _, n, _ in services], np.float64)
    fc = np.array([f0 + (s + n / 2) * D for _, s, n, _ in services], np.float64)
    se = np.array([e for _, _, _, e in services], np.int64)
    thr = np.array([float(g["thresholds_db"][e - 1]) for e in se], np.float64)
    by_link = {}
    for i, (links, _, _, _) in enumerate(services):   # rank order
        for l in links:
            by_link.setdefault(l, []).append(i)
    out = dict(gsnr_db=np.zeros(n_svc), margin_db=np.zeros(n_svc), osnr_ase_db=np.zeros(n_svc), snr_nli_db=np.zeros(n_svc))
    if n_svc:
        span_off, svc_off, clo, lengths, sb, sf, sse = [0], [0], [0], [], [], [], []
        for v, (links, _, _, _) in enumerate(services):
            for l in links:
                ns = int(g["link_num_spans"][l])
                lengths += [float(g["link_span_length_km"][l])] * ns
                span_off.append(len(lengths))
                for i in by_link[l]:
                    if i != v:
                        sb.append(bw[i]); sf.append(fc[i]); sse.append(int(se[i]))
                svc_off.append(len(sb))
            clo.append(len(span_off) - 1)
        n_sp = len(lengths)
        batch = dict(check_link_off=clo, link_span_off=span_off, link_svc_off=svc_off, bandwidth=bw, center_frequency=fc,
                     launch_power=dens * bw, span_length_km=lengths, span_attenuation=[att] * n_sp, span_noise_figure=[nf] * n_sp,
                     svc_bandwidth=sb, svc_center_frequency=sf, svc_se=sse, svc_is_self=[0] * len(sb))
        out["gsnr_db"] = np.asarray(orc.gn_osnr(batch), np.float64)
        out["margin_db"] = out["gsnr_db"] - thr
        # the two parts, calculate_osnr.py:24-53 in NumPy
        beta_2, gamma, h_plank, pi = -21.3e-27, 1.3e-3, 6.626e-34, math.pi
        l_eff_a = 1 / (2 * att)
        pm = np.array(PHI_MOD)[se - 1]
        for v, (links, _, _, _) in enumerate(services):
            acc_a = acc_n = 0.0
            pw = dens * bw[v]
            for l in links:
                length = float(g["link_span_length_km"][l])
                l_eff = (1 - np.exp(-2 * att * length * 1e3)) / (2 * att)
                sum_phi = math.asinh(pi ** 2 * abs(beta_2) * bw[v] ** 2 / (4 * att))
                idx = np.array([i for i in by_link[l] if i != v], np.int64)
                if idx.size:
                    df = fc[idx] - fc[v]
                    phi = (np.arcsinh(pi ** 2 * abs(beta_2) * l_eff_a * bw[idx] * (df + bw[idx] / 2))
                           - np.arcsinh(pi ** 2 * abs(beta_2) * l_eff_a * bw[idx] * (df - bw[idx] / 2))) \
                        - pm[idx] * (bw[idx] / np.abs(df)) * 5 / 3 * (l_eff / (length * 1e3))
                    sum_phi += float(np.sum(phi))
                p_nli = (pw / bw[v]) ** 3 * (8 / (27 * pi * abs(beta_2))) * gamma ** 2 * l_eff * sum_phi * bw[v]
                p_ase = bw[v] * h_plank * fc[v] * (math.exp(2 * att * length * 1e3) - 1) * nf
                ns = int(g["link_num_spans"][l])
                acc_a += ns * (p_ase / pw)
                acc_n += ns * (p_nli / pw)
            out["osnr_ase_db"][v] = 10 * np.log10(1 / acc_a)
            out["snr_nli_db"][v] = 10 * np.log10(1 / acc_n)
    m = out["margin_db"]
    out.update(n_running=n_svc, n_below=int((m < 0).sum()), min_margin_db=float(m.min()) if n_svc else np.nan,
               worst_rank=int(np.argmin(m)) if n_svc else -1)
    return out


def _slots(b, gate):
    return int(round(b / gate["slot_width_hz"]))


def services_of_shadow(shadow, gate):
    """The services of a ``ProtectingOracle.shadow`` -- (release, link set, centre, bandwidth, SE, ordered links) in provision order --
    sorted by release time: [(links, s, n, se)], and the sorted shadow entries next to them."""
    order = sorted(range(len(shadow)), key=lambda i: shadow[i][0])   # (stable; release times are distinct draws)
    D, f0 = gate["slot_width_hz"], gate["frequency_start_hz"]
    svc = []
    for i in order:
        _, _, f, b, se, links = shadow[i]
        n = _slots(b, gate)
        s = int(round((f - f0) / D - n / 2))
        svc.append((tuple(links), s, n, int(se)))
    return svc, [shadow[i] for i in order]


def path_links(topo, gid):
    return tuple(int(l) for l in topo.path_links[topo.path_link_off[gid]:topo.path_link_off[gid + 1]])


def services_of_running(run, i, topo):
    """The services of environment `i` of ``BatchedRMSAEnv.running_services()``: [(links, s, n, se)] in rank order."""
    n = int(run["count"][i])
    return [(path_links(topo, int(run["path_gid"][i, r])), int(run["slot"][i, r]), int(run["num_slots"][i, r]),
             int(topo.path_se[int(run["path_gid"][i, r])])) for r in range(n)]


def run_checkpoints(case, seed, protect, checkpoints=CHECKPOINTS):
    """One oracle environment of a case behind the gate (protect=False: GatedOracle's decisions, on a ProtectingOracle's shadow,
    which carries the ordered links) stepped to every checkpoint: {steps: dict(services, release, path, bit_rate, audit)} -- the
    state BETWEEN launches, the services due at the pending request's arrival dropped.  Run once per process and shared; read-only
    by agreement."""
    return _run_checkpoints(case, seed, bool(protect), tuple(checkpoints))


class AuditOracle(pref.ProtectingOracle):
    """The protecting oracle, or (protect=False) the gated one on the same shadow, which carries the ordered links: there the
    candidate's own check decides alone.  Remembers (bit rate, global path index) of every admitted service by its release time."""

    def __init__(self, *a, protect=True, **k):
        super().__init__(*a, **k)
        self.protect, self.admitted = protect, {}

    def neighbour_margin(self, links, s, n, se):
        return super().neighbour_margin(links, s, n, se) if self.protect else (np.nan, 0)

    def step(self, p, s):
        r, t = self.o.request(), self.topo
        row = super().step(p, s)
        if row["accepted"]:
            gid = int(t.pair_path_base[r.src * t.num_nodes + r.dst]) + p
            self.admitted[r.arrival_time + r.holding_time] = (int(r.bit_rate), gid)
        return row


@functools.lru_cache(maxsize=None)
def _run_checkpoints(case, seed, protect, checkpoints):
    c = pref.CASES[case]
    topo = load_topology(c["topology"])
    gate = pref.case_gate(topo, protect=protect)
    res = {}
    with device_log_in_oracle():
        po = AuditOracle(topo, pref.case_kwargs(case), gate, seed=seed, protect=protect)
        done = 0
        for at in checkpoints:
            while done < at:
                po.step(*po.propose(c["policy"]))
                done += 1
            po._drop_due()   # the state between launches holds no service due at the pending request's arrival
            svc, entries = services_of_shadow(po.shadow, gate)
            res[at] = dict(services=svc, release=np.array([e[0] for e in entries], np.float64),
                           bit_rate=np.array([po.admitted[e[0]][0] for e in entries], np.int64),
                           path_gid=np.array([po.admitted[e[0]][1] for e in entries], np.int64), audit=audit(svc, gate))
        po.close()
    return res
