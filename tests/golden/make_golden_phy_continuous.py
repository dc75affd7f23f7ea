#!/usr/bin/env python3
"""Generate the PhyRMSA fixtures with continuous bit rates (``bit_rate_selection="continuous"``) by running the
UNMODIFIED reference, like make_golden.py (whose trace recorder and table loaders this script imports).

    python tests/golden/make_golden_phy_continuous.py [--case NAME]

Outputs cont_*.npz: the per-step traces of run_phy_trace.  ``ch_used`` / ``ch_free`` are the float64 shares the
reference computes (``channel[0] + unassigned / 100``, ``candidate[2] + unassigned / 100``, ...): they pin the device's
operation order, not only its decisions.
"""
import argparse
import json
import os

import numpy as np

from make_golden import (HERE, PHY_BASE, PHY_TABLES, TOPOLOGIES, _jsonable, install_gym_stub, load_phy_tables,
                         load_pickled_topology, run_phy_trace)

CONT = dict(bit_rate_selection="continuous")
CASES = [
    # (name, tables, env kwargs over PHY_BASE, policy, steps): the default bounds 25..100 -- shares of ONE channel
    ("cont_us14_s20_sapff", "us14_k3", dict(seed=20), "sapff", 600),
    ("cont_us14_s21_bmff", "us14_k3", dict(seed=21), "bmff", 600),
    ("cont_us14_s22_sapbm", "us14_k3", dict(seed=22), "sapbm", 600),
    ("cont_us14_s23_faff", "us14_k3", dict(seed=23), "faff", 600),
    ("cont_us14_s24_bmfa", "us14_k3", dict(seed=24), "bmfa", 600),
    ("cont_us14_s25_bmfa_groom", "us14_k3", dict(seed=25, grooming=True), "bmfa", 600),
    ("cont_us14_s26_bmfa_rss_groom", "us14_k3", dict(seed=26, grooming=True), "bmfa_rss", 600),
    # 100..600: services over several channels with a partial last one
    ("cont_us14_s27_sapbm_100_600", "us14_k3", dict(seed=27, bit_rate_lower_bound=100, bit_rate_higher_bound=600),
     "sapbm", 600),
    ("cont_us14_s28_faff_rss_100_600", "us14_k3", dict(seed=28, bit_rate_lower_bound=100, bit_rate_higher_bound=600),
     "faff_rss", 600),
    # a load that blocks
    ("cont_us14_s29_sapff_100_600_load20000", "us14_k3",
     dict(seed=29, load=20000, bit_rate_lower_bound=100, bit_rate_higher_bound=600), "sapff", 1500),
    ("cont_jpn12_s30_bmff", "jpn12_k3", dict(seed=30, load=900), "bmff", 600),
]
MUST_BLOCK = {"cont_us14_s29_sapff_100_600_load20000"}


def gen(name, tab, over, policy, steps):
    kw = dict(PHY_BASE, **CONT)
    kw.update(over)
    topo = load_pickled_topology(TOPOLOGIES[PHY_TABLES[tab][2]])
    out = run_phy_trace(topo, load_phy_tables(tab), kw, policy, steps, True)
    acc = int(out["services_accepted"][-1])
    if name in MUST_BLOCK:
        assert acc < steps, (name, acc)
    frac = np.count_nonzero(out["ch_used"] * 100 != np.round(out["ch_used"] * 100))
    meta = dict(topology=PHY_TABLES[tab][2], tables=tab, env_kwargs=_jsonable(kw), policy=policy, steps=steps,
                reset_on_done=True)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "accepted", acc, "/", int(out["services_processed"][-1]), "virtual", int(out["virtual"].sum()),
          "max channels", int(out["n_channels"].max()), "shares off the hundredths", frac)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    install_gym_stub()
    for c in CASES:
        if args.case is None or c[0] == args.case:
            gen(*c)


if __name__ == "__main__":
    main()
