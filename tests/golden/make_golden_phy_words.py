#!/usr/bin/env python3
"""Generate the PhyRMSA fixtures at channel counts of one to four occupancy words per link (the phy_* / cont_* fixtures all
have C = 268: five words) by running the UNMODIFIED reference, like make_golden.py (whose trace recorder, table loaders and
gym stub this script imports) with other ``number_spectrum_channels`` / ``number_spectrum_channels_s_band``.

    python tests/golden/make_golden_phy_words.py [--case NAME]

Outputs words_*.npz (discrete bit rates) and words_cont_*.npz (continuous): the per-step traces of run_phy_trace.  The
reference indexes the QoT tables by channel, so a smaller channel count reads their first C columns; the tests hand the
device and the oracle the tables cut to these columns.  The names keep clear of the globs of the other collectors (phy_*,
cont_*, rmsa_*, deeprmsa_*), which hand the tables over uncut.  The archives are written with fixed member times, so that a
second run reproduces them byte for byte.
"""
import argparse
import io
import json
import os
import zipfile

import numpy as np

from make_golden import (HERE, PHY_BASE, PHY_TABLES, TOPOLOGIES, _jsonable, install_gym_stub, load_phy_tables,
                         load_pickled_topology, run_phy_trace)

BASE = dict(PHY_BASE, mean_service_holding_time=25, episode_length=150)
CUT = dict(defrag_period=7, number_moves=6, metric="cut")
RSS = dict(defrag_period=7, number_moves=6, metric="rss")
CONT = dict(bit_rate_selection="continuous", bit_rate_lower_bound=100, bit_rate_higher_bound=600)


def split(c, s):
    return dict(number_spectrum_channels=c, number_spectrum_channels_s_band=s)


CASES = [
    # (name, channels C, env kwargs over BASE, policy, steps); the loads of tests/phy_words_reference.py
    ("words_us14_c3_s40_bmfa_groom_defrag_cut", 3, dict(split(1, 1), seed=40, load=50, grooming=True, **CUT), "bmfa", 620),
    ("words_us14_c64_s41_bmfa_rss_groom_defrag_rss", 64, dict(split(10, 44), seed=41, load=6000, grooming=True, **RSS),
     "bmfa_rss", 500),
    ("words_us14_c65_s42_sapff_defrag_rss", 65, dict(split(10, 45), seed=42, load=6000, **RSS), "sapff", 500),
    ("words_us14_c129_s43_bmfa_groom_defrag_cut", 129, dict(split(20, 89), seed=43, load=16000, grooming=True, **CUT),
     "bmfa", 950),
    # plain; these two may stop short of blocking (the oracle carries them further in the GPU tests) but light their last word
    ("words_us14_c193_s44_faff", 193, dict(split(40, 113), seed=44, load=24000), "faff", 1150),
    ("words_us14_c256_s45_sapbm", 256, dict(split(80, 96), seed=45, load=32000), "sapbm", 720),
    # continuous bit rates 100..600 (with the default 25..100 the spectrum never fills)
    ("words_cont_us14_c65_s46_bmfa_groom", 65, dict(split(10, 45), seed=46, load=6000, grooming=True, **CONT), "bmfa", 500),
    ("words_cont_us14_c193_s47_sapbm", 193, dict(split(40, 113), seed=47, load=24000, **CONT), "sapbm", 700),
]
SATURATED = {3, 64, 65, 129}   # discrete fixtures that must block >= 20, accept >= 30 % and light channel C - 1
# run_phy_trace records more than the tests read: the fixtures keep these (and stay within the size of the phy_* ones)
DROP = ("occ_crc", "reward")


def save_reproducible(path, arrays):
    """np.savez_compressed with the members' times fixed (numpy stamps them with the clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=6)


def gen(name, C, over, policy, steps):
    kw = dict(BASE)
    kw.update(over)
    assert 2 * kw["number_spectrum_channels"] + kw["number_spectrum_channels_s_band"] == C
    tab = "us14_k3"
    topo = load_pickled_topology(TOPOLOGIES[PHY_TABLES[tab][2]])
    out = run_phy_trace(topo, load_phy_tables(tab), kw, policy, steps, True)
    acc = out["accepted"].astype(bool)
    phys = acc & ~out["virtual"].astype(bool)
    top = int(out["channels"][phys].max())
    cont = kw["bit_rate_selection"] == "continuous"
    last_word = 64 * ((C - 1) // 64)
    assert top >= last_word, (name, top)
    if not cont and C in SATURATED:
        assert (~acc).sum() >= 20 and acc.mean() >= 0.3 and top == C - 1, (name, int((~acc).sum()), acc.mean(), top)
        if kw["grooming"] or policy not in ("bmfa", "bmfa_rss"):
            assert out["virtual"].sum() >= 1, name
    if "defrag_period" in kw:   # (counters of the running episode)
        assert out["num_moves"].max() > 0 and out["num_defrag_cycle"].max() > 0, name
    for f in DROP:
        out.pop(f, None)
    meta = dict(topology=PHY_TABLES[tab][2], tables=tab, num_channels=C, env_kwargs=_jsonable(kw), policy=policy, steps=steps,
                reset_on_done=True)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, name + ".npz")
    save_reproducible(path, out)
    print(name, "accepted", int(acc.sum()), "/", steps, "blocked", int((~acc).sum()), "virtual", int(out["virtual"].sum()),
          "top channel", top, "running", int(out["n_running"].max()), "moves", float(out["num_moves"].max()),
          "bytes", os.path.getsize(path), flush=True)


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
