"""Oracle PhyRMSAEnv against the reference's traces at channel counts of one to four occupancy words per link (the phy_*
fixtures of test_oracle_phy.py all have C = 268): bit-exact, the QoT tables cut to their first C columns.  With the oracle
pinned here, a disagreement between the device and the oracle at a small channel count (tests/test_gpu_phy_words.py) can be
assigned to a side."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, phy_oracle_from_kwargs
from phy_words_reference import cut_tables, topology

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "words_us14_*.npz")))
SATURATED = {3, 64, 65, 129}


def test_fixtures_cover_one_to_four_words():
    counts = sorted(load_golden(c)[1]["num_channels"] for c in CASES)
    assert counts == [3, 64, 65, 129, 193, 256]


@pytest.mark.parametrize("case", CASES)
def test_phy_words_trace_bit_exact(case):
    z, meta = load_golden(case)
    C, kw, n = meta["num_channels"], meta["env_kwargs"], meta["steps"]
    assert meta["topology"] == "us14_3-paths_6-modulations" and meta["tables"] == "us14_k3"
    assert 2 * kw["number_spectrum_channels"] + kw["number_spectrum_channels_s_band"] == C and kw["bit_rate_selection"] == "discrete"
    # what the fixture reaches: its last word is lit; the smaller ones also saturate
    acc = z["accepted"].astype(bool)
    top = int(z["channels"][acc & ~z["virtual"].astype(bool)].max())
    assert top >= 64 * ((C - 1) // 64)
    if C in SATURATED:
        assert (~acc).sum() >= 20 and acc.mean() >= 0.3 and top == C - 1
        if kw["grooming"] or meta["policy"] not in ("bmfa", "bmfa_rss"):
            assert z["virtual"].sum() >= 1
    env = phy_oracle_from_kwargs(topology(), cut_tables(C), kw)
    tr = env.run(meta["policy"], n, reset_on_done=meta["reset_on_done"])
    assert np.array_equal(tr["src"], z["src_id"]) and np.array_equal(tr["dst"], z["dst_id"])
    assert np.array_equal(tr["bit_rate"], z["bit_rate"]) and np.array_equal(tr["service_id"], z["service_id"])
    assert np.array_equal(tr["arrival"], z["arrival"]) and np.array_equal(tr["holding"], z["holding"])
    assert np.array_equal(tr["act_path"], z["act_path"])
    assert np.array_equal(tr["n_channels"], z["n_channels"])
    assert np.array_equal(tr["channels"], z["channels"].astype(np.int32))
    assert np.array_equal(tr["ch_used"], z["ch_used"])
    assert np.array_equal(tr["ch_cap"], z["ch_cap"].astype(np.int32))
    assert np.array_equal(tr["num_moves"], z["num_moves"])
    assert np.array_equal(tr["num_moves_groom"], z["num_moves_groom"])
    assert np.array_equal(tr["num_defrag_cycle"], z["num_defrag_cycle"])
    for f in ("accepted", "done", "services_accepted", "path_index", "physical_paths", "n_running", "free_total"):
        assert np.array_equal(tr[f].astype(np.int64), z[f].astype(np.int64)), f
    for f in ("number_cuts_total", "rss_total_metric", "total_path_length", "avrage_gsnr", "average_path_index",
              "episode_service_blocking_rate", "bit_rate_blocking_rate", "current_time"):
        bad = np.nonzero(tr[f] != z[f])[0]
        assert bad.size == 0, (f, bad[:5], tr[f][bad[:5]], z[f][bad[:5]])
    # average_mod_level: the reference's uint8 accumulator wraps under NumPy >= 2 (as test_oracle_phy.py)
    want = (tr["total_modulation_level"] % 256) / (tr["channels_accepted"] + 1)
    assert np.array_equal(want, z["average_mod_level"])
    av = env.available_channels()
    assert av.shape[1] == C
    assert np.array_equal(np.packbits(av, axis=1, bitorder="little"), z["final_available_channels"])
    env.close()
