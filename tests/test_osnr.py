"""GN-model GSNR routine: oracle vs the golden grid (CPU) and device vs oracle / golden (GPU), tolerance 1e-6
relative as north_star states (observed ~1e-15).  Parity unpinned by the reference itself (no caller / no test).

The grid never leaves the kernel's fast path (one attenuation per link, at most 512 list entries, at most 64 spans):
tests/golden/osnr_edges.npz (make_golden_osnr_edges.py) holds the checks that do, with their 50-digit results
(oracle.gn_osnr_mp), and the tests below hold oracle and device to those."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN


def grid():
    return np.load(os.path.join(GOLDEN, "osnr_grid.npz"), allow_pickle=False)


def test_oracle_matches_golden_grid():
    import oracle as orc
    z = grid()
    got = orc.gn_osnr(z)
    np.testing.assert_allclose(got, z["gsnr_db"], rtol=1e-12)


def test_stale_phi_quirk_is_reproduced():
    """Putting the current service itself into a link's running list changes the result (the stale phi is added)."""
    import oracle as orc
    att = 0.2 / (2 * 10 * np.log10(np.exp(1)) * 1e3)
    base = dict(check_link_off=[0, 1], link_span_off=[0, 2], bandwidth=[50e9], center_frequency=[193.1e12],
                launch_power=[1e-3], span_length_km=[75.0, 75.0], span_attenuation=[att, att],
                span_noise_figure=[10 ** 0.55] * 2)
    without = dict(base, link_svc_off=[0, 1], svc_bandwidth=[50e9], svc_center_frequency=[193.2e12], svc_se=[2], svc_is_self=[0])
    with_self_after = dict(base, link_svc_off=[0, 2], svc_bandwidth=[50e9, 50e9], svc_center_frequency=[193.2e12, 193.1e12],
                           svc_se=[2, 1], svc_is_self=[0, 1])
    a, b = orc.gn_osnr(without)[0], orc.gn_osnr(with_self_after)[0]
    assert a != b and abs(a - b) < 1.0


@pytest.mark.gpu
def test_device_matches_oracle_and_golden():
    import oracle as orc
    from optical_rl_gym_amd import gn_osnr, modulation_level_from_gsnr
    z = grid()
    got = gn_osnr(z)
    np.testing.assert_allclose(got, z["gsnr_db"], rtol=1e-6)      # the stated tolerance
    np.testing.assert_allclose(got, z["gsnr_db"], rtol=1e-12)     # what is actually achieved
    np.testing.assert_allclose(got, orc.gn_osnr(z), rtol=1e-12)
    lv = modulation_level_from_gsnr(got)
    assert lv.min() >= 0 and lv.max() <= 6
    # empty batch and a check whose link lists are empty
    assert gn_osnr({k: z[k][:0] if k not in ("check_link_off", "link_span_off", "link_svc_off") else np.zeros(1, np.int32)
                    for k in z.files if k != "gsnr_db"}).shape == (0,)


# ------------------------------------------------------------------------------------- the edges of the kernel
FIELD_NAMES = ("check_link_off", "link_span_off", "link_svc_off", "bandwidth", "center_frequency", "launch_power",
               "span_length_km", "span_attenuation", "span_noise_figure", "svc_bandwidth", "svc_center_frequency", "svc_se",
               "svc_is_self")
RTOL = 1e-12     # on the dB value, as test_device_matches_oracle_and_golden states it
LANES, KMAX = 64, 8


def edges():
    z = np.load(os.path.join(GOLDEN, "osnr_edges.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def families(z):
    return [(str(name), np.nonzero(z["family"] == k)[0]) for k, name in enumerate(z["family_names"])]


def take_checks(z, checks):
    """The batch of the given checks alone, flattened again."""
    out = {k: [] for k in FIELD_NAMES}
    for k in ("check_link_off", "link_span_off", "link_svc_off"):
        out[k] = [0]
    for m in checks:
        for k in ("bandwidth", "center_frequency", "launch_power"):
            out[k].append(z[k][m])
        for l in range(z["check_link_off"][m], z["check_link_off"][m + 1]):
            s0, s1, i0, i1 = z["link_span_off"][l], z["link_span_off"][l + 1], z["link_svc_off"][l], z["link_svc_off"][l + 1]
            for k in ("span_length_km", "span_attenuation", "span_noise_figure"):
                out[k] += list(z[k][s0:s1])
            for k in ("svc_bandwidth", "svc_center_frequency", "svc_se", "svc_is_self"):
                out[k] += list(z[k][i0:i1])
            out["link_span_off"].append(len(out["span_length_km"]))
            out["link_svc_off"].append(len(out["svc_bandwidth"]))
        out["check_link_off"].append(len(out["link_span_off"]) - 1)
    return {k: np.array(v, dtype=z[k].dtype) for k, v in out.items()}


def classify_links(z):
    """Per link, from the inputs alone: does the kernel take its fast path (at most 8 x 64 list entries and one attenuation
    on all spans; a link without spans has nothing to differ in) or the direct one, how many chunks of 64 spans it has, and
    where the service's own entry sits in the list."""
    n_links = len(z["link_span_off"]) - 1
    fast, chunks, own = np.zeros(n_links, bool), np.zeros(n_links, int), []
    for l in range(n_links):
        att = z["span_attenuation"][z["link_span_off"][l]:z["link_span_off"][l + 1]]
        mine = np.nonzero(z["svc_is_self"][z["link_svc_off"][l]:z["link_svc_off"][l + 1]])[0]
        n = z["link_svc_off"][l + 1] - z["link_svc_off"][l]
        fast[l] = n <= LANES * KMAX and np.all(att == att[:1])
        chunks[l] = -(-len(att) // LANES)
        assert len(mine) <= 1
        own.append("absent" if len(mine) == 0 else "only" if n == 1 else "head" if mine[0] == 0 else
                   "tail" if mine[0] == n - 1 else "middle")
    return fast, chunks, np.array(own)


def worst_relative(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), (got[~fin], want[~fin])     # +inf dB: equal, not close
    return float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0


def test_oracle_matches_50_digits_on_the_edges():
    """Worst relative error of the oracle against the 50-digit values, per family: direct_att 1.7e-16, direct_len 1.5e-16,
    fast_bounds 2.5e-16, span_chunks 4.2e-16, carry_links 1.7e-16, degenerate 1.4e-16, se_bw_sides 1.6e-16 -- the oracle
    is a sound float64 witness on these inputs."""
    import oracle as orc
    z = edges()
    got = orc.gn_osnr(z)
    assert not np.isnan(got).any() and not np.isnan(z["gsnr_db_mp"]).any()
    for name, idx in families(z):
        worst = worst_relative(got[idx], z["gsnr_db_mp"][idx])
        print(f"oracle vs 50 digits, {name}: {worst:.2e}")
        assert worst <= RTOL, name
    fin = np.isfinite(got)
    assert got[fin].min() > 0 and got[fin].max() < 40 and (~fin).sum() == 3


def test_edges_fixture_is_what_50_digits_give():
    """Every stored value, computed again (a few seconds): a stale or edited fixture does not pass.  At 60 digits a sample of
    each family rounds to the same float64, so 50 digits are enough to round once."""
    import oracle as orc
    z = edges()
    assert np.array_equal(orc.gn_osnr_mp(z), z["gsnr_db_mp"])
    sample = np.concatenate([idx[:3] for _, idx in families(z)])
    assert np.array_equal(orc.gn_osnr_mp(z, checks=list(sample), dps=60), z["gsnr_db_mp"][sample])


def test_edges_cover_what_the_grid_does_not():
    """A condition on the inputs: the fixture holds every (kernel path, position of the own entry) cell and links of several
    span chunks on both paths, and the grid holds none of the direct path -- which is why the edge file exists."""
    z = edges()
    fast, chunks, own = classify_links(z)
    for path, on_path in (("fast", fast), ("direct", ~fast)):
        for cls in ("absent", "head", "middle", "tail", "only"):
            assert (on_path & (own == cls)).sum() >= 3, (path, cls)
        assert (on_path & (chunks >= 2)).sum() >= 2, path
        assert (on_path & (chunks >= 2) & (own == "head")).sum() >= 2, path    # the stale phi across the chunk boundary
    n = np.diff(z["link_svc_off"])
    assert {1, 63, 64, 65, 128, 129, 511, 512} <= set(n[fast]) and {513, 700} <= set(n[~fast])
    assert {64, 65, 128, 129, 130} <= set(np.diff(z["link_span_off"])[fast]) & set(np.diff(z["link_span_off"])[~fast])
    others = z["svc_is_self"] == 0
    assert set(z["svc_se"][others]) == {1, 2, 3, 4, 5, 6} and len(set(z["bandwidth"])) == 3
    # an own-entry-at-head link right after: a fast link, a direct link, an empty list, a list of the own entry only, nothing
    seen = set()
    for m in range(len(z["bandwidth"])):
        l0, l1 = z["check_link_off"][m], z["check_link_off"][m + 1]
        for l in range(l0, l1):
            if own[l] == "head":
                before = "first" if l == l0 else "empty" if n[l - 1] == 0 else "own_only" if own[l - 1] == "only" else \
                    "fast" if fast[l - 1] else "direct"
                seen.add((before, "fast" if fast[l] else "direct"))
    assert seen == {(b, p) for b in ("first", "fast", "direct", "empty", "own_only") for p in ("fast", "direct")}
    g = grid()
    gfast, gchunks, _ = classify_links(g)
    assert gfast.all() and gchunks.max() == 1


def small_batch():
    att = 0.2 / (2 * 10 * np.log10(np.exp(1)) * 1e3)
    return dict(check_link_off=[0, 2], link_span_off=[0, 2, 3], link_svc_off=[0, 2, 3], bandwidth=[50e9], center_frequency=[193.1e12],
                launch_power=[1e-3], span_length_km=[75.0, 75.0, 60.0], span_attenuation=[att] * 3, span_noise_figure=[10 ** 0.55] * 3,
                svc_bandwidth=[50e9] * 3, svc_center_frequency=[193.2e12, 193.1e12, 193.0e12], svc_se=[2, 1, 6], svc_is_self=[0, 1, 0])


@pytest.mark.parametrize("change,message", [
    (dict(check_link_off=[1, 2]), "check_link_off does not start at 0"),
    (dict(link_span_off=[0, 3, 2]), "link_span_off does not ascend"),
    (dict(link_svc_off=[0, 2, 4]), "link_svc_off ends at 4, not at the number of list entries"),
    (dict(check_link_off=[0, 1]), "check_link_off ends at 1, not at the number of links"),
    (dict(link_span_off=[0, 2, 2]), "link_span_off ends at 2, not at the number of spans"),
    (dict(check_link_off=[0, 1, 2]), "check_link_off has 3 entries for 1 checks"),
    (dict(span_noise_figure=[3.5, 3.5]), "arrays of one family differ in length"),
    (dict(launch_power=[1e-3, 1e-3]), "arrays of one family differ in length"),
    (dict(svc_se=[2, 1]), "arrays of one family differ in length"),
    (dict(link_svc_off=[0, 3]), "arrays of one family differ in length"),
    (dict(svc_se=[2, 1, 7]), "svc_se outside 1..6"),
    (dict(svc_se=[0, 1, 6]), "svc_se outside 1..6"),
    (dict(svc_is_self=[1, 1, 0]), "more than one self entry in the list of link 0"),
    (dict(svc_center_frequency=[193.2e12, 193.1e12, 193.1e12]), "a non-self entry sits on the center_frequency of its check"),
])
def test_gn_osnr_refuses_a_malformed_batch(change, message, monkeypatch):
    """ValueError before the library is loaded (loading it here, without a device or a compiler, would be another error)."""
    from optical_rl_gym_amd import _lib, gn_osnr
    from optical_rl_gym_amd.osnr import validate_batch

    def no_load(*a, **k):
        raise AssertionError("the library must not be loaded for a malformed batch")
    monkeypatch.setattr(_lib, "load", no_load)
    validate_batch(small_batch())     # the unchanged batch is fine (a self entry's svc_se is not looked at)
    validate_batch(dict(small_batch(), svc_se=[2, 0, 6]))
    with pytest.raises(ValueError, match=message):
        gn_osnr(dict(small_batch(), **change))


def test_fixtures_are_well_formed_batches():
    from optical_rl_gym_amd.osnr import validate_batch
    validate_batch(grid())
    validate_batch(edges())
    z = grid()
    validate_batch({k: z[k][:0] if k not in ("check_link_off", "link_span_off", "link_svc_off") else np.zeros(1, np.int32)
                    for k in z.files if k != "gsnr_db"})


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["direct_att", "direct_len", "fast_bounds", "span_chunks", "carry_links", "degenerate", "se_bw_sides"])
def test_device_matches_50_digits_on_the_edges(family):
    """Device against the 50-digit values and against the oracle, each family in a launch of its own, rtol 1e-12 on the dB
    value.  Measured worst relative error against the 50-digit values, device | oracle:
    direct_att 1.7e-16 | 1.7e-16, direct_len 1.5e-16 | 1.5e-16, fast_bounds 2.5e-16 | 2.5e-16, span_chunks 2.1e-16 | 4.2e-16,
    carry_links 1.6e-16 | 1.7e-16, degenerate 1.4e-16 | 1.4e-16, se_bw_sides 1.6e-16 | 1.6e-16 (device against oracle: at most
    3.2e-16) -- no family needs more than the last digit or two of a float64."""
    import oracle as orc
    from optical_rl_gym_amd import gn_osnr
    z = edges()
    idx = dict(families(z))[family]
    part = take_checks(z, idx)
    got, want, ora = gn_osnr(part), z["gsnr_db_mp"][idx], orc.gn_osnr(part)
    print(f"{family}: device vs 50 digits {worst_relative(got, want):.2e}, oracle vs 50 digits {worst_relative(ora, want):.2e}, "
          f"device vs oracle {worst_relative(got, ora):.2e}")
    assert not np.isnan(got).any()
    for m in range(len(idx)):    # one by one, so that a failure names its check
        np.testing.assert_allclose(got[m], want[m], rtol=RTOL, atol=0, err_msg=f"{family}, check {idx[m]} of the fixture vs 50 digits")
        np.testing.assert_allclose(got[m], ora[m], rtol=RTOL, atol=0, err_msg=f"{family}, check {idx[m]} of the fixture vs oracle")
    # the same checks inside the whole batch (other wavefronts of the workgroup busy with other checks)
    assert np.array_equal(gn_osnr(z)[idx], got)


@pytest.mark.gpu
def test_both_kernel_paths_agree_on_the_edges():
    """One ulp on the last span's attenuation of every fast-path link sends it down the direct path; the input moves by 1e-16,
    so the result must stay within 1e-12 -- stale phi and carry included -- and within 1e-12 of the 50-digit value."""
    from optical_rl_gym_amd import gn_osnr
    z = edges()
    fast, _, _ = classify_links(z)
    spans = np.diff(z["link_span_off"])
    moved = dict(z)
    moved["span_attenuation"] = z["span_attenuation"].copy()
    last = z["link_span_off"][1:][fast & (spans >= 2)] - 1
    moved["span_attenuation"][last] = np.nextafter(moved["span_attenuation"][last], 1.0)
    fast_after, _, _ = classify_links(moved)
    assert not fast_after[spans >= 2].any() and (fast & (spans >= 2)).sum() > 60
    check_of_link = np.repeat(np.arange(len(z["bandwidth"])), np.diff(z["check_link_off"]))
    changed = np.unique(check_of_link[fast & ~fast_after])
    a, b = gn_osnr(z), gn_osnr(moved)
    print(f"fast vs direct path on {len(changed)} checks: {worst_relative(b[changed], a[changed]):.2e}")
    for m in changed:
        np.testing.assert_allclose(b[m], a[m], rtol=RTOL, atol=0, err_msg=f"check {m}, family {z['family_names'][z['family'][m]]}")
        np.testing.assert_allclose(b[m], z["gsnr_db_mp"][m], rtol=RTOL, atol=0, err_msg=f"check {m} vs 50 digits")


DEVICE_POINTER_CHILD = """
import ctypes as C
import sys
import numpy as np, torch
torch.zeros(1, device="cuda")
sys.path[:0] = [%r, %r]
from conftest import GOLDEN
from optical_rl_gym_amd import _lib, gn_osnr
from optical_rl_gym_amd.osnr import FIELDS, OsnrBatch
z = dict(np.load(GOLDEN + "/osnr_edges.npz", allow_pickle=False))
want = gn_osnr(z)
L = _lib.load()
L.orlg_gn_osnr.argtypes = [C.POINTER(OsnrBatch), C.c_void_p, C.c_int32, C.c_void_p]
host = {n: np.ascontiguousarray(z[n], dtype=dt) for n, dt in FIELDS}
dev = {n: torch.from_numpy(host[n]).cuda() for n in host}
assert all(t.is_cuda for t in dev.values())
torch.cuda.synchronize()
stream = torch.cuda.Stream()
assert stream.cuda_stream != 0


def call(inputs_on_device, output_on_device):
    b = OsnrBatch()
    for n, _ in FIELDS:
        setattr(b, n, C.c_void_p(dev[n].data_ptr()) if inputs_on_device else host[n].ctypes.data_as(C.c_void_p))
    b.num_checks, b.num_links = len(host["bandwidth"]), len(host["link_span_off"]) - 1
    b.num_spans, b.num_services = len(host["span_length_km"]), len(host["svc_bandwidth"])
    if output_on_device:
        out = torch.full((b.num_checks,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.orlg_gn_osnr(C.byref(b), C.c_void_p(out.data_ptr()), 0, C.c_void_p(stream.cuda_stream)))
        stream.synchronize()      # all on the device: the call does not wait
        return out.cpu().numpy()
    out = np.full(b.num_checks, np.nan)
    _lib.check(L.orlg_gn_osnr(C.byref(b), out.ctypes.data_as(C.c_void_p), 0, C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return out


assert not np.isnan(want).any() and np.isinf(want).sum() == 3
for inputs_on_device, output_on_device in ((True, True), (False, True), (True, False), (False, False)):
    got = call(inputs_on_device, output_on_device)
    assert np.array_equal(got, want), (inputs_on_device, output_on_device, np.nonzero(got != want)[0][:5])
assert np.array_equal(gn_osnr(z, stream_ptr=stream.cuda_stream), want)
print("device pointers ok")
"""


@pytest.mark.gpu
def test_device_pointers_and_stream():
    """The C entry point takes host or device pointers for every array and for the output, and the caller's stream: device
    tensors on a side stream, and both mixtures, give the bits of the host-array call on the whole edge file.  In a child
    process: torch has to create its HIP context before the library does."""
    import subprocess
    import sys
    root = os.path.dirname(GOLDEN.rstrip(os.sep))
    code = DEVICE_POINTER_CHILD % (os.path.dirname(root), root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "device pointers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
