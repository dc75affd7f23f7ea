"""The name a launch reports (``last_kernel()``) is the kernel the launch ran, for every instantiation the library holds.

Device-free: ``variant_names.cpp`` is compiled as a plain host program against ``csrc/orlg_variants.h``, linked with the built
library and run (``host_programs.variant_names``).  For every legal key of every kernel family at every word count it asks the
library's lookup for the kernel, resolves the returned address to its symbol and compares the demangled symbol with the name the
host formats from the same key; it also requires one kernel per key, the answer of the unit that holds the key and of no other,
and null for keys outside the lists.  The per-feature tests assert their own lists' counts; this one asserts all of them."""
from host_programs import variant_names

# keys per list of csrc/orlg_variants.h and word count, in its order: a new variant adds its list's literal here
WAVE = {"ORLG_WAVE_KEYS": 11, "ORLG_WAVE_GN_KEYS": 3, "ORLG_WAVE_CAUSE_KEYS": 6, "ORLG_WAVE_ASSIGN_KEYS": 6, "ORLG_WAVE_CUT_KEYS": 6,
        "ORLG_WAVE_USAGE_KEYS": 6, "ORLG_WAVE_GN_ASSIGN_KEYS": 6, "ORLG_WAVE_GN_CUT_KEYS": 6, "ORLG_WAVE_GN_PROTECT_KEYS": 3,
        "ORLG_WAVE_GN_PROTECT_CAUSE_KEYS": 3, "ORLG_WAVE_GN_MM_KEYS": 6, "ORLG_WAVE_GN_AM_KEYS": 3}
GROUP = {"ORLG_GROUP_KEYS": 21, "ORLG_GROUP_CAUSE_KEYS": 9, "ORLG_GROUP_ASSIGN_KEYS": 18, "ORLG_GROUP_CUT_KEYS": 18, "ORLG_GROUP_USAGE_KEYS": 18}
QUERIES, AUDIT, PHY = 12, 2, 96   # single-kernel lookups per word count; the audit's two kernels (no word count); the QoT-aware keys


def test_reported_name_is_the_kernel_for_every_key():
    from optical_rl_gym_amd import build
    counts, checked = variant_names().counts, variant_names().checked
    n = len(build.WAVE_W)
    want = {name: k * n for name, k in {**WAVE, **GROUP}.items()}
    want.update(ORLG_PHY_KEYS=PHY * len(build.PHY_W), ORLG_WAVE_QUERIES=QUERIES * n + AUDIT)
    assert counts == want
    # 7 word counts x (56 wave + 6 max-margin + 3 adaptive + 84 group + 12 single kernels) + 5 x 96 QoT-aware + 2 audit = 1609
    assert checked == 7 * (11 + 3 + 6 + 6 + 6 + 6 + 6 + 6 + 3 + 3 + 6 + 3 + 21 + 9 + 18 + 18 + 18 + 12) + 5 * 96 + 2 == 1609
    assert checked == sum(want.values())
