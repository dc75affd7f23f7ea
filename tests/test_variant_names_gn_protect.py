"""The kernels of a handle that protects its running lightpaths (``csrc/orlg_variants.h`` ``ORLG_WAVE_GN_PROTECT_KEY_LIST``,
``ORLG_WAVE_GN_PROTECT_CAUSE_KEY_LIST``): every such key has a kernel and a distinct name at every word count, its unit
answers it and no other unit does, and every other key of the family answers as before.  Device-free: ``tests/variant_names.cpp``
walks them (``host_programs.variant_names``)."""
from host_programs import variant_names

OLD_WAVE_KEYS = 11 + 3 + 6 + 6 + 6 + 6 + 6 + 6   # the lists of the other two units of csrc/orlg_variants.h, in its order
NEW_KEYS = 3 + 3


def test_protecting_names_are_the_protecting_kernels():
    from optical_rl_gym_amd import build
    counts = variant_names().counts
    n = len(build.WAVE_W)
    assert (counts["ORLG_WAVE_GN_PROTECT_KEYS"], counts["ORLG_WAVE_GN_PROTECT_CAUSE_KEYS"]) == (3 * n, 3 * n)
    wave = [c for name, c in counts.items() if name.startswith("ORLG_WAVE_") and name not in ("ORLG_WAVE_GN_MM_KEYS", "ORLG_WAVE_GN_AM_KEYS", "ORLG_WAVE_QUERIES")]
    assert sum(wave) == (OLD_WAVE_KEYS + NEW_KEYS) * n
