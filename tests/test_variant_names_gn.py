"""The kernels of the GN-model admission check (``csrc/orlg_variants.h`` ``ORLG_WAVE_GN_KEY_LIST``): the name a gated launch
reports is the kernel it ran, at every word count -- ``test_variant_names.py`` for the three keys per word count that a handle
with a gate adds.  Device-free: ``tests/variant_names.cpp`` walks them (``host_programs.variant_names``)."""
from host_programs import variant_names


def test_gated_names_are_the_gated_kernels():
    from optical_rl_gym_amd import build
    counts = variant_names().counts
    assert counts["ORLG_WAVE_GN_KEYS"] == 3 * len(build.WAVE_W)
