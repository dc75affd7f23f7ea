"""The kernels of the GN-model admission check (``csrc/orlg_variants.h`` ``ORLG_WAVE_GN_KEY_LIST``): the name a gated launch
reports is the kernel it ran, at every word count -- ``test_variant_names.py`` for the three keys per word count that a handle
with a gate adds.  Device-free: ``variant_names_gn.cpp`` is a plain host program linked with the built library."""
import os
import subprocess

from conftest import ROOT


def test_gated_names_are_the_gated_kernels(tmp_path):
    from optical_rl_gym_amd import build
    if build.needs_build():
        build.build(verbose=False)
    exe = str(tmp_path / "variant_names_gn")
    lib = build.LIB
    subprocess.run([build._hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", build.CSRC,
                    "-x", "c++", os.path.join(ROOT, "tests", "variant_names_gn.cpp"), "-x", "none", lib,
                    "-Wl,-rpath," + os.path.dirname(lib), "-ldl", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert run.stdout.strip().splitlines()[-1] == "checked %d" % (3 * len(build.WAVE_W))
