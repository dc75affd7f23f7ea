"""The host programs of the suite: plain C++ compiled against ``csrc``, linked with the built library and run without a device.

``variant_names()`` compiles and runs ``tests/variant_names.cpp`` once per session and returns what it printed: the keys it walked
per list of ``csrc/orlg_variants.h`` (summed over the word counts the library holds), the number of kernels it checked and its lines."""
import functools
import os
import subprocess
import tempfile
import types

from conftest import ROOT


@functools.lru_cache(maxsize=None)
def variant_names():
    """.counts {list name: keys walked}, .checked, .lines (all it printed); fails where the program does"""
    from optical_rl_gym_amd import build
    if build.needs_build():
        build.build(verbose=False)
    lib = build.LIB   # (the tree's own library, whatever ORLG_LIB_PATH says: the program is compiled against the tree's header)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "variant_names")
        subprocess.run([build._hipcc(), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", build.CSRC,
                        "-x", "c++", os.path.join(ROOT, "tests", "variant_names.cpp"), "-x", "none", lib,
                        "-Wl,-rpath," + os.path.dirname(lib), "-ldl", "-o", exe], check=True)
        run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    counts = {name: int(n) for _, name, n in (line.split() for line in lines if line.startswith("list "))}
    assert lines[-1].startswith("checked ")
    return types.SimpleNamespace(counts=counts, checked=int(lines[-1].split()[1]), lines=lines)
