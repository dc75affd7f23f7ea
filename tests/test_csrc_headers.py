"""The include structure of ``csrc``: every header stands on its own, and a kernel family's objects depend on that family only.

Device-free: the headers are parsed by the device compiler (``--cuda-device-only -fsyntax-only``, nothing is generated), and
the family boundaries are read from the depfiles the build writes next to its objects.  Both are what ``build.py`` promises when
it says that an edit of one kernel family recompiles that family only."""
import concurrent.futures
import fnmatch
import glob
import os
import shutil
import subprocess

import pytest

from optical_rl_gym_amd import build

pytestmark = pytest.mark.skipif(shutil.which(build._hipcc()) is None, reason="needs hipcc")

# the text of a function body, included inside orlg_rmsa_group_kernel and orlg_rmsa_group_body: says so in its first lines
NOT_AT_FILE_SCOPE = {"orlg_group_body.h"}
# what a header needs on the command line: the instantiation units' shared header is compiled for one word count
DEFINES = {"orlg_inst.h": ["-DORLG_INST_W=5"]}


def _included_files():
    """Every csrc/*.h, and every *.hip that is meant to be included: those carry `#pragma once`, a translation unit does not."""
    files = sorted(glob.glob(os.path.join(build.CSRC, "*.h")) + glob.glob(os.path.join(build.CSRC, "*.hip")))
    once = [f for f in files if "\n#pragma once\n" in open(f).read()]
    headers = {os.path.basename(f) for f in files if f.endswith(".h")}
    assert headers - {os.path.basename(f) for f in once} == NOT_AT_FILE_SCOPE
    return once


def _parse_alone(header, tmp):
    src = os.path.join(tmp, os.path.basename(header) + ".hip")
    with open(src, "w") as f:
        f.write('#include "%s"\n' % os.path.basename(header))
    run = subprocess.run([build._hipcc()] + build.FLAGS + DEFINES.get(os.path.basename(header), []) +
                         ["--cuda-device-only", "-fsyntax-only", "-I", build.CSRC, src],
                         capture_output=True, text=True)
    return os.path.basename(header), run.returncode, run.stderr


def test_every_header_is_self_contained(tmp_path):
    headers = _included_files()
    assert len(headers) >= 20
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        results = list(ex.map(lambda h: _parse_alone(h, str(tmp_path)), headers))
    failed = {name: err[-2000:] for name, rc, err in results if rc != 0}
    assert not failed, failed


def _dep_names(pattern):
    """{object name: base names of the files its depfile names} for the units of build.units() that match the pattern"""
    out = {}
    for name, _, _ in build.units():
        if fnmatch.fnmatchcase(name, pattern):
            deps = build._deps(os.path.join(build.OBJ, name + ".d"))
            assert deps, name
            out[name] = {os.path.basename(d) for d in deps}
    assert out, pattern
    return out


def _none_named(deps, *patterns):
    return {name: sorted(hit) for name, names in deps.items()
            for hit in [{n for n in names if any(fnmatch.fnmatchcase(n, p) for p in patterns)}] if hit}


def test_family_boundaries_hold():
    build.build(verbose=False)
    # the wave-per-environment step kernel is parsed by its own objects only
    for pattern in ("orlg_inst_phy*_w*", "orlg_inst_group_w*", "orlg_api", "orlg_api_step", "orlg_api_query", "orlg_phy_api", "orlg_osnr"):
        assert _none_named(_dep_names(pattern), "orlg_kernels.hip") == {}
    assert len(_dep_names("orlg_inst_phy*_w*")) == 10 and len(_dep_names("orlg_inst_group_w*")) == 7
    # the QoT-aware family takes path_word from orlg_spectrum.h and nothing of the RMSA path's layout or statistics
    for pattern in ("orlg_inst_phy*_w*", "orlg_phy_api"):
        assert _none_named(_dep_names(pattern), "orlg_rmsa_layout.h", "orlg_link_stats.h", "orlg_group_*") == {}
    # the OSNR kernel stands on the wave library alone
    assert _none_named(_dep_names("orlg_osnr"), "orlg_phy_*", "orlg_spectrum.h", "orlg_link_stats.h", "orlg_rmsa_layout.h") == {}
    assert "orlg_wave.h" in _dep_names("orlg_osnr")["orlg_osnr"]
    # ... and the wave family parses neither of the other two
    wave = _dep_names("orlg_inst_wave_w*")
    assert len(wave) == 7
    assert _none_named(wave, "orlg_group_*", "orlg_phy_*") == {}
    assert all("orlg_kernels.hip" in names for names in wave.values())
