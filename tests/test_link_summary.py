"""A link's summary at a provision on the host (csrc/orlg_link_summary.h): tests/link_summary_check.cc clears every wholly free
window of bitmaps of 64, 100, 128, 320 and 400 slots at several densities, derives the seven integers of the link's statistics
from the summary before, the window and its two neighbouring bits, and compares them with a bit-loop recount of the cleared bitmap;
pack and unpack round-trip.  Compiled with the address and undefined-behaviour sanitizers and run as a program of its own; no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optical-rl-gym-qot-aware_amd", "csrc")


def test_provisioned_summary_equals_recount_on_every_free_window(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "link_summary_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "link_summary_check.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "summary and recount agree on every window" in r.stdout, r.stdout
