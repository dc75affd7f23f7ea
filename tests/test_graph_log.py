"""The lean body's graph log on the host (csrc/orlg_graph_log.h): tests/graph_log_check.cc packs random updates at the field limits
into a row of lanes, works them off in batches the way group_graph_replay does and compares the three doubles bit for bit with
a plain sequential _update_network_stats.  Compiled with the address and undefined-behaviour sanitizers and run as a program of
its own; no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optical-rl-gym-qot-aware_amd", "csrc")


def test_batched_graph_log_equals_sequential_update(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "graph_log_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "graph_log_check.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "agree bit for bit" in r.stdout, r.stdout

