"""Compare the device code of two trees, unit by unit and byte by byte.

    python tools/device_code_diff.py <tree A> <tree B> [-j N] [--only PATTERN]

Every unit of tree A's ``build.units()`` that holds device code is compiled in both trees with the library's flags plus
``--offload-device-only --no-gpu-bundle-output``, and the ``.text``, ``.rodata`` (kernel descriptors) and ``.note`` (metadata) sections
of the two code objects are compared.  (Whole files differ from compile to compile: a ``__hip_cuid_<hash>`` symbol.)  Prints one line
per unit and exits 1 where any differs.  Needs no GPU."""
import concurrent.futures
import fnmatch
import importlib.util
import os
import subprocess
import sys
import tempfile

SECTIONS = (".text", ".rodata", ".note")
PKG = "optical-rl-gym-qot-aware_amd"


def _build_module(tree):
    spec = importlib.util.spec_from_file_location("orlg_build_" + str(abs(hash(tree))), os.path.join(tree, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sections(build, src, defines, out):
    cmd = [build._hipcc()] + build.FLAGS + defines + ["--offload-device-only", "--no-gpu-bundle-output", "-I", build.CSRC, "-c",
                                                      os.path.join(build.CSRC, src), "-o", out]
    subprocess.run(cmd, check=True)
    objcopy = os.path.join(os.path.dirname(os.path.realpath(build._hipcc())), "..", "lib", "llvm", "bin", "llvm-objcopy")
    got = {}
    for sec in SECTIONS:
        subprocess.run([objcopy, "-O", "binary", "--only-section=" + sec, out, out + sec], check=True)
        got[sec] = open(out + sec, "rb").read()
    return got


def _unit(a, b, name, src, defines, tmp):
    sa, sb = (_sections(m, src, defines, os.path.join(tmp, "%s_%s.co" % (side, name))) for side, m in (("a", a), ("b", b)))
    return name, [sec for sec in SECTIONS if sa[sec] != sb[sec]], sum(len(v) for v in sa.values())


def main(argv):
    jobs = int(argv[argv.index("-j") + 1]) if "-j" in argv else min(os.cpu_count() or 1, 16)
    only = argv[argv.index("--only") + 1] if "--only" in argv else "*"
    a, b = _build_module(os.path.abspath(argv[1])), _build_module(os.path.abspath(argv[2]))
    units = [u for u in a.units() if fnmatch.fnmatchcase(u[0], only)]
    differ = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        for name, bad, size in ex.map(lambda u: _unit(a, b, u[0], u[1], u[2], tmp), units):
            print("%-28s %9d B  %s" % (name, size, "differs in " + ", ".join(bad) if bad else "identical"), flush=True)
            differ += bool(bad)
    print("%d of %d units differ" % (differ, len(units)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
