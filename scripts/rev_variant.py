#!/usr/bin/env python3
"""Build romis_amd/_build/variants/<name>/libromis_amd.so from romis_amd/csrc as committed at a git revision, for A/B runs
against the working tree with scripts/kbench_libs.sh.  The sources and headers are the files present at the revision
(one restir.cpp before the C ABI was split into units, several units after); a file the working tree's build still
lists keeps its flags, any other .hip gets the kernels' and any other .cpp the host HIP flags.

    python scripts/rev_variant.py <name> <rev>
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from romis_amd import build  # noqa: E402


def main():
    name, rev = sys.argv[1], sys.argv[2]
    vdir = os.path.join(build.OUT, "variants", name)
    os.makedirs(vdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "csrc")
        os.makedirs(src)
        at_rev = subprocess.check_output(["git", "-C", ROOT, "ls-tree", "--name-only", f"{rev}:romis_amd/csrc"]).decode().split()
        known = dict(build.SOURCES)
        by_ext = {".hip": known["kernels.hip"], ".cpp": ["-x", "hip"] + build.DEVICE}
        sources = [(f, known.get(f, by_ext[os.path.splitext(f)[1]])) for f in at_rev if os.path.splitext(f)[1] in by_ext]
        for f in [s for s, _ in sources] + [h for h in at_rev if h.endswith(".h")]:
            with open(os.path.join(src, f), "wb") as fh:
                fh.write(subprocess.check_output(["git", "-C", ROOT, "show", f"{rev}:romis_amd/csrc/{f}"]))
        objs = []
        for s, extra in sources:
            obj = os.path.join(vdir, s + ".o")
            flags = [c if not c.startswith("-I" + build.CSRC) else "-I" + src for c in build.COMMON]
            subprocess.check_call([build.HIPCC] + flags + extra + ["-c", os.path.join(src, s), "-o", obj])
            objs.append(obj)
    subprocess.check_call([build.HIPCC, "-shared", f"--offload-arch={build.ARCH}", "-fno-gpu-rdc", "-o",
                           os.path.join(vdir, "libromis_amd.so")] + objs)
    print(name, rev)


if __name__ == "__main__":
    main()
