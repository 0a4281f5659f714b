"""Build libromis_amd.so in-tree (romis_amd/_build/) with hipcc for gfx950.

    python -m romis_amd.build [--force]

Flags that matter for parity (DESIGN.md "Floating point"): -ffp-contract=off (no FMA contraction, host and
device), correctly rounded f32 division / sqrt, no fast-math.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "_build")
LIB = os.path.join(OUT, "libromis_amd.so")
ARCH = os.environ.get("ROMIS_AMD_ARCH", "gfx950")

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
COMMON = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", f"-I{os.path.join(ROOT, 'include')}",
          f"-I{CSRC}"]
DEVICE = [f"--offload-arch={ARCH}", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-rdc"]

# -fno-slp-vectorize: the SLP pass packs independent f32 multiplies / adds into v_pk_* ops, which issue at the
# cost of an FMA (≈4.5 cycles per wave instruction on gfx950) instead of ≈2.4 for each scalar op, and need
# v_mov shuffles to assemble their operand pairs; without it: RIS 354 -> 340 us, spatial 85 -> 81, final 104 -> 92
# (kbench, profiles/r2/noslp), fewer VGPRs and no RIS scratch spill.  Results are identical (no contraction).
KERNEL_FLAGS = ["-fno-slp-vectorize"]

# The units behind include/restir_c.h, with their flags.  source_hash() hashes them as the launcher: together with
# route.h they decide which buffers a pass reads and writes.
ABI_UNITS = [
    ("restir.cpp", ["-x", "hip"] + DEVICE),      # HIP host code, no KERNEL_FLAGS
    ("abi_error.cpp", ["-x", "c++"]),            # no HIP header
    ("layout.cpp", ["-x", "c++"]),
    ("denoise_host.cpp", ["-x", "c++"]),         # no HIP header, no HIP call: a stand-alone program links it
    ("history_host.cpp", ["-x", "c++"]),         # likewise
]

SOURCES = [("kernels.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS)] + ABI_UNITS + [
    ("mis.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("refit.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("reproject.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("shadow_lists.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("shadow_vis.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("phat_table.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("present.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("accum.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("exact.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("denoise.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("history.hip", ["-x", "hip"] + DEVICE + KERNEL_FLAGS),
    ("bvh.cpp", ["-x", "c++"]),
    ("screen.cpp", ["-x", "c++"]),
]
HEADERS = ["device_math.h", "restir_types.h", "launch.h", "bvh.h", "pow10_table.h", "kernels_common.h", "launch_events.h", "launch_shape.h",
           "route.h", "ris_members.h", "refit.h", "reproject.h", "shadow_lists.h", "shadow_vis.h", "phat_table.h", "abi_error.h", "layout.h", "halo_segs.h", "present.h", "accum.h", "exact.h", "denoise.h", "ris_ahead.h", "history.h"]


def source_hash() -> str:
    """sha256 over the device sources, the launcher (the C ABI's units and route.h decide which buffers a pass reads and
    writes) and the flags: identifies the kernels a profile was measured on (bench.py reports a committed PMC traffic figure
    only when it matches)."""
    import hashlib
    h = hashlib.sha256()
    for f in [SOURCES[0][0], "phat_table.hip"] + [u for u, _ in ABI_UNITS] + HEADERS:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    h.update(" ".join([c for c in COMMON + DEVICE + KERNEL_FLAGS if not c.startswith("-I")]).encode())   # flags, not paths
    return h.hexdigest()[:16]


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _deps(src: str) -> list[str]:
    return [os.path.join(CSRC, src)] + [os.path.join(CSRC, h) for h in HEADERS] + \
        [os.path.join(ROOT, "include", "restir_c.h"), __file__]


def _compile(src: str, extra: list[str], force: bool) -> str:
    obj = os.path.join(OUT, os.path.basename(src) + ".o")
    if force or _stale(obj, _deps(src)):
        cmd = [HIPCC] + COMMON + extra + ["-c", os.path.join(CSRC, src), "-o", obj]
        subprocess.check_call(cmd)
    return obj


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OUT, exist_ok=True)
    # a library newer than every source stands even where its object files are gone (a tree copied without them)
    if force or _stale(LIB, [d for s in SOURCES for d in _deps(s[0])]):
        with cf.ThreadPoolExecutor(max_workers=min(len(SOURCES), 16)) as ex:
            objs = list(ex.map(lambda s: _compile(s[0], s[1], force), SOURCES))
        if force or _stale(LIB, objs):
            cmd = [HIPCC, "-shared", f"--offload-arch={ARCH}", "-fno-gpu-rdc", "-o", LIB] + objs
            subprocess.check_call(cmd)
    tool = os.path.join(OUT, "tools", "fastmath_check")
    src = os.path.join(ROOT, "tests", "hip", "fastmath_check.hip")
    if os.path.exists(src) and (force or _stale(tool, [src, os.path.join(CSRC, "device_math.h"), __file__])):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call([HIPCC] + COMMON + DEVICE + ["-x", "hip", src, "-o", tool])
    build_route_check(force)
    build_bvh_check(force)
    build_refit_check(force)
    build_shadow_lists_check(force)
    build_shadow_vis_layout(force)
    build_phat_layout(force)
    build_ris_ahead_key(force)
    build_ris_batch_ring(force)
    if verbose:
        print(LIB)
    return LIB


def build_route_check(force: bool = False) -> str:
    """tools/route_check: the route functions of csrc/route.h as a host program that replays tests/golden/launch_routes.txt
    (tests/test_launch_routes.py); plain C++ over the headers, no device code."""
    tool = os.path.join(OUT, "tools", "route_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", f) for f in ("route_check.cpp", "route_rows.h")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("route.h", "ris_members.h", "launch_shape.h", "restir_types.h")] + [__file__]
    if os.path.exists(srcs[0]) and (force or _stale(tool, deps)):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")
        subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                               f"-I{rocm_include}", f"-I{CSRC}", f"-I{os.path.dirname(srcs[0])}", srcs[0], "-o", tool])
    return tool


def build_bvh_check(force: bool = False) -> str:
    """tools/bvh_check: tests/cpp/bvh_check.cpp over csrc/bvh.cpp with the host compiler -- the BVH's invariants and the
    ray walks' pruning against brute force (tests/test_bvh_invariants.py); no device code."""
    tool = os.path.join(OUT, "tools", "bvh_check")
    src = os.path.join(ROOT, "tests", "cpp", "bvh_check.cpp")
    deps = [src, os.path.join(CSRC, "bvh.cpp"), os.path.join(CSRC, "bvh.h"), __file__]
    if os.path.exists(src) and (force or _stale(tool, deps)):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", "-pthread", f"-I{CSRC}",
                               src, os.path.join(CSRC, "bvh.cpp"), "-o", tool])
    return tool


def build_refit_check(force: bool = False) -> str:
    """tools/refit_check: tests/cpp/refit_check.cpp (which includes bvh_check.cpp for its invariants, walks and rays) over
    csrc/bvh.cpp with the host compiler -- refit_bvh's trees (tests/test_bvh_refit.py) and the refitted arrays the device
    tests compare with (tests/test_gpu_dynamic_scene.py); no device code."""
    tool = os.path.join(OUT, "tools", "refit_check")
    src = os.path.join(ROOT, "tests", "cpp", "refit_check.cpp")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "bvh_check.cpp"), os.path.join(CSRC, "bvh.cpp"),
            os.path.join(CSRC, "bvh.h"), __file__]
    if os.path.exists(src) and (force or _stale(tool, deps)):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", "-pthread", f"-I{CSRC}",
                               src, os.path.join(CSRC, "bvh.cpp"), "-o", tool])
    return tool


def build_shadow_lists_check(force: bool = False) -> str:
    """tools/shadow_lists_check: tests/cpp/shadow_lists_check.cpp over csrc/shadow_lists.h with the host compiler -- no
    record leaves out a triangle a ray of its family hits (tests/test_shadow_lists_host.py); no device code."""
    tool = os.path.join(OUT, "tools", "shadow_lists_check")
    src = os.path.join(ROOT, "tests", "cpp", "shadow_lists_check.cpp")
    deps = [src, os.path.join(CSRC, "shadow_lists.h"), __file__]
    if os.path.exists(src) and (force or _stale(tool, deps)):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", f"-I{CSRC}", src, "-o", tool])
    return tool


def build_shadow_vis_layout(force: bool = False) -> str:
    """tools/shadow_vis_layout: tests/cpp/shadow_vis_layout.cpp over csrc/shadow_vis.h with the host compiler -- the
    plane's indices as the header computes them (tests/test_shadow_vis_layout.py); no device code."""
    tool = os.path.join(OUT, "tools", "shadow_vis_layout")
    src = os.path.join(ROOT, "tests", "cpp", "shadow_vis_layout.cpp")
    deps = [src, os.path.join(CSRC, "shadow_vis.h"), __file__]
    if os.path.exists(src) and (force or _stale(tool, deps)):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", f"-I{CSRC}", src, "-o", tool])
    return tool


def build_phat_layout(force: bool = False) -> str:
    """tools/phat_layout: tests/cpp/phat_layout.cpp over csrc/phat_table.h with the host compiler -- the table's indices
    as the header computes them (tests/test_phat_layout.py); no device code."""
    tool = os.path.join(OUT, "tools", "phat_layout")
    src = os.path.join(ROOT, "tests", "cpp", "phat_layout.cpp")
    deps = [src, os.path.join(CSRC, "phat_table.h"), __file__]
    if os.path.exists(src) and (force or _stale(tool, deps)):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", f"-I{CSRC}", src, "-o", tool])
    return tool


def build_ris_ahead_key(force: bool = False) -> str:
    """tools/ris_ahead_key: tests/cpp/ris_ahead_key.cpp over csrc/ris_ahead.h with the host compiler -- the look-ahead
    key's comparison, one case per member (tests/test_ris_ahead_key.py); no device code, no HIP header."""
    tool = os.path.join(OUT, "tools", "ris_ahead_key")
    src = os.path.join(ROOT, "tests", "cpp", "ris_ahead_key.cpp")
    deps = [src, os.path.join(CSRC, "ris_ahead.h"), __file__]
    if os.path.exists(src) and (force or _stale(tool, deps)):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", f"-I{CSRC}", src, "-o", tool])
    return tool


def build_ris_batch_ring(force: bool = False) -> str:
    """tools/ris_batch_ring: tests/cpp/ris_batch_ring.cpp over csrc/ris_ahead.h with the host compiler -- the result
    ring and the two batch cadences walked over every reachable state (tests/test_ris_batch_ring.py); no device code."""
    tool = os.path.join(OUT, "tools", "ris_batch_ring")
    src = os.path.join(ROOT, "tests", "cpp", "ris_batch_ring.cpp")
    deps = [src, os.path.join(CSRC, "ris_ahead.h"), __file__]
    if os.path.exists(src) and (force or _stale(tool, deps)):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", f"-I{CSRC}", src, "-o", tool])
    return tool


def build_variant(name: str, defines: list[str], flags: list[str] | None = None) -> str:
    """Build _build/variants/<name>/libromis_amd.so with kernels.hip compiled under extra -D defines (launch-bound
    knobs such as ROMIS_SPATIAL_WPE) and compiler flags.  The host objects are the shipped ones."""
    build()
    vdir = os.path.join(OUT, "variants", name)
    os.makedirs(vdir, exist_ok=True)
    obj = os.path.join(vdir, "kernels.hip.o")
    subprocess.check_call([HIPCC] + COMMON + SOURCES[0][1] + [f"-D{d}" for d in defines] + list(flags or []) +
                          ["-c", os.path.join(CSRC, "kernels.hip"), "-o", obj])
    lib = os.path.join(vdir, "libromis_amd.so")
    objs = [obj] + [os.path.join(OUT, s + ".o") for s, _ in SOURCES[1:]]
    subprocess.check_call([HIPCC, "-shared", f"--offload-arch={ARCH}", "-fno-gpu-rdc", "-o", lib] + objs)
    return lib


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    args = ap.parse_args(argv)
    build(force=args.force, verbose=True)
    return 0



# C++ programs over the C++ binding (include/romis_amd/restir.hpp): the reference-side callers the C++ wrapper tests
# drive (tests/test_cpp_wrapper.py).  Built on the build host next to the library; the GPU box runs the prebuilt ones.
CPP_PROGRAMS = [("render_scene.cpp", "render_scene"), ("render_threads.cpp", "render_threads"),
                ("write_outputs.cpp", "write_outputs"), ("update_scene.cpp", "update_scene"),
                ("present_frames.cpp", "present_frames"), ("accumulate_frames.cpp", "accumulate_frames"),
                ("exact_image.cpp", "exact_image"), ("denoise_frames.cpp", "denoise_frames"),
                ("denoise_lum_frames.cpp", "denoise_lum_frames"), ("history_frames.cpp", "history_frames"),
                ("history_gather_frames.cpp", "history_gather_frames")]
CPP_DIR = os.path.join(ROOT, "tests", "cpp")


def build_cpp_program(src: str, out: str) -> str:
    """g++ one program against libromis_amd.so (rpath to the in-tree build) when it is older than its sources."""
    lib = LIB if os.path.exists(LIB) else build()
    libdir = os.path.dirname(lib)
    deps = [src, os.path.join(CPP_DIR, "scene_io.h"), os.path.join(ROOT, "include", "restir_c.h"),
            os.path.join(ROOT, "include", "romis_amd", "restir.hpp")]
    if _stale(out, deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-pthread", f"-I{os.path.join(ROOT, 'include')}",
                               src, "-o", out, f"-L{libdir}", "-lromis_amd", f"-Wl,-rpath,{libdir}"])
    return out


def build_cpp_programs() -> list[str]:
    return [build_cpp_program(os.path.join(CPP_DIR, src), os.path.join(OUT, out)) for src, out in CPP_PROGRAMS]

if __name__ == "__main__":
    sys.exit(main())
