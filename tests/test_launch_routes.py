"""The route functions of csrc/route.h choose what the launchers chose before them.

tests/golden/launch_routes.txt holds, for a matrix of scenes, features, regions, asks and knobs, what the five frame
launchers did when each still derived its own conditions (the file's header names the commit and the format), and what
the five predicates restir_render consulted returned.  tools/route_check (tests/cpp/route_check.cpp, built by
romis_amd.build) replays every row over route.h; this test compares the two, row by row.
"""
import os
import re
import subprocess

import pytest

from romis_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_routes.txt")
DEFAULTS = ["32,1,0,0,0,1", "100,200,1", "1,5,10,0,0,32", "1920,1080,1920,1080,1,2073600", "0", "0,0,0", "1,0"]


@pytest.fixture(scope="module")
def rows():
    tool = os.path.join(build.OUT, "tools", "route_check")
    if not os.path.exists(tool):
        tool = build.build_route_check()
    with open(GOLDEN) as fh:
        text = fh.read()
    new = subprocess.run([tool], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    old = [l for l in text.splitlines() if l and not l.startswith("#")]
    assert len(old) == len(new) > 1200
    pairs = []
    for o, n in zip(old, new):
        (oi, oo), (ni, no) = o.split(" | "), n.split(" | ")
        assert oi == ni
        inp = oi.split()   # stage, then eight groups; "-" is a group's default (tests/cpp/route_rows.h)
        pairs.append(([inp[0]] + [d if g == "-" else g for g, d in zip(inp[1:8], DEFAULTS)] + inp[8:], oo, no))
    return pairs


def _plain(inp):
    """A rect that is not empty (a frame path never has one; a route then names no kernel), in SoA planes whose 16-byte
    offsets fit 32 bits: the region facts restir_render tested beside the predicates (!fb.records, view pixels * 16 <=
    0xFFFFFFFF), which the routes now test themselves."""
    n = int(inp[3].split(",")[0])
    vw, vh, rw, rh, ps, js = (int(v) for v in inp[4].split(","))
    return rw * rh > 0 and ps == 1 and vw * vh * 16 + (js * 16 if n == 2 else 0) <= 0xFFFFFFFF


def test_every_launch_matches(rows):
    """Kernel, grid, block, LDS, the out-parameters' values, map2d / xcd_rows / xcd_cols, which pointers reach the kernel,
    the skip_res / res_dead / mode words, MissTiles m / gbuf and miss_shade_zero: equal wherever the launcher launched or
    had nothing to launch."""
    seen = set()
    for inp, old, new in rows:
        if inp[0] == "pred" or " einval " in old:
            continue
        new = re.sub(r"( (hk|ok|gb)=\S+)+$", "", new)
        assert new == old, " ".join(inp)
        seen.add(old.split()[0])
    assert len(seen) == 84, len(seen)   # the 83 kernels of the five launchers, and "-"


def test_invalid_value_rows_are_excluded_by_the_frame_decision(rows):
    """Where a launcher returned hipErrorInvalidValue its caller had asked for something the frame-level decision rules
    out: the fused kernels when their route is not ok, input handles of a kind spatial_handle_kind does not yield."""
    n = 0
    for inp, old, new in rows:
        if " einval " not in old:
            continue
        n += 1
        if inp[0] in ("pris", "prist"):
            assert new.endswith(" ok=0"), " ".join(inp)
        else:
            assert inp[0] == "spatial" and int(inp[5], 16) & 2, " ".join(inp)   # input handles asked
            got, asked = re.search(r" hk=(-?\d+)/(\d)$", new).groups()
            assert got != asked, " ".join(inp)
    assert n > 100


def test_cached_gbuffer_route_names_the_fused_member(rows):
    """Over a cached G-buffer (Ask::gbuf_cached) a fused primary + RIS route names the same member of the k_gbuf_ris
    family in the same launch shape.  Expected from the golden row alone: its kernel under the other prefix, its grid,
    block and map=, and its LDS less the BVH's (2 num_nodes + 3 num_tris) float4s -- the rows have no initial-visibility
    rays, so the cached kernel stages no BVH."""
    fused, seen, n = set(), set(), 0
    for inp, old, new in rows:
        if inp[0] not in ("pris", "prist"):
            continue
        where = " ".join(inp)
        got = re.search(r" gb=(\S+)$", new)
        o = old.split()
        if o[4] != "launch":
            assert not got, where
            continue
        n += 1
        fused.add(o[0])
        assert o[0].startswith("k_primary_ris_") and got, where
        nodes, tris, _ = (int(v) for v in inp[2].split(","))
        map2d, xcd_rows, xcd_cols = re.search(r" map=(\d+),(\d+),(\d+) ", old).groups()
        want = ["k_gbuf_ris_" + o[0][len("k_primary_ris_"):], str(int(o[3]) - (2 * nodes + 3 * tris) * 16), o[1], o[2], map2d,
                xcd_rows, xcd_cols]
        assert got.group(1).split(",") == want, where
        seen.add(got.group(1).split(",")[0])
    assert n > 100
    assert len(fused) == 22 and seen == {"k_gbuf_ris_" + k[len("k_primary_ris_"):] for k in fused}, sorted(seen)


def test_predicates_are_reads_of_routes(rows):
    """spatial_reads_flags = the pass route's bg_known, final_reads_flags = the final route's flags (N = 1, its only
    use), primary_ris_fits / primary_ris_temporal_fits = the fused routes' ok, spatial_handle_kind as before -- now with
    the region and BVH facts the frame path used to test beside it, so there it may only say no."""
    n = 0
    for inp, old, new in rows:
        if inp[0] != "pred":
            continue
        n += 1
        o = {k: int(v) for k, v in (kv.split("=") for kv in old.split())}
        g = {k: int(v) for k, v in (kv.split("=") for kv in new.split())}
        where = " ".join(inp)
        assert g["prf"] == o["prf"] and g["prtf"] == o["prtf"], where
        if inp[3].split(",")[0] == "1" and int(inp[4].split(",")[2]):
            assert g["frf"] == o["frf"], where
        if _plain(inp):
            assert g["srf"] == o["srf"], where
        else:
            assert g["srf"] == 0, where
        if _plain(inp) and o["prf"]:
            assert g["hk"] == o["hk"], where
        else:
            assert g["hk"] == -1, where
    assert n > 300
