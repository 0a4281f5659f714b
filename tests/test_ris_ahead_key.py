"""csrc/ris_ahead.h on the CPU: the key a RIS look-ahead result is stored under (DESIGN.md §6 "RIS look-ahead").

restir_render takes a look-ahead result only when the key of the frame it is about to render equals the stored one, so
a member that the comparison forgot would let a stale result through.  tools/ris_ahead_key (tests/cpp/ris_ahead_key.cpp)
changes one member at a time: every case must compare unequal, in both argument orders, and every word of the three
arrays on its own.  The struct's size and the header's member count are pinned here: a member added later without a
comparison and a case changes one of them.  The program is also built once with -fsanitize=address,undefined and run.
"""
import os
import subprocess

import pytest

from romis_amd import build

MEMBERS = ["seed", "frame", "gbuf_epoch", "scene_gen", "geom_gen", "phat_build", "cam", "width", "height", "tile", "tex_on",
           "features", "passes", "route_grid", "route_lds", "route_bits", "tuning_gen"]
# 4-byte members: 2 + cam 9 + 2 + tile 10 + 1 + features 22 + 1 + 3 = 50; 8-byte members: 5
SIZE = 4 * 50 + 8 * 5


def parse(text):
    out = {}
    for line in text.splitlines():
        name, *vals = line.split()
        out.setdefault(name, []).append([int(v) for v in vals])
    return out


@pytest.fixture(scope="module")
def lines():
    build.build_ris_ahead_key()
    tool = os.path.join(build.OUT, "tools", "ris_ahead_key")
    return parse(subprocess.run([tool], capture_output=True, text=True, timeout=60, check=True).stdout)


def test_a_key_equals_itself_and_its_copy(lines):
    assert lines["self"] == [[1]] and lines["copy"] == [[1]]


@pytest.mark.parametrize("member", MEMBERS)
def test_one_changed_member_makes_the_keys_unequal(lines, member):
    assert lines[member] == [[0]], f"{member}: the comparison does not see it"
    assert lines[member + "_swapped"] == [[0]]


def test_every_member_has_a_case(lines):
    """The header's count, the program's cases and this file's list agree, and the struct holds nothing else"""
    assert lines["fields"] == [[len(MEMBERS), SIZE]]   # "fields <count> <sizeof>"


def test_every_word_of_the_arrays_is_compared(lines):
    assert lines["cam_word"] == [[0]] * 9
    assert lines["tile_word"] == [[0]] * 10
    assert lines["features_word"] == [[0]] * 22


def test_the_next_frames_key_differs_in_the_frame_alone(lines):
    assert lines["next"] == [[1, 0]]
    assert lines["next_wraps"] == [[0]]   # frame indices wrap as restir_render's counter does
    assert lines["other_set"] == [[1, 0]]
    assert lines["cases"] == [[len(MEMBERS)]]


def test_under_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program (its own main) built with -fsanitize=address,undefined and run"""
    exe = tmp_path / "ris_ahead_key_san"
    src = os.path.join(build.ROOT, "tests", "cpp", "ris_ahead_key.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{build.CSRC}", src, "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines()[1] == "self 1"
