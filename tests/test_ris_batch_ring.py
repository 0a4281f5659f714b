"""csrc/ris_ahead.h on the CPU: the ring of look-ahead results and the batch cadences (DESIGN.md §6 "RIS batch").

A look-ahead launch may serve two frames, so up to three results wait in up to four plane sets.  A launch that wrote a
set a frame is reading, or one a result still waits in, would change that frame's image.  tools/ris_batch_ring
(tests/cpp/ris_batch_ring.cpp) walks every reachable state of restir_render's use of the header under frames.batch 1 and 2,
both cadence forms and two frames.batch_after values, with a drop of everything possible at every frame boundary, and
counts the violations: all must be zero.  It also pins the key of the n-th frame, the set choice and the discard
accounting (one per launch with a result nobody took).  The program is built once more with -fsanitize=address,undefined.
"""
import os
import subprocess

import pytest

from romis_amd import build


def parse(text):
    out = {}
    for line in text.splitlines():
        name, *vals = line.split()
        out.setdefault(name, []).append([int(v) for v in vals])
    return out


@pytest.fixture(scope="module")
def lines():
    build.build_ris_batch_ring()
    tool = os.path.join(build.OUT, "tools", "ris_batch_ring")
    return parse(subprocess.run([tool], capture_output=True, text=True, timeout=60, check=True).stdout)


def test_the_nth_key_differs_in_the_frame_alone(lines):
    # "nth n <frame is k.frame + n> <equal to k once the frame is put back> <equal to k as it is>"
    assert lines["nth"] == [[0, 1, 1, 1], [1, 1, 1, 0], [2, 1, 1, 0], [3, 1, 1, 0]]
    assert lines["nth_is_next"] == [[1]]
    assert lines["nth_wraps"] == [[1]]   # frame indices wrap as restir_render's counter does


def test_set_choice(lines):
    assert lines["pick"] == [[1, 1, 2]]        # set 0 read: the two lowest others
    assert lines["pick_b"] == [[1, 0, 3]]      # sets 1 and 2 busy
    assert lines["pick_full"] == [[0]]         # one free set of four: no room for two
    assert lines["pick_three_sets"] == [[0]]   # form a's three sets with two busy
    assert lines["sets"] == [[2, 2, 3, 4]]


def test_discards_count_launches(lines):
    assert lines["drop_both"] == [[1]]
    assert lines["drop_second"] == [[1]]
    assert lines["push_second_launch"] == [[1]]
    assert lines["busy"] == [[0b1111]]         # reading set 1; results wait in 2, 0 and 3
    assert lines["push_full"] == [[0, 3]]      # refused, nothing changed
    assert lines["drop_two_launches"] == [[2]]
    assert lines["drop_nothing"] == [[0, 0]]
    assert lines["find_after_drop"] == [[-1]]


@pytest.mark.parametrize("batch,form,max_pending,max_set", [(1, 0, 1, 1), (1, 1, 1, 1), (2, 0, 2, 2), (2, 1, 3, 3)])
def test_no_writer_gets_a_busy_set_in_any_reachable_state(lines, batch, form, max_pending, max_set):
    rows = [r for r in lines["walk"] if r[0] == batch and r[1] == form]
    assert len(rows) == 2   # frames.batch_after 3 and 8
    for _, _, after, states, launches, bad_sets, bad_takes, bad_keys, bad_discards, pend, mset in rows:
        assert states > 3 and launches > 0, after
        assert (bad_sets, bad_takes, bad_keys, bad_discards) == (0, 0, 0, 0), after
        assert pend == max_pending and mset == max_set, after
    assert lines["walk_low_after"] == [[0, 0, 0, 3]]


def test_under_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program (its own main) built with -fsanitize=address,undefined and run"""
    exe = tmp_path / "ris_batch_ring_san"
    src = os.path.join(build.ROOT, "tests", "cpp", "ris_batch_ring.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{build.CSRC}", src, "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines()[0] == "nth 0 1 1 1"
