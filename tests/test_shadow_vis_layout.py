"""csrc/shadow_vis.h on the CPU: where the bit of (pixel, light) lies in the visibility plane.

tools/shadow_vis_layout (tests/cpp/shadow_vis_layout.cpp) prints the header's own numbers; this file restates the layout
in plain Python -- per-pixel records of (L + 31) // 32 words, the pixels tile by tile (32 x 16, row-major over the rect),
inside a tile in the order of the frame kernel's 512 threads: eight 8 x 8 waves, four across and two down, a wave's lanes
row-major -- and checks every (pixel, light) of a ragged 70 x 37 rect: the same index, distinct, in bounds, and the pair
read back from (index, bit).
"""
import os
import subprocess

import pytest

from romis_amd import build

RW, RH = 70, 37
LIGHTS = [1, 31, 32, 33, 128, 200, 254]


def py_words(L):
    return (L + 31) // 32


def py_slot(rw, x, y):
    ntx = (rw + 31) // 32
    tile = (y // 16) * ntx + x // 32
    lx, ly = x % 32, y % 16
    wave = (ly // 8) * 4 + lx // 8
    lane = (ly % 8) * 8 + lx % 8
    return tile * 512 + wave * 64 + lane


def py_pixel(rw, slot):
    """py_slot's inverse"""
    ntx = (rw + 31) // 32
    tile, t = divmod(slot, 512)
    wave, lane = divmod(t, 64)
    return (tile % ntx) * 32 + (wave % 4) * 8 + lane % 8, (tile // ntx) * 16 + (wave // 4) * 8 + lane // 8


@pytest.fixture(scope="module")
def tool():
    build.build_shadow_vis_layout()
    return os.path.join(build.OUT, "tools", "shadow_vis_layout")


@pytest.mark.parametrize("L", LIGHTS)
def test_every_pixel_and_light_has_its_own_bit(tool, L):
    out = subprocess.run([tool, str(RW), str(RH), str(L)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    head = out[0].split()
    words, size = int(head[1]), int(head[3])
    assert words == py_words(L) and 1 <= words <= 8
    tiles = ((RW + 31) // 32) * ((RH + 15) // 16)
    assert size == tiles * 512 * words
    px = [tuple(map(int, l.split())) for l in out[1:1 + RW * RH]]
    lights = [l.split() for l in out[1 + RW * RH:]]
    assert len(px) == RW * RH and len(lights) == L
    word_of, bit_of = {}, {}
    for k, (tag, i, w, b) in enumerate(lights):
        assert tag == "light" and int(i) == k
        word_of[k], bit_of[k] = int(w), int(b)
        assert word_of[k] == k // 32 < words and bit_of[k] == 1 << (k % 32)
    seen = set()
    for n, (x, y, slot, first, last) in enumerate(px):
        assert (x, y) == (n % RW, n // RW)
        assert slot == py_slot(RW, x, y)
        assert py_pixel(RW, slot) == (x, y)
        assert first == slot * words and last == slot * words + words - 1
        for i in range(L):   # every (pixel, light): a place of its own, inside the plane, that names the pair again
            idx, bit = slot * words + word_of[i], bit_of[i]
            assert 0 <= idx < size
            assert (idx, bit) not in seen
            seen.add((idx, bit))
            assert py_pixel(RW, idx // words) == (x, y) and (idx % words) * 32 + bit.bit_length() - 1 == i
    assert len(seen) == RW * RH * L
