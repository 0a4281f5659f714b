"""restir_last_error across the translation units behind include/restir_c.h (romis_amd/csrc: restir.cpp and layout.cpp
so far, over abi_error.cpp).  The error text is one thread-local string (abi_error.cpp) that every unit's failures set; a
unit with a copy of its own would leave restir_last_error with another call's text, or none.  Each case is an entry point
that fails on its arguments before any device call, one of layout.cpp and one per section of restir.cpp (so only the
boundary between those two units is crossed today): after a failure of another case's entry, calling it must return its status and leave its own
message.  abi_error.cpp itself has no failing entry (restir_last_error only reads the string), so it is covered through
the others.  CPU only."""
import ctypes as C

import pytest

from romis_amd import _abi

INVALID = 1


def _layout(lib):
    return lib.restir_layout_even(64, 64, 0, 1, C.byref(_abi.TileLayout()))


def _render(lib):
    return lib.restir_render(None, None, None, 64, 64, None, None, None, None)


def _scene(lib):
    return lib.restir_set_scene(None, None, 0, None, 0)


def _stage(lib):
    return lib.restir_stage_configure(None, 64, 64, 1)


def _halo(lib):
    return lib.restir_halo_pack(None, None, 0, 0)


def _frames(lib):
    return lib.restir_frame_retain(None)


def _mis(lib):
    f = _abi.default_features(ray_trace_mode=_abi.MODE_RMIS)
    return lib.restir_render_mis_tile(None, None, C.byref(f), 64, 64, None, None)


def _tuning(lib):
    return lib.restir_set_tuning(None, None, 0)


# (unit: subsystem, failing call, its message); neighbours in the list (and last / first) leave different messages
CASES = [
    ("layout.cpp", _layout, b"restir_tile_plan: bad arguments (W=64 H=64 tiles=0x1)"),
    ("restir.cpp: render", _render, b"ctx is NULL"),
    ("restir.cpp: stage", _stage, b"bad stage size"),
    ("restir.cpp: scene", _scene, b"ctx is NULL"),
    ("restir.cpp: halo", _halo, b"null argument"),
    ("restir.cpp: frames", _frames, b"frame is NULL"),
    ("restir.cpp: tuning", _tuning, b"null argument"),
    ("restir.cpp: mis", _mis, b"camera is NULL"),
]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_unit_failure_sets_the_shared_error_text(abi_lib, i):
    _, before, other = CASES[(i + 1) % len(CASES)]
    unit, call, message = CASES[i]
    assert other != message
    assert before(abi_lib) == INVALID
    assert abi_lib.restir_last_error() == other   # the previous call's text, from another unit
    assert call(abi_lib) == INVALID, unit
    assert abi_lib.restir_last_error() == message, unit


def test_every_unit_in_sequence(abi_lib):
    for unit, call, message in CASES + CASES[::-1]:
        assert call(abi_lib) == INVALID, unit
        assert abi_lib.restir_last_error() == message, unit
