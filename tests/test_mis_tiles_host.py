"""What R-MIS / R-OMIS screen tiles decide on the host, with no device: restir_render_mis_tile checks its arguments -- the
mode, the tile, its ghost ring, the image's R-OMIS window rule -- before it looks at the context, so a NULL context shows
each verdict; and distributed.MisTiles refuses a layout of another image before it touches the process group."""
import ctypes as C

import pytest

from romis_amd import _abi, scene

W, H = 48, 32
INVALID, UNSUPPORTED = 1, 5


def tile(abi_lib, tx, ty, rank, ghost, width=W, height=H):
    t = _abi.Tile()
    assert abi_lib.restir_tile_plan(width, height, tx, ty, rank, ghost, C.byref(t)) == 0
    return t


def call(abi_lib, f, t, width=W, height=H):
    cam = scene.camera_for("nightclub_128pt", width, height)
    st = abi_lib.restir_render_mis_tile(None, C.byref(cam), C.byref(f), width, height, C.byref(t) if t is not None else None,
                                        None)
    return st, abi_lib.restir_last_error().decode()


def test_render_mis_tile_argument_checks(abi_lib):
    romis = _abi.default_features(ray_trace_mode=_abi.MODE_ROMIS)
    rmis = _abi.default_features(ray_trace_mode=_abi.MODE_RMIS)
    r = romis.spatial_resample_radius
    # valid arguments reach the context check
    for f in (romis, rmis):
        for t in (tile(abi_lib, 2, 2, 3, r), tile(abi_lib, 4, 1, 1, r), tile(abi_lib, 2, 2, 0, r + 5), None):
            assert call(abi_lib, f, t) == (INVALID, "ctx is NULL")
    # a ghost ring narrower than the radius, on any side, for every strategy
    for f in (romis, rmis, _abi.default_features(ray_trace_mode=_abi.MODE_ROMIS, neighbour_selection_strategy=0)):
        st, msg = call(abi_lib, f, tile(abi_lib, 2, 2, 3, r - 1))
        assert st == INVALID and f"radius {r}" in msg
    t = tile(abi_lib, 2, 2, 0, r)
    t.gwidth -= 1
    st, msg = call(abi_lib, romis, t)
    assert st == INVALID and "radius" in msg
    # ... clipped at the image border: an owned rectangle at the corner needs no ring there
    t = tile(abi_lib, 2, 2, 0, r)
    assert (t.gx0, t.gy0) == (0, 0) and call(abi_lib, romis, t) == (INVALID, "ctx is NULL")
    # ReSTIR mode
    st, msg = call(abi_lib, _abi.default_features(), tile(abi_lib, 2, 2, 0, 2 * r))
    assert st == INVALID and "RMIS or ROMIS" in msg
    # inconsistent tiles
    for field, delta in [("width", W), ("global_width", 1), ("global_height", 1), ("gx0", 30), ("height", H)]:
        t = tile(abi_lib, 2, 2, 0, r)
        setattr(t, field, getattr(t, field) + delta)
        st, msg = call(abi_lib, romis, t)
        assert st == INVALID and ("inconsistent" in msg or "global size" in msg), (field, msg)
    t = tile(abi_lib, 2, 2, 0, r)
    t.width = 0
    assert call(abi_lib, romis, t)[0] == INVALID
    # more than RESTIR_ROMIS_MAX_TECHNIQUES techniques
    st, _ = call(abi_lib, _abi.default_features(ray_trace_mode=_abi.MODE_ROMIS, num_neighbours_to_sample=8), tile(abi_lib, 2, 2, 0, r))
    assert st == UNSUPPORTED
    # the R-OMIS corner rule is the image's: the centre tile of 3 x 3 is nowhere near a corner
    f1 = _abi.default_features(ray_trace_mode=_abi.MODE_ROMIS, spatial_resample_radius=1)
    st, msg = call(abi_lib, f1, tile(abi_lib, 3, 3, 4, 1))
    assert st == INVALID and "corner" in msg
    assert call(abi_lib, _abi.default_features(ray_trace_mode=_abi.MODE_RMIS, spatial_resample_radius=1),
                tile(abi_lib, 3, 3, 4, 1)) == (INVALID, "ctx is NULL")   # R-MIS has no such rule


def test_render_mis_tiles_argument_checks(abi_lib):
    romis = _abi.default_features(ray_trace_mode=_abi.MODE_ROMIS)
    cam = scene.camera_for("nightclub_128pt", W, H)
    out = (C.c_float * (W * H * 3))()
    L = _abi.TileLayout.from_cuts(W, H, {"x": [0, 19, 48], "y": [[0, 13, 32], [0, 13, 32]]})
    assert abi_lib.restir_render_mis_tiles(None, C.byref(cam), C.byref(romis), C.byref(L), out) == INVALID
    assert abi_lib.restir_last_error() == b"ctx is NULL"
    bad = _abi.TileLayout.from_cuts(W, H, {"x": [0, 19, 40], "y": [[0, 13, 32], [0, 13, 32]]})   # x cuts end short of W
    assert abi_lib.restir_render_mis_tiles(None, C.byref(cam), C.byref(romis), C.byref(bad), out) == INVALID
    assert abi_lib.restir_last_error() != b"ctx is NULL"
    assert abi_lib.restir_render_mis_tiles(None, C.byref(cam), C.byref(romis), C.byref(L), None) == INVALID


def test_mis_tiles_refuses_a_layout_of_another_image():
    from romis_amd import distributed
    f = _abi.default_features(ray_trace_mode=_abi.MODE_RMIS)
    L = _abi.TileLayout.from_cuts(W + 16, H, {"x": [0, 32, 64], "y": [[0, 16, 32], [0, 16, 32]]})
    with pytest.raises(ValueError, match=f"{W + 16}x{H}"):
        distributed.MisTiles(None, W, H, (2, 2), 0, f, layout=L)
    L = _abi.TileLayout.from_cuts(W, H, {"x": [0, 16, 32, 48], "y": [[0, 32]] * 3})
    with pytest.raises(ValueError, match="3x1 layout"):
        distributed.MisTiles(None, W, H, (2, 2), 0, f, layout=L)
