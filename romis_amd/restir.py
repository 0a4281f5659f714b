"""Python host binding of the C ABI (include/restir_c.h) -- mirrors the reference's render surface.

    renderer = Renderer(device=0)
    renderer.set_scene(scene)                                  # EmbreeInterface(scene) (embree_interface.cpp:14-51)
    rgb, grid = renderer.render_restir(prev_grid, camera, W, H, features)   # renderReSTIR (render.cpp:28-62)

Errors raise RestirError (the reference throws std::runtime_error, render.cpp:99/278).  Everything runs in
libromis_amd.so on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import RestirError, check  # noqa: F401


class ReservoirGrid:
    """Device-resident ReservoirGrid (reservoir.h:75) -- a reference-counted restir_frame handle."""

    def __init__(self, lib, handle):
        self._lib = lib
        self.handle = handle

    def __del__(self):
        if getattr(self, "handle", None):
            self._lib.restir_frame_release(self.handle)
            self.handle = None

    def info(self) -> dict:
        """(W, H) of the image and the (vx0, vy0, vw, vh) view the grid covers, N sub-reservoirs per pixel."""
        v = [C.c_uint32() for _ in range(7)]
        check(self._lib, self._lib.restir_frame_info(self.handle, *[C.byref(x) for x in v]), "restir_frame_info")
        return dict(zip(("W", "H", "vx0", "vy0", "vw", "vh", "N"), (x.value for x in v)))

    def download(self):
        """The grid's (pos [N][vh][vw][3], color [N][vh][vw][3], W [N][vh][vw], M [N][vh][vw] uint32), rows y = 0
        bottom -- the per-pixel Reservoir state renderReSTIR returns (render.cpp:61)."""
        i = self.info()
        n = i["N"] * i["vh"] * i["vw"]
        pos, col = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        w, m = np.zeros(n, np.float32), np.zeros(n, np.uint32)
        FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        check(self._lib, self._lib.restir_frame_download(self.handle, pos.ctypes.data_as(FP), col.ctypes.data_as(FP),
                                                         w.ctypes.data_as(FP), m.ctypes.data_as(UP)),
              "restir_frame_download")
        shp = (i["N"], i["vh"], i["vw"])
        return pos.reshape(shp + (3,)), col.reshape(shp + (3,)), w.reshape(shp), m.reshape(shp)


class PresentedImage:
    """A snapshot of a Renderer's last image on its way to pinned host memory (restir_image_begin): the next frame may
    be enqueued at once.  ready() never blocks; wait() blocks on this snapshot's copy only and returns a numpy view of
    the pinned bytes -- (H, W, 4) uint8 for "rgba8" / "bgra8_bottom_up", (H, W, 3) float32 for "rgb32f" -- valid until
    release().  A context manager (release on exit); keeps its Renderer alive.  Closing the Renderer invalidates it."""

    def __init__(self, renderer: "Renderer", handle):
        self._renderer = renderer
        self._lib = renderer.lib
        self.handle = handle
        w, h, fmt, n = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(self._lib, self._lib.restir_image_info(handle, C.byref(w), C.byref(h), C.byref(fmt), C.byref(n)),
              "restir_image_info")
        self.width, self.height, self.format, self.nbytes = w.value, h.value, fmt.value, n.value

    def _live(self):
        if not self.handle or not self._renderer.ctx:
            raise RestirError("the presented image has been released (or its Renderer closed)")
        return self.handle

    def ready(self) -> bool:
        r = C.c_int()
        check(self._lib, self._lib.restir_image_ready(self._live(), C.byref(r)), "restir_image_ready")
        return bool(r.value)

    def wait(self) -> np.ndarray:
        p = C.c_void_p()
        check(self._lib, self._lib.restir_image_wait(self._live(), C.byref(p)), "restir_image_wait")
        buf = (C.c_uint8 * self.nbytes).from_address(p.value)
        if self.format == _abi.IMAGE_RGB32F:
            return np.frombuffer(buf, np.float32).reshape(self.height, self.width, 3)
        return np.frombuffer(buf, np.uint8).reshape(self.height, self.width, 4)

    def release(self) -> None:
        if getattr(self, "handle", None):
            if self._renderer.ctx:   # a closed Renderer freed the slots itself
                self._lib.restir_image_release(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        self.release()


class Renderer:
    def __init__(self, device: int = 0):
        self.lib = _abi.load_library()
        h = C.c_void_p()
        check(self.lib, self.lib.restir_create(device, C.byref(h)), "restir_create")
        self.ctx = h
        self._scene_keep = None
        self.stage_shape = None

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.restir_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        self.close()

    # ---- scene / seed -------------------------------------------------------------------------------
    def set_scene(self, scene) -> None:
        """EmbreeInterface(scene): meshes, lights and the Images of textured materials (restir_set_scene_textured)."""
        meshes, nm, lights, nl, keep = scene.to_abi()
        texs, ntex, tkeep = scene.textures_abi()
        check(self.lib, self.lib.restir_set_scene_textured(self.ctx, meshes, nm, lights, nl, texs, ntex),
              "restir_set_scene_textured")
        self._scene_keep = (meshes, lights, keep, texs, tkeep)

    def update_meshes(self, meshes: dict) -> None:
        """restir_update_meshes: {mesh index: (positions [V][3], normals [V][3] or None)} -- new vertex positions (and
        normals) for meshes of the scene set; the device refits the BVH, nothing is rebuilt or uploaded again."""
        FP = C.POINTER(C.c_float)
        ups = (_abi.MeshUpdate * max(1, len(meshes)))()
        keep = []
        for i, (m, (pos, nrm)) in enumerate(meshes.items()):
            p = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
            keep.append(p)
            ups[i].mesh, ups[i].num_vertices, ups[i].positions = int(m), len(p), p.ctypes.data_as(FP)
            if nrm is not None:
                n = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3)
                if len(n) != len(p):
                    raise ValueError(f"mesh {m}: {len(n)} normals for {len(p)} positions")
                keep.append(n)
                ups[i].normals = n.ctypes.data_as(FP)
        check(self.lib, self.lib.restir_update_meshes(self.ctx, ups, len(meshes)), "restir_update_meshes")

    def set_lights(self, lights) -> None:
        """restir_set_lights: another list of _abi.Light over the same geometry; the BVH and the kept G-buffer stay."""
        arr = (_abi.Light * max(1, len(lights)))()
        for i, l in enumerate(lights):
            arr[i] = l
        check(self.lib, self.lib.restir_set_lights(self.ctx, arr, len(lights)), "restir_set_lights")

    def debug_scene(self) -> dict:
        """restir_debug_scene_download: the device's scene arrays as they stand -- nodes [n][8] float32, nodes_q [n][4]
        uint32 (None without quantized nodes), tri_v0 / tri_e1 / tri_e2 [T][4] in BVH order, tri_n0 / tri_n1 / tri_n2
        [T][4] in the upload's order."""
        info = self.scene_info()
        n, t = info.num_nodes, info.num_tris
        out = {"nodes": np.zeros((n, 8), np.float32), "nodes_q": np.zeros((n, 4), np.uint32) if info.nodes_q_ok else None}
        for k in ("tri_v0", "tri_e1", "tri_e2", "tri_n0", "tri_n1", "tri_n2"):
            out[k] = np.zeros((t, 4), np.float32)
        FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        ptr = lambda a, ty: a.ctypes.data_as(ty) if a is not None and a.size else None
        check(self.lib, self.lib.restir_debug_scene_download(
            self.ctx, ptr(out["nodes"], FP), ptr(out["nodes_q"], UP),
            *[ptr(out[k], FP) for k in ("tri_v0", "tri_e1", "tri_e2", "tri_n0", "tri_n1", "tri_n2")]),
            "restir_debug_scene_download")
        return out

    def scene_info(self) -> _abi.SceneInfo:
        """restir_scene_info: what set_scene derived from the scene -- BVH size and LDS bytes, the light types present,
        the compact light-table forms it qualifies for, light_scale, nodes_q_ok (the shadow rays' quantized nodes
        exist).  Runs no kernel."""
        info = _abi.SceneInfo()
        check(self.lib, self.lib.restir_scene_info(self.ctx, C.byref(info)), "restir_scene_info")
        return info

    def set_seed(self, seed: int = _abi.RESTIR_DEFAULT_SEED, frame: int = 0) -> None:
        check(self.lib, self.lib.restir_set_seed(self.ctx, seed, frame), "restir_set_seed")

    def set_renders_dir(self, path) -> None:
        """The reference's RENDERS_DIR for file side outputs (None = none): R-OMIS renders with
        save_alphas_visualisation write visualiseAlphas' bitmaps there after every iteration."""
        d = None if path is None else os.fsencode(path)
        check(self.lib, self.lib.restir_set_renders_dir(self.ctx, d), "restir_set_renders_dir")

    # ---- frame ----------------------------------------------------------------------------------------
    def render_restir(self, prev: ReservoirGrid | None, camera, width: int, height: int, features,
                      tile=None, want_rgb: bool = True, want_grid: bool = True):
        """renderReSTIR: returns (rgb [h][w][3] row 0 = top, or None; ReservoirGrid or None)."""
        out = C.c_void_p()
        rgb = None
        rgb_ptr = None
        if want_rgb:
            h_ = tile.height if tile is not None else height
            w_ = tile.width if tile is not None else width
            rgb = np.zeros((h_, w_, 3), np.float32)
            rgb_ptr = rgb.ctypes.data_as(C.POINTER(C.c_float))
        st = self.lib.restir_render(self.ctx, C.byref(camera), C.byref(features), width, height,
                                    C.byref(tile) if tile is not None else None,
                                    prev.handle if prev is not None else None,
                                    C.byref(out) if want_grid else None, rgb_ptr)
        check(self.lib, st, "restir_render")
        grid = ReservoirGrid(self.lib, out) if want_grid and out.value else None
        return rgb, grid

    def reproject(self, prev: ReservoirGrid, cam_prev, cam_cur, want_map: bool = False):
        """restir_frame_reproject: a new predecessor grid for a camera that moved from cam_prev to cam_cur -- at each
        pixel the reservoirs of `prev` at the pixel where the current surface point was seen from cam_prev, or empty
        ones.  Pass it to render_restir as `prev`.  want_map: returns (grid, map [h][w] uint32, rows y = 0 bottom) with
        the source pixel's flat index or 0xFFFFFFFF - reason (0 miss, 1 behind, 2 off-screen, 3 predecessor miss,
        4 depth, 5 normal), and synchronises."""
        out = C.c_void_p()
        smap = None
        if want_map:
            i = prev.info()
            smap = np.zeros((i["H"], i["W"]), np.uint32)
        check(self.lib, self.lib.restir_frame_reproject(self.ctx, prev.handle, C.byref(cam_prev), C.byref(cam_cur), C.byref(out),
                                                        smap.ctypes.data_as(C.POINTER(C.c_uint32)) if want_map else None),
              "restir_frame_reproject")
        grid = ReservoirGrid(self.lib, out)
        return (grid, smap) if want_map else grid

    def synchronize(self) -> None:
        check(self.lib, self.lib.restir_synchronize(self.ctx), "restir_synchronize")

    def download_rgb(self, width: int, height: int) -> np.ndarray:
        rgb = np.zeros((height, width, 3), np.float32)
        check(self.lib, self.lib.restir_download_rgb(self.ctx, rgb.ctypes.data_as(C.POINTER(C.c_float)), rgb.size),
              "restir_download_rgb")
        return rgb

    # ---- presenting a frame (include/restir_c.h "presenting a frame") ---------------------------------
    def present(self, format: str | int = "rgba8") -> PresentedImage:
        """restir_image_begin: a snapshot of the last image as "rgba8", "bgra8_bottom_up" or "rgb32f", converted on the
        device and copied to pinned memory behind the frame that produced it; returns without synchronising."""
        fmt = _abi.IMAGE_FORMATS[format] if isinstance(format, str) else int(format)
        h = C.c_void_p()
        check(self.lib, self.lib.restir_image_begin(self.ctx, fmt, C.byref(h)), "restir_image_begin")
        return PresentedImage(self, h)

    def download_rgba8(self, width: int | None = None, height: int | None = None) -> np.ndarray:
        """The last image as (H, W, 4) uint8 -- restir_rgb_to_rgba8's bytes, converted on the device.  With the image's
        size (as download_rgb takes it) this is restir_download_rgba8; without, a snapshot that tells its own size,
        waited for and copied."""
        if width is None or height is None:
            with self.present("rgba8") as im:
                return im.wait().copy()
        out = np.zeros((height, width, 4), np.uint8)
        check(self.lib, self.lib.restir_download_rgba8(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)), width * height),
              "restir_download_rgba8")
        return out

    def write_bmp(self, path) -> None:
        """restir_write_image_bmp: the last image as the BMP file Screen::writeBitmapToFile writes."""
        check(self.lib, self.lib.restir_write_image_bmp(self.ctx, os.fsencode(path)), "restir_write_image_bmp")

    # ---- accumulating frames (include/restir_c.h "accumulating frames") -------------------------------
    def accum_begin(self, variance: bool = True) -> None:
        """restir_accum_begin: start (or restart) an accumulation with an empty state -- a running mean per float of the
        image and, with `variance`, the sum of squared deviations the stats need."""
        check(self.lib, self.lib.restir_accum_begin(self.ctx, _abi.RESTIR_ACCUM_VARIANCE if variance else 0),
              "restir_accum_begin")

    def accum_add(self) -> None:
        """restir_accum_add: fold the last image in, on the device; only enqueues.  Render the frames with
        enable_tone_mapping = 0 and tone map the mean (accum_resolve)."""
        check(self.lib, self.lib.restir_accum_add(self.ctx), "restir_accum_add")

    def accum_resolve(self, features=None) -> None:
        """restir_accum_resolve: the mean becomes the last image -- tone mapped by `features`' enable_tone_mapping /
        gamma / exposure, or its own bits without --, which download_rgb, present, download_rgba8 and write_bmp serve."""
        check(self.lib, self.lib.restir_accum_resolve(self.ctx, C.byref(features) if features is not None else None),
              "restir_accum_resolve")

    def accum_stats(self) -> _abi.AccumStats:
        """restir_accum_stats_get (needs the variance and two frames; synchronises): est_mse, the estimate of
        E|mean - expectation|^2 per float, mean_value and the nonfinite floats left out of both."""
        s = _abi.AccumStats()
        check(self.lib, self.lib.restir_accum_stats_get(self.ctx, C.byref(s)), "restir_accum_stats_get")
        return s

    def accum_state(self, width: int | None = None, height: int | None = None):
        """restir_accum_download: (mean, m2), each [height][width][3] float32, as the state stands (m2 zeros for an
        accumulation without the variance); synchronises.  width x height is the accumulated images' size; without it
        the size is asked of accum_stats(), which needs the variance and two frames."""
        if width is None or height is None:
            s = self.accum_stats()
            width, height = s.width, s.height
        mean, m2 = np.zeros((height, width, 3), np.float32), np.zeros((height, width, 3), np.float32)
        FP = C.POINTER(C.c_float)
        check(self.lib, self.lib.restir_accum_download(self.ctx, mean.ctypes.data_as(FP), m2.ctypes.data_as(FP), mean.size),
              "restir_accum_download")
        return mean, m2

    def accum_end(self) -> None:
        """restir_accum_end: close the accumulation and free its buffers."""
        check(self.lib, self.lib.restir_accum_end(self.ctx), "restir_accum_end")

    def render_accumulated(self, camera, width: int, height: int, features, frames: int, target_mse: float = 0.0,
                           min_frames: int = 0, check_every: int = 8, variance: bool = True, tile=None,
                           want_rgb: bool = True):
        """restir_render_accumulate: a fresh accumulation of up to `frames` frames of one view, each rendered without
        tone mapping and added on the device with no synchronisation between them (with temporal_reuse each frame's grid
        is the next one's predecessor), then resolved with `features`' tone-mapping fields.  With target_mse > 0 (needs
        `variance`) the stats are taken after frame min_frames and then every check_every frames and the loop stops once
        est_mse <= target_mse.  Returns (rgb [h][w][3] of the resolved image or None, AccumStats); the accumulation stays
        open."""
        req = _abi.AccumRequest(flags=_abi.RESTIR_ACCUM_VARIANCE if variance else 0, min_frames=min_frames,
                                max_frames=frames, check_every=check_every, target_mse=target_mse)
        stats = _abi.AccumStats()
        rgb = None
        if want_rgb:
            h_ = tile.height if tile is not None else height
            w_ = tile.width if tile is not None else width
            rgb = np.zeros((h_, w_, 3), np.float32)
        check(self.lib, self.lib.restir_render_accumulate(
            self.ctx, C.byref(camera), C.byref(features), width, height, C.byref(tile) if tile is not None else None,
            C.byref(req), C.byref(stats), rgb.ctypes.data_as(C.POINTER(C.c_float)) if want_rgb else None),
            "restir_render_accumulate")
        return rgb, stats

    # ---- the exact image and error figures (include/restir_c.h "the exact direct-lighting image") ------
    def render_exact(self, camera, width: int, height: int, features, tile=None, download: bool = True):
        """restir_render_exact: the exact direct-lighting image of a point-light scene -- per pixel the float32 sum, in
        light-table order, of computeShading times visibility over every light, tone mapped by `features` -- written as
        the context's image (a producer: accum_add, present, download_rgb and write_bmp serve it).  Only `features`'
        shading, texture and tone-mapping fields are read; no frame index is consumed.  Returns rgb [h][w][3] (row 0 =
        top) of the tile's owned rectangle, or None with download=False, which only enqueues."""
        rgb = None
        if download:
            h_ = tile.height if tile is not None else height
            w_ = tile.width if tile is not None else width
            rgb = np.zeros((h_, w_, 3), np.float32)
        check(self.lib, self.lib.restir_render_exact(
            self.ctx, C.byref(camera), C.byref(features), width, height, C.byref(tile) if tile is not None else None,
            rgb.ctypes.data_as(C.POINTER(C.c_float)) if download else None), "restir_render_exact")
        return rgb

    def reference_set(self) -> None:
        """restir_reference_set: keep a device copy of the last image as the reference error() compares with; enqueues."""
        check(self.lib, self.lib.restir_reference_set(self.ctx), "restir_reference_set")

    def reference_clear(self) -> None:
        """restir_reference_clear: free the kept reference."""
        check(self.lib, self.lib.restir_reference_clear(self.ctx), "restir_reference_clear")

    def reference_info(self):
        """restir_reference_info: (width, height, present) of the kept reference."""
        w, h, present = C.c_uint32(), C.c_uint32(), C.c_int()
        check(self.lib, self.lib.restir_reference_info(self.ctx, C.byref(w), C.byref(h), C.byref(present)),
              "restir_reference_info")
        return w.value, h.value, bool(present.value)

    def error(self, source: str | int = "image") -> _abi.ErrorStats:
        """restir_error_get (synchronises): true MSE, MAE, relative MSE, bias and the largest deviation of the last image
        ("image") or of the open accumulation's mean ("accum") against the kept reference, reduced on the device."""
        src = {"image": _abi.RESTIR_ERROR_SRC_IMAGE, "accum": _abi.RESTIR_ERROR_SRC_ACCUM_MEAN}[source] \
            if isinstance(source, str) else int(source)
        s = _abi.ErrorStats()
        check(self.lib, self.lib.restir_error_get(self.ctx, src, C.byref(s)), "restir_error_get")
        return s

    # ---- denoising the last image (include/restir_c.h "denoising the last image") ----------------------
    def denoise(self, camera, width: int, height: int, tile=None, params=None, tone=None, download: bool = True):
        """restir_denoise: the edge-avoiding a-trous filter over the context's last image, in place, guided by the
        normal, position and material of `camera`'s G-buffer (traced once per view and kept).  params: a
        DenoiseParams (None: the defaults); tone: a Features whose tone-mapping fields are applied after the last level
        (None: none).  The result is marked like a resolve: present, download_rgb, write_bmp, reference_set and error
        serve it, accum_add refuses it.  Returns rgb [h][w][3] (row 0 = top) of the tile's owned rectangle, or None
        with download=False, which only enqueues."""
        if params is None:
            params = denoise_params()
        rgb = None
        if download:
            h_ = tile.height if tile is not None else height
            w_ = tile.width if tile is not None else width
            rgb = np.zeros((h_, w_, 3), np.float32)
        check(self.lib, self.lib.restir_denoise(
            self.ctx, C.byref(camera), width, height, C.byref(tile) if tile is not None else None, C.byref(params),
            C.byref(tone) if tone is not None else None,
            rgb.ctypes.data_as(C.POINTER(C.c_float)) if download else None), "restir_denoise")
        return rgb

    def denoise_lum(self, camera, width: int, height: int, tile=None, params=None, tone=None, download: bool = True):
        """restir_denoise_lum: denoise() with a variance-guided luminance term.  params: a DenoiseLumParams (None: the
        defaults); with variance_source = RESTIR_DENOISE_VAR_ACCUM the image is the open accumulation's mean and the
        variance comes from its m2, otherwise the last image is filtered with a variance estimated from it.  Returns
        rgb [h][w][3] (row 0 = top) of the tile's owned rectangle, or None with download=False, which only enqueues."""
        if params is None:
            params = denoise_lum_params()
        rgb = None
        if download:
            h_ = tile.height if tile is not None else height
            w_ = tile.width if tile is not None else width
            rgb = np.zeros((h_, w_, 3), np.float32)
        check(self.lib, self.lib.restir_denoise_lum(
            self.ctx, C.byref(camera), width, height, C.byref(tile) if tile is not None else None, C.byref(params),
            C.byref(tone) if tone is not None else None,
            rgb.ctypes.data_as(C.POINTER(C.c_float)) if download else None), "restir_denoise_lum")
        self._denoise_lum_shape = (tile.height, tile.width) if tile is not None else (height, width)
        return rgb

    def denoise_lum_variance(self) -> np.ndarray:
        """restir_denoise_lum_variance_download: the last denoise_lum's final variance plane [h][w] (row 0 = top) of its
        owned rectangle; synchronises.  A test hook."""
        shape = getattr(self, "_denoise_lum_shape", None)
        if shape is None:
            raise RuntimeError("denoise_lum_variance before denoise_lum")
        var = np.zeros(shape, np.float32)
        check(self.lib, self.lib.restir_denoise_lum_variance_download(self.ctx, var.ctypes.data_as(C.POINTER(C.c_float)), var.size),
              "restir_denoise_lum_variance_download")
        return var

    def denoise_guide_builds(self) -> int:
        """restir_denoise_guide_builds: how often denoise() traced its guides (a still view traces them once)."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_denoise_guide_builds(self.ctx, C.byref(n)), "restir_denoise_guide_builds")
        return n.value

    # ---- a reprojected image history (include/restir_c.h "a reprojected image history") --------------
    def history_begin(self, params=None) -> None:
        """restir_history_begin: open (or restart) an empty image history -- per pixel a mean, the variance of the samples
        and a count, which history_advance carries from camera to camera.  params: a HistoryParams (None: the defaults)."""
        if params is None:
            params = history_params()
        check(self.lib, self.lib.restir_history_begin(self.ctx, C.byref(params)), "restir_history_begin")

    def history_advance(self, camera, width: int, height: int, want_map: bool = False):
        """restir_history_advance: move the history to `camera` -- the camera the last image was rendered with -- and fold
        that image in; only enqueues.  Render the frames with enable_tone_mapping = 0.  want_map: returns the map [h][w]
        uint32 (rows y = 0 bottom) with the source pixel's flat index or 0xFFFFFFFF - reason (restir_frame_reproject's 0 -
        5, 6 material, 7 no history), and synchronises."""
        smap = np.zeros((height, width), np.uint32) if want_map else None
        check(self.lib, self.lib.restir_history_advance(self.ctx, C.byref(camera), width, height,
                                                        smap.ctypes.data_as(C.POINTER(C.c_uint32)) if want_map else None),
              "restir_history_advance")
        self._history_shape = (height, width)
        return smap

    def history_gather(self, mode: int | None = None) -> int:
        """restir_history_gather_set / _get: how history_advance gathers the kept state -- HISTORY_GATHER_NEAREST (the
        default) from the nearest source pixel, HISTORY_GATHER_BILINEAR from the 2 x 2 records around the continuous source
        position.  Sets the mode when one is given; returns the current mode.  Context state: it holds until set again,
        across history_begin / history_end and resets."""
        if mode is not None:
            check(self.lib, self.lib.restir_history_gather_set(self.ctx, int(mode)), "restir_history_gather_set")
        g = C.c_uint32()
        check(self.lib, self.lib.restir_history_gather_get(self.ctx, C.byref(g)), "restir_history_gather_get")
        return g.value

    def history_resolve(self, features=None) -> None:
        """restir_history_resolve: the history's mean becomes the last image -- tone mapped by `features`, or its own bits
        without."""
        check(self.lib, self.lib.restir_history_resolve(self.ctx, C.byref(features) if features is not None else None),
              "restir_history_resolve")

    def history_denoise(self, params=None, tone=None, download: bool = True):
        """restir_history_denoise: denoise_lum's levels over the history's mean for the last advance's view, the initial
        variance taken from the history (a pixel with a short history takes the spatial estimate).  Returns rgb [h][w][3]
        (row 0 = top), or None with download=False, which only enqueues; denoise_lum_variance serves the final plane."""
        if params is None:
            params = denoise_lum_params()
        shape = getattr(self, "_history_shape", None)
        if shape is None:
            raise RuntimeError("history_denoise before history_advance")
        rgb = np.zeros(shape + (3,), np.float32) if download else None
        check(self.lib, self.lib.restir_history_denoise(
            self.ctx, C.byref(params), C.byref(tone) if tone is not None else None,
            rgb.ctypes.data_as(C.POINTER(C.c_float)) if download else None), "restir_history_denoise")
        self._denoise_lum_shape = shape
        return rgb

    def history_state(self):
        """restir_history_download: (mean [h][w][3] float32, S [h][w][3] float32, n [h][w] uint32) in image rows as the
        last advance left them; synchronises.  A test hook."""
        shape = getattr(self, "_history_shape", None)
        if shape is None:
            raise RuntimeError("history_state before history_advance")
        mean, S, n = np.zeros(shape + (3,), np.float32), np.zeros(shape + (3,), np.float32), np.zeros(shape, np.uint32)
        FP = C.POINTER(C.c_float)
        check(self.lib, self.lib.restir_history_download(self.ctx, mean.ctypes.data_as(FP), S.ctypes.data_as(FP),
                                                         n.ctypes.data_as(C.POINTER(C.c_uint32)), n.size),
              "restir_history_download")
        return mean, S, n

    def history_frames(self) -> tuple[int, int]:
        """restir_history_frames: (advances, resets) since history_begin."""
        a, r = C.c_uint64(), C.c_uint64()
        check(self.lib, self.lib.restir_history_frames(self.ctx, C.byref(a), C.byref(r)), "restir_history_frames")
        return a.value, r.value

    def history_end(self) -> None:
        """restir_history_end: close the history and free its planes."""
        check(self.lib, self.lib.restir_history_end(self.ctx), "restir_history_end")

    # ---- halo-mode frames (include/restir_c.h "halo-mode frames") -------------------------------------
    def halo_begin(self, prev, camera, width, height, features, tiles, rank, layout=None):
        """Primary rays on the tile + ring, RIS / temporal on the owned tile.  Returns (send_bytes, recv_bytes).
        layout: an uneven restir_tile_layout (layout_balanced) instead of the even tiles split."""
        sb, rb_ = C.c_uint64(), C.c_uint64()
        ph = prev.handle if prev is not None else None
        if layout is not None:
            check(self.lib, self.lib.restir_halo_begin_layout(self.ctx, C.byref(camera), C.byref(features), C.byref(layout),
                                                              rank, ph, C.byref(sb), C.byref(rb_)), "restir_halo_begin_layout")
        else:
            check(self.lib, self.lib.restir_halo_begin(self.ctx, C.byref(camera), C.byref(features), width, height,
                                                       tiles[0], tiles[1], rank, ph, C.byref(sb), C.byref(rb_)),
                  "restir_halo_begin")
        return sb.value, rb_.value

    def halo_pack(self, buf_ptr: int, nbytes: int, host: bool) -> None:
        check(self.lib, self.lib.restir_halo_pack(self.ctx, buf_ptr, nbytes, int(host)), "restir_halo_pack")

    def halo_unpack(self, buf_ptr: int, nbytes: int, host: bool) -> None:
        check(self.lib, self.lib.restir_halo_unpack(self.ctx, buf_ptr, nbytes, int(host)), "restir_halo_unpack")

    def halo_spatial(self) -> None:
        check(self.lib, self.lib.restir_halo_spatial(self.ctx), "restir_halo_spatial")

    def halo_spatial_interior(self) -> None:
        """The current pass's interior (reads no exchanged reservoir): issue it before waiting on the exchange."""
        check(self.lib, self.lib.restir_halo_spatial_interior(self.ctx), "restir_halo_spatial_interior")

    def halo_spatial_border(self) -> None:
        """The current pass's border strips (after the unpack); completes the pass."""
        check(self.lib, self.lib.restir_halo_spatial_border(self.ctx), "restir_halo_spatial_border")

    def halo_attach_rccl(self, unique_id: bytes, nranks: int, rank: int) -> None:
        """Native RCCL halo transport: ncclCommInitRank on this context's device (restir_halo_attach_rccl)."""
        buf = C.create_string_buffer(bytes(unique_id), _abi.RESTIR_RCCL_ID_BYTES)
        check(self.lib, self.lib.restir_halo_attach_rccl(self.ctx, C.cast(buf, C.c_void_p), nranks, rank),
              "restir_halo_attach_rccl")

    def halo_pass(self) -> None:
        """One spatial pass with the exchange over the attached communicator, overlapped with the interior."""
        check(self.lib, self.lib.restir_halo_pass(self.ctx), "restir_halo_pass")

    def halo_record(self, on: bool = True) -> None:
        """restir_halo_record: halo_pass logs the steps it issues instead of calling RCCL (no communicator needed)."""
        check(self.lib, self.lib.restir_halo_record(self.ctx, 1 if on else 0), "restir_halo_record")

    def halo_log(self) -> list:
        """restir_halo_log: the record-only passes' steps in issue order (then cleared), as HaloEvent structs."""
        n = C.c_uint32(0)
        rc = self.lib.restir_halo_log(self.ctx, None, C.byref(n))
        if rc != 0 and n.value == 0:
            check(self.lib, rc, "restir_halo_log")
        buf = (_abi.HaloEvent * max(1, n.value))()
        n2 = C.c_uint32(n.value)
        check(self.lib, self.lib.restir_halo_log(self.ctx, buf, C.byref(n2)), "restir_halo_log")
        return list(buf[:n2.value])

    def halo_end(self, tile, want_rgb: bool = True, want_grid: bool = True):
        out = C.c_void_p()
        rgb = np.zeros((tile.height, tile.width, 3), np.float32) if want_rgb else None
        check(self.lib, self.lib.restir_halo_end(self.ctx, C.byref(out) if want_grid else None,
                                                 rgb.ctypes.data_as(C.POINTER(C.c_float)) if want_rgb else None),
              "restir_halo_end")
        return rgb, (ReservoirGrid(self.lib, out) if want_grid and out.value else None)

    def measure_read_bandwidth(self, nbytes: int = 4 << 30, iters: int = 10) -> float:
        """GB/s of a streaming-read kernel over `nbytes` of HBM (restir_measure_read_bandwidth)."""
        out = C.c_double()
        check(self.lib, self.lib.restir_measure_read_bandwidth(self.ctx, int(nbytes), int(iters), C.byref(out)),
              "restir_measure_read_bandwidth")
        return out.value

    def background_pixels(self) -> tuple[int, int]:
        """(background, computed) pixels of the last render_restir frame (restir_background_pixels): the pixels of its
        RIS tiles flagged all-miss, which the spatial passes and final shading write without reading."""
        bg, px = C.c_uint64(), C.c_uint64()
        check(self.lib, self.lib.restir_background_pixels(self.ctx, C.byref(bg), C.byref(px)), "restir_background_pixels")
        return int(bg.value), int(px.value)

    def gbuf_reuses(self) -> int:
        """render_restir frames so far that read the context's kept G-buffer instead of tracing their primary rays
        (restir_gbuf_reuses; tuning "gbuf.reuse")."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_gbuf_reuses(self.ctx, C.byref(n)), "restir_gbuf_reuses")
        return int(n.value)

    def shadow_list_frames(self) -> int:
        """render_restir frames so far whose fused last pass traced its shadow rays over the view's candidate triangle
        lists (restir_shadow_list_frames; tuning "final.lists")."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_shadow_list_frames(self.ctx, C.byref(n)), "restir_shadow_list_frames")
        return int(n.value)

    def debug_shadow_lists(self, light: int, width: int, height: int):
        """(by the BVH walk, over the list): [height][width] uint8 planes of the last frame's owned rectangle, the shadow
        ray of every pixel to point light `light` (restir_debug_shadow_lists)."""
        a = np.zeros((height, width), np.uint8)
        b = np.zeros((height, width), np.uint8)
        U8 = C.POINTER(C.c_uint8)
        check(self.lib, self.lib.restir_debug_shadow_lists(self.ctx, light, width, height, a.ctypes.data_as(U8),
                                                           b.ctypes.data_as(U8)),
              "restir_debug_shadow_lists")
        return a, b

    def shadow_vis_frames(self) -> int:
        """render_restir frames so far whose fused last pass read its shadow rays' answers from the view's visibility
        bits (restir_shadow_vis_frames; tuning "final.vis")."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_shadow_vis_frames(self.ctx, C.byref(n)), "restir_shadow_vis_frames")
        return int(n.value)

    def shadow_vis_builds(self) -> int:
        """Builds of the visibility bits so far (restir_shadow_vis_builds)."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_shadow_vis_builds(self.ctx, C.byref(n)), "restir_shadow_vis_builds")
        return int(n.value)

    def debug_shadow_vis(self, light: int, width: int, height: int):
        """[height][width] uint8 plane of the last frame's owned rectangle: the stored answer of every pixel's shadow ray to
        point light `light`, 1 / 0, 0xFF where no bit is held (restir_debug_shadow_vis)."""
        a = np.zeros((height, width), np.uint8)
        check(self.lib, self.lib.restir_debug_shadow_vis(self.ctx, light, width, height, a.ctypes.data_as(C.POINTER(C.c_uint8))),
              "restir_debug_shadow_vis")
        return a

    def phat_frames(self) -> int:
        """render_restir frames so far whose RIS read its candidates' target pdfs from the view's p-hat table
        (restir_phat_frames; tuning "ris.phat")."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_phat_frames(self.ctx, C.byref(n)), "restir_phat_frames")
        return int(n.value)

    def phat_builds(self) -> int:
        """Builds of the p-hat table so far (restir_phat_builds)."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_phat_builds(self.ctx, C.byref(n)), "restir_phat_builds")
        return int(n.value)

    def ahead_frames(self) -> int:
        """render_restir frames so far that took their RIS result from the look-ahead the frame before launched
        (restir_ahead_frames; tuning "frames.ahead")."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_ahead_frames(self.ctx, C.byref(n)), "restir_ahead_frames")
        return int(n.value)

    def ahead_discards(self) -> int:
        """Look-ahead results so far that no frame took (restir_ahead_discards)."""
        n = C.c_uint64()
        check(self.lib, self.lib.restir_ahead_discards(self.ctx, C.byref(n)), "restir_ahead_discards")
        return int(n.value)

    def debug_phat(self, light: int, width: int, height: int):
        """[height][width] float32 plane of the last frame's view: the stored target pdf of point light `light` at every
        pixel, -1 where none is held (restir_debug_phat)."""
        a = np.zeros((height, width), np.float32)
        check(self.lib, self.lib.restir_debug_phat(self.ctx, light, width, height, a.ctypes.data_as(C.POINTER(C.c_float))),
              "restir_debug_phat")
        return a

    # ---- timing ---------------------------------------------------------------------------------------
    def enable_timing(self, on: bool = True) -> None:
        check(self.lib, self.lib.restir_enable_timing(self.ctx, 1 if on else 0), "restir_enable_timing")

    def timings(self):
        ms = (C.c_double * _abi.K_COUNT)()
        n = (C.c_uint64 * _abi.K_COUNT)()
        check(self.lib, self.lib.restir_timings(self.ctx, ms, n), "restir_timings")
        return {name: (ms[i], n[i]) for i, name in enumerate(_abi.KERNEL_NAMES)}

    def set_tuning(self, key: str, value: int) -> None:
        check(self.lib, self.lib.restir_set_tuning(self.ctx, key.encode(), int(value)), "restir_set_tuning")

    def reset_timings(self) -> None:
        check(self.lib, self.lib.restir_reset_timings(self.ctx), "restir_reset_timings")

    # ---- stage API (parity tests) ---------------------------------------------------------------------
    def stage_configure(self, width: int, height: int, n: int) -> None:
        check(self.lib, self.lib.restir_stage_configure(self.ctx, width, height, n), "restir_stage_configure")
        self.stage_shape = (width, height, n)

    def _shape(self, which):
        w, h, n = self.stage_shape
        npx = w * h
        return {
            _abi.BUF_GBUF_N_T: (npx, 4), _abi.BUF_GBUF_P_MAT: (npx, 4),
            _abi.BUF_RES_A: (n, npx, 4), _abi.BUF_RES_B: (n, npx, 4), _abi.BUF_RES_DBG: (n, npx, 2),
            _abi.BUF_PREV_A: (n, npx, 4), _abi.BUF_PREV_B: (n, npx, 4), _abi.BUF_PREV_DBG: (n, npx, 2),
            _abi.BUF_RGB: (h, w, 3), _abi.BUF_GBUF_UV: (npx, 2),
        }[which]

    def upload(self, which: int, arr: np.ndarray) -> None:
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(self._shape(which))
        check(self.lib, self.lib.restir_stage_upload(self.ctx, which, a.ctypes.data, a.nbytes), "restir_stage_upload")

    def download(self, which: int) -> np.ndarray:
        a = np.zeros(self._shape(which), np.float32)
        check(self.lib, self.lib.restir_stage_download(self.ctx, which, a.ctypes.data, a.nbytes),
              "restir_stage_download")
        return a

    def stage_primary(self, camera) -> None:
        check(self.lib, self.lib.restir_stage_primary(self.ctx, C.byref(camera)), "restir_stage_primary")

    def stage_ris(self, camera, features, key: int, debug: bool = True) -> None:
        check(self.lib, self.lib.restir_stage_ris(self.ctx, C.byref(camera), C.byref(features), key, int(debug)),
              "restir_stage_ris")

    def stage_temporal(self, camera, features, key: int, debug: bool = True) -> None:
        check(self.lib, self.lib.restir_stage_temporal(self.ctx, C.byref(camera), C.byref(features), key,
                                                       int(debug)), "restir_stage_temporal")

    def stage_spatial(self, camera, features, key: int, debug: bool = True) -> None:
        check(self.lib, self.lib.restir_stage_spatial(self.ctx, C.byref(camera), C.byref(features), key,
                                                      int(debug)), "restir_stage_spatial")

    def stage_final(self, camera, features) -> None:
        check(self.lib, self.lib.restir_stage_final(self.ctx, C.byref(camera), C.byref(features)),
              "restir_stage_final")

    # ---- R-MIS / R-OMIS (render.cpp:64-265) ------------------------------------------------------------
    def render_mis(self, camera, width: int, height: int, features, tile=None) -> np.ndarray:
        """renderRMIS / renderROMIS by features.ray_trace_mode: the screen image (row 0 = top).  No grid is
        returned, as renderRayTraced returns std::nullopt for these modes (render.cpp:274-279).
        tile: a screen tile whose ghost zone is the resample radius (tile_plan(..., ghost=radius)); the result is then
        the tile's owned rectangle [tile.height][tile.width][3], bit for bit the whole image's pixels
        (restir_render_mis_tile)."""
        if tile is None:
            rgb, _ = self.render_restir(None, camera, width, height, features, want_grid=False)
            return rgb
        rgb = np.zeros((tile.height, tile.width, 3), np.float32)
        check(self.lib, self.lib.restir_render_mis_tile(self.ctx, C.byref(camera), C.byref(features), width, height,
                                                        C.byref(tile), rgb.ctypes.data_as(C.POINTER(C.c_float))),
              "restir_render_mis_tile")
        return rgb

    def render_mis_tiled(self, camera, width: int, height: int, features, tiles=(2, 2), layout=None) -> np.ndarray:
        """The whole R-MIS / R-OMIS image rendered tile after tile on this one context, all tiles with one frame index
        (restir_render_mis_tiles): frames whose whole-image buffers would not fit.  tiles: an even (tx, ty) split;
        layout: a restir_tile_layout of the width x height image instead."""
        if layout is None:
            layout = layout_even(width, height, tiles[0], tiles[1])
        elif (layout.global_width, layout.global_height) != (width, height):
            raise ValueError(f"layout is of a {layout.global_width}x{layout.global_height} image, not {width}x{height}")
        rgb = np.zeros((height, width, 3), np.float32)
        check(self.lib, self.lib.restir_render_mis_tiles(self.ctx, C.byref(camera), C.byref(features), C.byref(layout),
                                                         rgb.ctypes.data_as(C.POINTER(C.c_float))),
              "restir_render_mis_tiles")
        return rgb

    def mis_capacity(self, features) -> int:
        cap = C.c_uint32()
        check(self.lib, self.lib.restir_stage_mis_capacity(self.ctx, C.byref(features), C.byref(cap)),
              "restir_stage_mis_capacity")
        return cap.value

    def stage_neighbours(self, features, key_similar: int, key_dissimilar: int) -> None:
        check(self.lib, self.lib.restir_stage_neighbours(self.ctx, C.byref(features), key_similar, key_dissimilar),
              "restir_stage_neighbours")

    def stage_mis_accumulate(self, camera, features, iteration: int) -> None:
        check(self.lib, self.lib.restir_stage_mis_accumulate(self.ctx, C.byref(camera), C.byref(features), iteration),
              "restir_stage_mis_accumulate")

    def stage_mis_finish(self, features) -> None:
        check(self.lib, self.lib.restir_stage_mis_finish(self.ctx, C.byref(features)), "restir_stage_mis_finish")

    def mis_buffers(self, features, nbr: np.ndarray | None = None, acc: np.ndarray | None = None):
        """Upload (when given) and download the MIS_NBR (uint32 [1 + cap][pixels]) and MIS_ACC (float
        [rows][pixels]) stage buffers."""
        w, h, _ = self.stage_shape
        cap = self.mis_capacity(features)
        T = features.num_neighbours_to_sample + 1
        rows = T * T + 6 * T + 3 if features.ray_trace_mode == _abi.MODE_ROMIS else 3
        for which, arr, dt, shape in [(_abi.BUF_MIS_NBR, nbr, np.uint32, (1 + cap, w * h)),
                                      (_abi.BUF_MIS_ACC, acc, np.float32, (rows, w * h))]:
            if arr is not None:
                a = np.ascontiguousarray(arr, dtype=dt).reshape(shape)
                check(self.lib, self.lib.restir_stage_upload(self.ctx, which, a.ctypes.data, a.nbytes),
                      "restir_stage_upload")
        out = []
        for which, dt, shape in [(_abi.BUF_MIS_NBR, np.uint32, (1 + cap, w * h)),
                                 (_abi.BUF_MIS_ACC, np.float32, (rows, w * h))]:
            a = np.zeros(shape, dt)
            check(self.lib, self.lib.restir_stage_download(self.ctx, which, a.ctypes.data, a.nbytes),
                  "restir_stage_download")
            out.append(a)
        return tuple(out)

    def debug_cod_solve(self, A: np.ndarray, b: np.ndarray) -> np.ndarray:
        """Batched least squares (A [count][n][n] row-major numpy, b [count][n]) with the device routine of the
        R-OMIS finish (Eigen CompleteOrthogonalDecomposition::solve, render_utils.h:52)."""
        A = np.asarray(A, np.float32)
        count, n, _ = A.shape
        Ac = np.ascontiguousarray(np.transpose(A, (0, 2, 1)), np.float32)   # column-major per system
        bc = np.ascontiguousarray(b, np.float32).reshape(count, n)
        x = np.zeros((count, n), np.float32)
        FP = C.POINTER(C.c_float)
        check(self.lib, self.lib.restir_debug_cod_solve(self.ctx, n, Ac.ctypes.data_as(FP), bc.ctypes.data_as(FP),
                                                        x.ctypes.data_as(FP), count), "restir_debug_cod_solve")
        return x

    def debug_math(self, x: np.ndarray, y: np.ndarray):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        pw = np.zeros_like(x)
        ex = np.zeros_like(x)
        FP = C.POINTER(C.c_float)
        check(self.lib, self.lib.restir_debug_math(self.ctx, x.ctypes.data_as(FP), y.ctypes.data_as(FP),
                                                   pw.ctypes.data_as(FP), ex.ctypes.data_as(FP), x.size),
              "restir_debug_math")
        return pw, ex


def rng_key(seed: int, frame: int, stage: int, pass_: int = 0) -> int:
    return _abi.load_library().restir_rng_key(seed, frame, stage, pass_)


def accum_fold(mean: np.ndarray, m2: np.ndarray | None, x, n: int) -> None:
    """restir_accum_fold (pure host): fold x into mean (and m2) IN PLACE as the n-th value -- contiguous float32 arrays of
    one size; the device's own arithmetic, bit for bit."""
    lib = _abi.load_library()
    xa = np.ascontiguousarray(x, np.float32)
    for a in (mean, m2):
        if a is not None and (a.dtype != np.float32 or not a.flags.c_contiguous or a.size != xa.size):
            raise ValueError("accum_fold: mean and m2 must be contiguous float32 arrays of x's size")
    FP = C.POINTER(C.c_float)
    check(lib, lib.restir_accum_fold(mean.ctypes.data_as(FP), m2.ctypes.data_as(FP) if m2 is not None else None,
                                     xa.ctypes.data_as(FP), xa.size, n), "restir_accum_fold")


def error_measure(a, r) -> _abi.ErrorStats:
    """restir_error_measure (pure host): the error figures of array a against the reference r -- float32 arrays of one
    size -- by the device reduction's own arithmetic and order, bit for bit (width, height, source and frames are 0)."""
    lib = _abi.load_library()
    aa, ra = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(r, np.float32)
    if aa.size != ra.size:
        raise ValueError("error_measure: a and r must have one size")
    FP = C.POINTER(C.c_float)
    s = _abi.ErrorStats()
    check(lib, lib.restir_error_measure(aa.ctypes.data_as(FP), ra.ctypes.data_as(FP), aa.size, C.byref(s)),
          "restir_error_measure")
    return s


def denoise_params(iterations: int | None = None, normal_power_log2: int | None = None,
                   sigma_plane: float | None = None) -> _abi.DenoiseParams:
    """restir_denoise_params_default, with the given fields replaced."""
    lib = _abi.load_library()
    p = _abi.DenoiseParams()
    lib.restir_denoise_params_default(C.byref(p))
    if iterations is not None:
        p.iterations = iterations
    if normal_power_log2 is not None:
        p.normal_power_log2 = normal_power_log2
    if sigma_plane is not None:
        p.sigma_plane = sigma_plane
    return p


def denoise_lum_params(iterations: int | None = None, normal_power_log2: int | None = None, sigma_plane: float | None = None,
                       variance_source: int | None = None, sigma_lum: float | None = None) -> _abi.DenoiseLumParams:
    """restir_denoise_lum_params_default, with the given fields replaced."""
    lib = _abi.load_library()
    p = _abi.DenoiseLumParams()
    lib.restir_denoise_lum_params_default(C.byref(p))
    if iterations is not None:
        p.geo.iterations = iterations
    if normal_power_log2 is not None:
        p.geo.normal_power_log2 = normal_power_log2
    if sigma_plane is not None:
        p.geo.sigma_plane = sigma_plane
    if variance_source is not None:
        p.variance_source = variance_source
    if sigma_lum is not None:
        p.sigma_lum = sigma_lum
    return p


def denoise_lum_host(rgb, n_t, p_mat, miss_material: int, params=None, var=None):
    """restir_denoise_lum_host (pure host): Renderer.denoise_lum's arithmetic, bit for bit, without the tone-mapping step.
    rgb, n_t, p_mat, miss_material as denoise_host's; var [h][w] (row 0 = top): the initial variance plane, None: the
    spatial estimate.  Returns (the filtered rgb [h][w][3], the last level's variance plane [h][w])."""
    lib = _abi.load_library()
    c = np.ascontiguousarray(rgb, np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("denoise_lum_host: rgb must be [h][w][3]")
    h, w = c.shape[:2]
    nt, pm = np.ascontiguousarray(n_t, np.float32), np.ascontiguousarray(p_mat, np.float32)
    if nt.size != 4 * w * h or pm.size != 4 * w * h:
        raise ValueError("denoise_lum_host: n_t and p_mat must hold 4 floats per pixel of rgb")
    FP = C.POINTER(C.c_float)
    v = None
    if var is not None:
        v = np.ascontiguousarray(var, np.float32)
        if v.size != w * h:
            raise ValueError("denoise_lum_host: var must hold one float per pixel of rgb")
    if params is None:
        params = denoise_lum_params()
    out, out_var = np.zeros_like(c), np.zeros((h, w), np.float32)
    check(lib, lib.restir_denoise_lum_host(c.ctypes.data_as(FP), v.ctypes.data_as(FP) if v is not None else None,
                                           nt.ctypes.data_as(FP), pm.ctypes.data_as(FP), w, h, miss_material, C.byref(params),
                                           out.ctypes.data_as(FP), out_var.ctypes.data_as(FP)), "restir_denoise_lum_host")
    return out, out_var


def denoise_host(rgb, n_t, p_mat, miss_material: int, params=None) -> np.ndarray:
    """restir_denoise_host (pure host): Renderer.denoise's arithmetic, bit for bit, without the tone-mapping step.  rgb
    [h][w][3] (row 0 = top); n_t, p_mat [h][w][4] or [h * w][4] as stage_primary gives them (row y = 0 at the bottom,
    p_mat's w the material's bits); miss_material: the scene's num_materials - 1.  Returns the filtered [h][w][3]."""
    lib = _abi.load_library()
    c = np.ascontiguousarray(rgb, np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("denoise_host: rgb must be [h][w][3]")
    h, w = c.shape[:2]
    nt, pm = np.ascontiguousarray(n_t, np.float32), np.ascontiguousarray(p_mat, np.float32)
    if nt.size != 4 * w * h or pm.size != 4 * w * h:
        raise ValueError("denoise_host: n_t and p_mat must hold 4 floats per pixel of rgb")
    if params is None:
        params = denoise_params()
    out = np.zeros_like(c)
    FP = C.POINTER(C.c_float)
    check(lib, lib.restir_denoise_host(c.ctypes.data_as(FP), nt.ctypes.data_as(FP), pm.ctypes.data_as(FP), w, h,
                                       miss_material, C.byref(params), out.ctypes.data_as(FP)), "restir_denoise_host")
    return out


# restir_history_gather: Renderer.history_gather's modes
HISTORY_GATHER_NEAREST = _abi.RESTIR_HISTORY_GATHER_NEAREST
HISTORY_GATHER_BILINEAR = _abi.RESTIR_HISTORY_GATHER_BILINEAR


def history_params(max_frames: int | None = None, spatial_below: int | None = None) -> _abi.HistoryParams:
    """restir_history_params_default, with the given fields replaced."""
    lib = _abi.load_library()
    p = _abi.HistoryParams()
    lib.restir_history_params_default(C.byref(p))
    if max_frames is not None:
        p.max_frames = max_frames
    if spatial_below is not None:
        p.spatial_below = spatial_below
    return p


def history_fold(mean, S, n, smap, x, max_frames: int):
    """restir_history_fold (pure host): one advance's gather and fold, bit for bit.  mean, S [h][w][3] float32 and n [h][w]
    uint32 (image rows): the kept state; smap [h][w] uint32 (rows y = 0 bottom): history_advance's map; x [h][w][3]: the
    image.  Returns the new (mean, S, n)."""
    lib = _abi.load_library()
    xa = np.ascontiguousarray(x, np.float32)
    if xa.ndim != 3 or xa.shape[2] != 3:
        raise ValueError("history_fold: x must be [h][w][3]")
    h, w = xa.shape[:2]
    m, s = np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(S, np.float32)
    na, ma = np.ascontiguousarray(n, np.uint32), np.ascontiguousarray(smap, np.uint32)
    if m.size != xa.size or s.size != xa.size or na.size != w * h or ma.size != w * h:
        raise ValueError("history_fold: mean, S, n and the map must have x's size")
    mo, so, no = np.zeros_like(xa), np.zeros_like(xa), np.zeros((h, w), np.uint32)
    FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    check(lib, lib.restir_history_fold(m.ctypes.data_as(FP), s.ctypes.data_as(FP), na.ctypes.data_as(UP), ma.ctypes.data_as(UP),
                                       xa.ctypes.data_as(FP), w, h, max_frames, mo.ctypes.data_as(FP), so.ctypes.data_as(FP),
                                       no.ctypes.data_as(UP)), "restir_history_fold")
    return mo, so, no


def history_map_host(prev_cam: _abi.CameraFrame, width: int, height: int, cur_gbuffer, kept, miss_material: int) -> np.ndarray:
    """restir_history_map_host (pure host): history_advance's map [h][w] uint32 (rows y = 0 bottom).  cur_gbuffer: (n_t,
    p_mat) of the new camera, 4 floats per pixel, rows y = 0 bottom; kept: (n_t, material, n) the history kept from the
    advance before -- n_t and the material's words in G-buffer rows, n [h][w] in image rows --, or None: nothing kept."""
    lib = _abi.load_library()
    FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    cn, cp = (np.ascontiguousarray(a, np.float32) for a in cur_gbuffer)
    px = width * height
    if cn.size != 4 * px or cp.size != 4 * px:
        raise ValueError("history_map_host: the G-buffer must hold 4 floats per pixel")
    kn = km = kc = None
    if kept is not None:
        kn, km, kc = np.ascontiguousarray(kept[0], np.float32), np.ascontiguousarray(kept[1], np.uint32), \
            np.ascontiguousarray(kept[2], np.uint32)
        if kn.size != 4 * px or km.size != px or kc.size != px:
            raise ValueError("history_map_host: kept must be (n_t, material, n) of the image's size")
    out = np.zeros((height, width), np.uint32)
    check(lib, lib.restir_history_map_host(C.byref(prev_cam), width, height, cn.ctypes.data_as(FP), cp.ctypes.data_as(FP),
                                           kn.ctypes.data_as(FP) if kept is not None else None,
                                           km.ctypes.data_as(UP) if kept is not None else None,
                                           kc.ctypes.data_as(UP) if kept is not None else None, miss_material,
                                           out.ctypes.data_as(UP)), "restir_history_map_host")
    return out


def history_advance_host(prev_cam: _abi.CameraFrame, cur_gbuffer, kept, mean, S, n, x, miss_material: int, max_frames: int,
                         gather: int = _abi.RESTIR_HISTORY_GATHER_NEAREST):
    """restir_history_advance_host (pure host): one whole history_advance in either gather mode, bit for bit.  prev_cam: the
    derived CameraFrame of the advance before; cur_gbuffer: (n_t, p_mat) of the new camera and kept: (n_t, material) the
    history kept from the advance before, or None: nothing kept -- all in rows y = 0 bottom; mean, S [h][w][3] float32
    and n [h][w] uint32 (image rows): the kept state; x [h][w][3]: the image.  Returns (mean, S, n, map): the new state and
    the map [h][w] uint32 (rows y = 0 bottom)."""
    lib = _abi.load_library()
    FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    xa = np.ascontiguousarray(x, np.float32)
    if xa.ndim != 3 or xa.shape[2] != 3:
        raise ValueError("history_advance_host: x must be [h][w][3]")
    h, w = xa.shape[:2]
    px = w * h
    cn, cp = (np.ascontiguousarray(a, np.float32) for a in cur_gbuffer)
    if cn.size != 4 * px or cp.size != 4 * px:
        raise ValueError("history_advance_host: the G-buffer must hold 4 floats per pixel")
    kn = km = None
    if kept is not None:
        kn, km = np.ascontiguousarray(kept[0], np.float32), np.ascontiguousarray(kept[1], np.uint32)
        if kn.size != 4 * px or km.size != px:
            raise ValueError("history_advance_host: kept must be (n_t, material) of the image's size")
    m, s, na = np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(S, np.float32), np.ascontiguousarray(n, np.uint32)
    if m.size != xa.size or s.size != xa.size or na.size != px:
        raise ValueError("history_advance_host: mean, S and n must have x's size")
    mo, so, no, smap = np.zeros_like(xa), np.zeros_like(xa), np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)
    check(lib, lib.restir_history_advance_host(
        C.byref(prev_cam), w, h, cn.ctypes.data_as(FP), cp.ctypes.data_as(FP),
        kn.ctypes.data_as(FP) if kept is not None else None, km.ctypes.data_as(UP) if kept is not None else None,
        m.ctypes.data_as(FP), s.ctypes.data_as(FP), na.ctypes.data_as(UP), xa.ctypes.data_as(FP), miss_material, max_frames,
        int(gather), mo.ctypes.data_as(FP), so.ctypes.data_as(FP), no.ctypes.data_as(UP), smap.ctypes.data_as(UP)),
        "restir_history_advance_host")
    return mo, so, no, smap


def history_variance_host(mean, S, n, n_t, p_mat, miss_material: int, params=None, geo=None) -> np.ndarray:
    """restir_history_variance_host (pure host): history_denoise's initial variance plane [h][w] (row 0 = top), bit for
    bit.  mean, S, n as history_state gives them; n_t, p_mat as denoise_host's; params: a HistoryParams, geo: a
    DenoiseParams (None: the defaults)."""
    lib = _abi.load_library()
    m = np.ascontiguousarray(mean, np.float32)
    if m.ndim != 3 or m.shape[2] != 3:
        raise ValueError("history_variance_host: mean must be [h][w][3]")
    h, w = m.shape[:2]
    s, na = np.ascontiguousarray(S, np.float32), np.ascontiguousarray(n, np.uint32)
    nt, pm = np.ascontiguousarray(n_t, np.float32), np.ascontiguousarray(p_mat, np.float32)
    if s.size != m.size or na.size != w * h or nt.size != 4 * w * h or pm.size != 4 * w * h:
        raise ValueError("history_variance_host: S, n, n_t and p_mat must have mean's size")
    if params is None:
        params = history_params()
    if geo is None:
        geo = denoise_params()
    var = np.zeros((h, w), np.float32)
    FP = C.POINTER(C.c_float)
    check(lib, lib.restir_history_variance_host(m.ctypes.data_as(FP), s.ctypes.data_as(FP), na.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                nt.ctypes.data_as(FP), pm.ctypes.data_as(FP), w, h, miss_material,
                                                C.byref(params), C.byref(geo), var.ctypes.data_as(FP)),
          "restir_history_variance_host")
    return var


def reproject_pixel(prev_cam: _abi.CameraFrame, width: int, height: int, point):
    """restir_reproject_pixel (pure host): (x, y, depth) -- the pixel of the width x height image where the camera
    prev_cam (a derived CameraFrame) saw world point `point`, x = y = 0xFFFFFFFF - reason when behind (1) or off-screen
    (2), and the point's distance from the camera."""
    lib = _abi.load_library()
    P = (C.c_float * 3)(*[float(v) for v in point])
    x, y, d = C.c_uint32(), C.c_uint32(), C.c_float()
    check(lib, lib.restir_reproject_pixel(C.byref(prev_cam), width, height, P, C.byref(x), C.byref(y), C.byref(d)),
          "restir_reproject_pixel")
    return x.value, y.value, d.value


def rccl_unique_id() -> bytes:
    """restir_rccl_unique_id: the RESTIR_RCCL_ID_BYTES bytes one rank hands to all (ncclGetUniqueId)."""
    lib = _abi.load_library()
    buf = C.create_string_buffer(_abi.RESTIR_RCCL_ID_BYTES)
    check(lib, lib.restir_rccl_unique_id(C.cast(buf, C.c_void_p), _abi.RESTIR_RCCL_ID_BYTES), "restir_rccl_unique_id")
    return buf.raw


def halo_plan(width: int, height: int, tiles_x: int, tiles_y: int, rank: int, radius: int, N: int, layout=None):
    """restir_halo_plan: ([send segments], [recv segments]) for `rank`, one pair per adjacent rank (layout: an
    uneven restir_tile_layout instead of the even tiles_x x tiles_y split)."""
    lib = _abi.load_library()
    send = (_abi.HaloSegment * 8)()
    recv = (_abi.HaloSegment * 8)()
    n = C.c_uint32(8)
    if layout is not None:
        check(lib, lib.restir_layout_halo_plan(C.byref(layout), rank, radius, N, send, recv, C.byref(n)),
              "restir_layout_halo_plan")
    else:
        check(lib, lib.restir_halo_plan(width, height, tiles_x, tiles_y, rank, radius, N, send, recv, C.byref(n)),
              "restir_halo_plan")
    return list(send[:n.value]), list(recv[:n.value])


def halo_ops(width: int, height: int, tiles_x: int, tiles_y: int, rank: int, radius: int, N: int, layout=None) -> list:
    """restir_halo_ops: the sends / receives restir_halo_pass posts per spatial pass, in posting order."""
    lib = _abi.load_library()
    ops = (_abi.HaloOp * 16)()
    n = C.c_uint32(16)
    if layout is not None:
        check(lib, lib.restir_layout_halo_ops(C.byref(layout), rank, radius, N, ops, C.byref(n)), "restir_layout_halo_ops")
    else:
        check(lib, lib.restir_halo_ops(width, height, tiles_x, tiles_y, rank, radius, N, ops, C.byref(n)),
              "restir_halo_ops")
    return list(ops[:n.value])


def tile_plan(width: int, height: int, tiles_x: int, tiles_y: int, rank: int, ghost: int, layout=None) -> _abi.Tile:
    lib = _abi.load_library()
    t = _abi.Tile()
    if layout is not None:
        check(lib, lib.restir_layout_tile(C.byref(layout), rank, ghost, C.byref(t)), "restir_layout_tile")
    else:
        check(lib, lib.restir_tile_plan(width, height, tiles_x, tiles_y, rank, ghost, C.byref(t)), "restir_tile_plan")
    return t


def layout_even(width: int, height: int, tiles_x: int, tiles_y: int) -> _abi.TileLayout:
    """restir_layout_even: restir_tile_plan's even split as a layout."""
    lib = _abi.load_library()
    L = _abi.TileLayout()
    check(lib, lib.restir_layout_even(width, height, tiles_x, tiles_y, C.byref(L)), "restir_layout_even")
    return L


def _cost_arg(cost):
    c = np.ascontiguousarray(cost, dtype=np.float32)
    if c.ndim != 2:
        raise ValueError("cost grid must be 2-D [rows (row 0 = bottom)][columns]")
    return c, c.ctypes.data_as(C.POINTER(C.c_float))


def layout_balanced(width: int, height: int, tiles_x: int, tiles_y: int, cost, align=(32, 8)):
    """restir_layout_balanced: (layout, implied efficiency) balancing the cost grid [rows][cols] (row 0 = bottom)."""
    lib = _abi.load_library()
    c, ptr = _cost_arg(cost)
    L = _abi.TileLayout()
    eff = C.c_double()
    check(lib, lib.restir_layout_balanced(width, height, tiles_x, tiles_y, ptr, c.shape[1], c.shape[0], align[0], align[1],
                                          C.byref(L), C.byref(eff)), "restir_layout_balanced")
    return L, eff.value


def layout_shares(layout, cost) -> np.ndarray:
    """restir_layout_shares: each rank's share of the cost grid under `layout` (sums to 1)."""
    lib = _abi.load_library()
    c, ptr = _cost_arg(cost)
    out = np.zeros(layout.tiles_x * layout.tiles_y, np.float64)
    check(lib, lib.restir_layout_shares(C.byref(layout), ptr, c.shape[1], c.shape[0],
                                        out.ctypes.data_as(C.POINTER(C.c_double))), "restir_layout_shares")
    return out


def tile_grid(n: int) -> tuple:
    """Screen tiling for n ranks: 1x1, 2x1, 2x2, 4x2 (tiles_x, tiles_y)."""
    return {1: (1, 1), 2: (2, 1), 4: (2, 2), 8: (4, 2)}.get(n) or (n, 1)
