"""The specification of restir_render_exact, built on the CPU from the oracle's existing passes (nothing under oracle/
knows the feature): the G-buffer of pyoracle.gbuffer, then one pyoracle.final per light with N = 1, tone mapping off and
every pixel's reservoir set to (position of light i, colour of light i, W = 1, M = 1), float32-summed in light order from
+0, and or_tonemap where tone mapping is on.  `0 + sc * 1`, `/ 1` and the running sum never produce -0, so the sum's
bits are the kernel's.  Also the census every ray test starts from: the (pixel, light) pairs with a positive target pdf
that are visible, and those that are occluded.  Helpers of tests/test_gpu_exact.py; no test lives here."""
import ctypes as C

import numpy as np

from romis_amd import _abi

F32 = np.float32
FP = C.POINTER(C.c_float)


def origin_of(oracle, cam):
    return np.asarray(list(oracle.camera_frame(cam).origin), F32)


def point_lights(sc):
    """(positions [L][3], colours [L][3]) of a scene whose lights are all point lights"""
    assert all(l.type == _abi.LIGHT_POINT for l in sc.lights)
    pos = np.array([list(l.p0) for l in sc.lights], F32).reshape(-1, 3)
    col = np.array([list(l.c0) for l in sc.lights], F32).reshape(-1, 3)
    return pos, col


def shading_features(f):
    """N = 1, tone mapping off, f's shading and texture fields: one light's run of final shading"""
    return _abi.default_features(num_samples_in_reservoir=1, enable_tone_mapping=0, enable_shading=f.enable_shading,
                                 enable_texture_mapping=f.enable_texture_mapping)


def tonemap(oracle, img, exposure, gamma):
    lib = oracle.lib()
    src = np.ascontiguousarray(img, F32).reshape(-1, 3)
    out = np.zeros_like(src)
    for i in range(len(src)):
        lib.or_tonemap(src[i].ctypes.data_as(FP), exposure, gamma, out[i].ctypes.data_as(FP))
    return out.reshape(np.shape(img))


def exact_image(oracle, osc, sc, cam, w, h, f, view=None):
    """rgb [h][w][3] (row 0 = top) of the whole image, or of the rectangle `view` (an oracle Rect) of it"""
    view = view or oracle.full_rect(w, h)
    n_t, p_mat = oracle.gbuffer(osc, cam, w, h, view)
    npx = view.w * view.h
    pos, col = point_lights(sc)
    f1, o = shading_features(f), origin_of(oracle, cam)
    one = np.array([1], np.uint32).view(F32)[0]
    color = np.zeros((view.h, view.w, 3), F32)
    for i in range(len(pos)):
        a = np.empty((1, npx, 4), F32)
        b = np.empty((1, npx, 4), F32)
        a[0, :, :3], a[0, :, 3] = pos[i], F32(1.0)
        b[0, :, :3], b[0, :, 3] = col[i], one
        color = color + oracle.final(osc, f1, o, w, h, n_t, p_mat, (a, b), view=view)   # float32, in light order
        assert color.dtype == F32
    if f.enable_tone_mapping:
        color = tonemap(oracle, color, f.exposure, f.gamma)
    return color


def pair_census(oracle, osc, sc, cam, w, h):
    """(visible, occluded): the (pixel, light) pairs of the frame whose target pdf is positive, by the answer of the
    shadow ray (or_target_pdf with shading on, pyoracle.visible)"""
    n_t, p_mat = oracle.gbuffer(osc, cam, w, h)
    pos, col = point_lights(sc)
    f, o = _abi.default_features(), origin_of(oracle, cam)
    lib = oracle.lib()
    fr, op = C.byref(f), o.ctypes.data_as(FP)
    nt_p = [n_t[p].ctypes.data_as(FP) for p in range(len(n_t))]
    pm_p = [p_mat[p].ctypes.data_as(FP) for p in range(len(n_t))]
    vis_n = occ_n = 0
    for i in range(len(pos)):
        lp, lc = pos[i].ctypes.data_as(FP), col[i].ctypes.data_as(FP)
        lit = np.array([lib.or_target_pdf(osc.handle, fr, op, nt_p[p], pm_p[p], lp, lc) > 0.0 for p in range(len(n_t))])
        if not lit.any():
            continue
        P = np.ascontiguousarray(p_mat[lit, :3])
        v = oracle.visible(osc, P, np.tile(pos[i], (len(P), 1)))
        vis_n += int(v.sum())
        occ_n += int((~v).sum())
    return vis_n, occ_n
