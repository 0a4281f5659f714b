"""The specification of the image history (include/restir_c.h "a reprojected image history") in numpy: one advance's map,
gather and fold, and restir_history_denoise's initial variance plane.  Every numpy step is one float32 operation, divide and
sqrt correctly rounded, nothing contracted, in csrc/history.h's order.  The map extends tests/test_reproject_host.py's
np_map by reasons 6 and 7; the variance plane is denoise_lum_spec's spatial estimate with the history's own entries over
it.  Helpers of tests/test_history_host.py and tests/test_gpu_history.py; no test lives here.

Rows: G-buffer records and the map are in G-buffer rows (y = 0 bottom), images and state in image rows (row 0 = top)."""
import numpy as np

import denoise_lum_spec as lspec
import denoise_spec as dspec
from test_reproject_host import DEPTH, MISS, NONE, NORMAL, PREV_MISS, np_source

F32, U32 = np.float32, np.uint32
MATERIAL, NO_HISTORY = 6, 7
REASONS = ("miss", "behind", "off-screen", "predecessor miss", "depth", "normal", "material", "no history")


def material(p_mat, miss_material):
    """the clamped material words of a G-buffer's p_mat [px][4]"""
    return np.minimum(np.ascontiguousarray(p_mat[:, 3]).view(U32), U32(miss_material))


def flip(a, w, h):
    """a plane of w x h pixels between image rows and G-buffer rows (its own inverse), as [h][w]..."""
    a = np.asarray(a)
    k = a.size // (w * h)
    return np.ascontiguousarray(a.reshape((h, w) if k == 1 else (h, w, k))[::-1])


def np_map(cf_prev, w, h, gb_cur, kept, miss_material):
    """restir_history_advance's map [h * w] (G-buffer rows).  gb_cur = (n_t, p_mat) [px][4] of the new camera; kept =
    (n_t [px][4], material [px] uint32, both G-buffer rows, n [h][w] uint32 image rows), or None: nothing kept."""
    cn, cp = gb_cur
    px = w * h
    if kept is None:
        return np.full(px, NONE - NO_HISTORY, U32)
    kn, kmat, kcount = kept
    kmat = np.minimum(np.asarray(kmat, U32).reshape(-1), U32(miss_material))
    kcount = flip(np.asarray(kcount, U32).reshape(h, w), w, h).reshape(-1)   # -> G-buffer rows
    cmat = material(cp, miss_material)
    x, y, d, why = np_source(cf_prev, w, h, cp[:, :3])
    q = y.astype(np.int64) * w + x
    with np.errstate(all="ignore"):
        depth = np.abs(F32(1.0) - kn[q, 3] / d) > F32(0.1)
        dot = (kn[q, 0] * cn[:, 0] + kn[q, 1] * cn[:, 1]) + kn[q, 2] * cn[:, 2]
        normal = dot < F32(0.90630778703)
    after = np.where(kmat[q] == miss_material, PREV_MISS,
                     np.where(depth, DEPTH, np.where(normal, NORMAL,
                                                     np.where(kmat[q] != cmat, MATERIAL,
                                                              np.where(kcount[q] == 0, NO_HISTORY, NONE)))))
    why = np.where(why != NONE, why, after)
    why = np.where(cmat == miss_material, MISS, why).astype(np.int64)
    return np.where(why == NONE, q, NONE - why).astype(U32)


def classes(m):
    """{class: pixels} of a map: every reason, "valid" and "moved" (valid at another pixel)"""
    m = np.asarray(m).reshape(-1)
    out = {name: int(np.count_nonzero(m == NONE - k)) for k, name in enumerate(REASONS)}
    valid = m <= NONE - len(REASONS)
    out["valid"] = int(valid.sum())
    out["moved"] = int(np.count_nonzero(valid & (m != np.arange(m.size))))
    return out


def fold(mean, S, n, smap, x, max_frames):
    """One advance: the kept state (mean, S [h][w][3], n [h][w], image rows) gathered by the map (G-buffer rows) and
    folded with the image x [h][w][3].  Returns the new (mean, S, n)."""
    x = np.ascontiguousarray(x, F32)
    h, w = x.shape[:2]
    m = flip(np.asarray(smap, U32).reshape(h, w), w, h).reshape(-1)            # the map entry of each image pixel
    ok = m <= NONE - len(REASONS)
    src = np.where(ok, m, 0).astype(np.int64)
    qi = (h - 1 - src // w) * w + src % w                                      # the source's image-row index
    gm = np.where(ok[:, None], np.ascontiguousarray(mean, F32).reshape(-1, 3).view(U32)[qi], U32(0)).view(F32)
    gs = np.where(ok[:, None], np.ascontiguousarray(S, F32).reshape(-1, 3).view(U32)[qi], U32(0)).view(F32)
    gn = np.where(ok, np.asarray(n, U32).reshape(-1)[qi], U32(0)).astype(U32)
    xs = x.reshape(-1, 3)
    fin = np.isfinite(xs).all(axis=1)
    n1 = np.where(gn < U32(max_frames), gn + U32(1), U32(max_frames)).astype(U32)
    with np.errstate(all="ignore"):
        a = (F32(1.0) / n1.astype(F32))[:, None]
        om = F32(1.0) - a
        d = xs - gm
        mean1 = gm + d * a
        dd = d * d
        t = a * dd
        u = gs + t
        S1 = om * u
    assert mean1.dtype == F32 and S1.dtype == F32
    empty = (gn == 0)
    # an x that is not finite: the gathered state passes through; an empty one shows x's bits
    pm = np.where(empty[:, None], xs.view(U32), gm.view(U32)).view(F32)
    ps = np.where(empty[:, None], U32(0), gs.view(U32)).view(F32)
    mean_o = np.where(fin[:, None], mean1.view(U32), pm.view(U32)).view(F32)
    S_o = np.where(fin[:, None], S1.view(U32), ps.view(U32)).view(F32)
    n_o = np.where(fin, n1, gn).astype(U32)
    return mean_o.reshape(h, w, 3), S_o.reshape(h, w, 3), n_o.reshape(h, w)


def variance(mean, S, n, n_t, p_mat, miss_material, spatial_below, normal_power_log2, sigma_plane):
    """restir_history_denoise's initial variance plane [h][w] (image rows)"""
    mean = np.ascontiguousarray(mean, F32)
    h, w = mean.shape[:2]
    G = dspec.guides(n_t, p_mat, w, h, miss_material)
    v = lspec.var_spatial(mean, G, normal_power_log2, sigma_plane)
    n = np.asarray(n, U32).reshape(h, w)
    temporal = (n >= spatial_below) & np.isfinite(mean).all(axis=-1)
    with np.errstate(all="ignore"):
        inv = (F32(1.0) / (np.maximum(n, 2) - U32(1)).astype(F32))[..., None]
        s = np.sqrt(np.ascontiguousarray(S, F32) * inv)
        sl = lspec.lum(s)
        vt = lspec.clean(sl * sl)
    assert vt.dtype == F32
    return np.where(temporal, vt, v).astype(F32)
