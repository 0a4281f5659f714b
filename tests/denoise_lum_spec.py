"""The specification of restir_denoise_lum / restir_denoise_lum_host in numpy (include/restir_c.h "denoising with a
variance-guided luminance term"), over denoise_spec's guides: every numpy step is one float32 operation, divide and sqrt
correctly rounded, nothing contracted, over whole shifted planes instead of per pixel, the taps in the contract's order
(dy outside, dx inside).  Helpers of tests/test_denoise_lum_host.py and tests/test_gpu_denoise_lum.py; no test lives here."""
import numpy as np

import denoise_spec as spec
from denoise_spec import F32, K, U32

G3 = [F32(0.25), F32(0.5), F32(0.25)]


def lum(c):
    """l(c) = (0.2126 r + 0.7152 g) + 0.0722 b"""
    out = (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]
    assert out.dtype == F32
    return out


def clean(v):
    """a variance as the initial plane stores it: not finite, or not > 0 -> +0"""
    v = np.ascontiguousarray(v, F32)
    with np.errstate(all="ignore"):
        return np.where((v > 0) & np.isfinite(v), v, F32(0)).astype(F32)


def window(h, w, oy, ox):
    """(p, q) slices of the centres whose tap at offset (ox, oy) lies inside an h x w image, None when there is none"""
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def geo_weight(G, p, q, hk, inv_s, normal_power_log2):
    """restir_denoise's weight of the taps q for the centres p, other than the centre itself: 0 where its material or
    flat rule skips the tap"""
    g, P, mat, flat, _ = G
    cn = (g[p][..., 0] * g[q][..., 0] + g[p][..., 1] * g[q][..., 1]) + g[p][..., 2] * g[q][..., 2]
    cn = np.where(cn > 0, cn, F32(0))
    for _ in range(normal_power_log2):
        cn = cn * cn
    d = P[q] - P[p]
    e = (g[p][..., 0] * d[..., 0] + g[p][..., 1] * d[..., 1]) + g[p][..., 2] * d[..., 2]
    r = e * inv_s[p]
    wp = F32(1.0) - r * r
    wn = hk * (cn * wp)
    both, neither = flat[p] & flat[q], ~flat[p] & ~flat[q]
    wt = np.where(both, hk, np.where(neither, wn, F32(0))).astype(F32)
    return np.where(mat[q] == mat[p], wt, F32(0)).astype(F32)


def var_spatial(c, G, normal_power_log2, sigma_plane):
    """RESTIR_DENOISE_VAR_SPATIAL's plane [h][w] of the image c [h][w][3]"""
    t = G[4]
    h, w = c.shape[:2]
    fin = np.isfinite(c).all(axis=-1)
    s0, s1, s2 = (np.zeros((h, w), F32) for _ in range(3))
    with np.errstate(all="ignore"):
        l = lum(c)
        inv_s = F32(1.0) / (F32(sigma_plane) * t)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                pq = window(h, w, dy, dx)
                if pq is None:
                    continue
                p, q = pq
                ok = fin[q].copy()
                if dx == 0 and dy == 0:
                    wt = np.full(ok.shape, F32(1.0), F32)
                else:
                    wt = geo_weight(G, p, q, F32(1.0), inv_s, normal_power_log2)
                ok &= wt > 0
                lq = l[q]
                s0[p] = np.where(ok, s0[p] + wt, s0[p])
                s1[p] = np.where(ok, s1[p] + wt * lq, s1[p])
                s2[p] = np.where(ok, s2[p] + wt * (lq * lq), s2[p])
        m1 = s1 / s0
        v = s2 / s0 - m1 * m1
    assert v.dtype == F32
    return np.where(fin, clean(v), F32(0)).astype(F32)


def var_accum(m2, n):
    """RESTIR_DENOISE_VAR_ACCUM's plane [h][w] of the accumulation's m2 [h][w][3] after n frames"""
    m2 = np.ascontiguousarray(m2, F32)
    inv = F32(1.0) / (F32(n) * F32(n - 1))
    with np.errstate(all="ignore"):
        s = np.sqrt(m2 * inv)
        sl = lum(s)
        v = sl * sl
    assert v.dtype == F32
    return clean(v)


def level(c, v, G, s, normal_power_log2, sigma_plane, sigma_lum):
    """one level with step s over the image c [h][w][3] and the variance v [h][w]: (colour, variance)"""
    t = G[4]
    h, w = c.shape[:2]
    fin = np.isfinite(c).all(axis=-1)
    with np.errstate(all="ignore"):
        gn, gd = np.zeros((h, w), F32), np.zeros((h, w), F32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                pq = window(h, w, dy, dx)
                if pq is None:
                    continue
                p, q = pq
                gw = G3[dy + 1] * G3[dx + 1]
                gn[p] = gn[p] + gw * v[q]
                gd[p] = gd[p] + gw
        gv = gn / gd
        inv_den = F32(1.0) / (F32(sigma_lum) * np.sqrt(gv) + F32(1e-6))
        l = lum(c)
        inv_s = F32(1.0) / (F32(sigma_plane) * t)
        sw, sv = np.zeros((h, w), F32), np.zeros((h, w), F32)
        sc = np.zeros((h, w, 3), F32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                pq = window(h, w, s * dy, s * dx)
                if pq is None:
                    continue   # every such tap lies outside the image
                p, q = pq
                hk = K[dy + 2] * K[dx + 2]
                ok = fin[q].copy()
                if dx == 0 and dy == 0:
                    wt = np.full(ok.shape, hk, F32)
                else:
                    r = np.abs(l[q] - l[p]) * inv_den[p]
                    wl = F32(1.0) / (F32(1.0) + r * r)
                    wt = geo_weight(G, p, q, hk, inv_s, normal_power_log2) * wl
                ok &= wt > 0
                assert wt.dtype == F32
                sw[p] = np.where(ok, sw[p] + wt, sw[p])
                sc[p] = np.where(ok[..., None], sc[p] + wt[..., None] * c[q], sc[p])
                sv[p] = np.where(ok, sv[p] + (wt * wt) * v[q], sv[p])
        out = sc / sw[..., None]
        vout = sv / (sw * sw)
    assert out.dtype == F32 and vout.dtype == F32
    # a centre that is not finite keeps its input's bits, and its variance
    out = np.where(fin[..., None], out.view(U32), np.ascontiguousarray(c, F32).view(U32)).view(F32)
    vout = np.where(fin, vout.view(U32), np.ascontiguousarray(v, F32).view(U32)).view(F32)
    return out, vout


def denoise(rgb, var, n_t, p_mat, miss_material, iterations, normal_power_log2, sigma_plane, sigma_lum):
    """(the filtered image [h][w][3], the last level's variance [h][w]) of rgb [h][w][3] (row 0 = top); var [h][w]: the
    initial plane, None: the spatial estimate.  No tone mapping"""
    c = np.ascontiguousarray(rgb, F32)
    h, w = c.shape[:2]
    G = spec.guides(n_t, p_mat, w, h, miss_material)
    v = var_spatial(c, G, normal_power_log2, sigma_plane) if var is None else clean(np.asarray(var, F32).reshape(h, w))
    for i in range(iterations):
        c, v = level(c, v, G, 1 << i, normal_power_log2, sigma_plane, sigma_lum)
    return c, v
