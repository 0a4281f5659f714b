"""The specification of restir_denoise / restir_denoise_host in numpy (include/restir_c.h "denoising the last image"): the
edge-avoiding a-trous filter restated with vectorised float32 operations -- every numpy step is one float32 operation,
divide and sqrt correctly rounded, nothing contracted -- over whole shifted planes instead of per pixel, the 25 taps in the
contract's order (dy outside, dx inside).  Nothing under oracle/ knows the feature.  Helpers of tests/test_denoise_host.py
and tests/test_gpu_denoise.py; no test lives here."""
import numpy as np

F32 = np.float32
U32 = np.uint32
K = [F32(1 / 16), F32(1 / 4), F32(3 / 8), F32(1 / 4), F32(1 / 16)]


def guides(n_t, p_mat, w, h, miss_material):
    """(g [h][w][3], P [h][w][3], material bits [h][w], flat [h][w], t [h][w]) in image rows (row 0 = top) of the
    G-buffer planes n_t / p_mat ([h * w][4], row y = 0 at the bottom)"""
    nt = np.ascontiguousarray(n_t, F32).reshape(h, w, 4)[::-1]
    pm = np.ascontiguousarray(p_mat, F32).reshape(h, w, 4)[::-1]
    N, t, P = nt[..., :3], nt[..., 3], pm[..., :3]
    mat = np.ascontiguousarray(pm[..., 3]).view(U32)
    with np.errstate(all="ignore"):
        l2 = (N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2]
        flat = (mat == U32(miss_material)) | ~(l2 > 0) | ~np.isfinite(l2)
        r = np.sqrt(l2)
        g = np.where(flat[..., None], F32(0), N / r[..., None]).astype(F32)
    assert l2.dtype == F32 and r.dtype == F32
    return g, np.ascontiguousarray(P), mat, flat, np.ascontiguousarray(t)


def level(c, G, s, normal_power_log2, sigma_plane):
    """one level with step s over the image c [h][w][3]"""
    g, P, mat, flat, t = G
    h, w = c.shape[:2]
    fin = np.isfinite(c).all(axis=-1)
    sw = np.zeros((h, w), F32)
    sc = np.zeros((h, w, 3), F32)
    with np.errstate(all="ignore"):
        inv_s = F32(1.0) / (F32(sigma_plane) * t)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                if y0 >= y1 or x0 >= x1:
                    continue   # every such tap lies outside the image
                p = (slice(y0, y1), slice(x0, x1))
                q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                hk = K[dy + 2] * K[dx + 2]
                ok = fin[q].copy()
                if dx == 0 and dy == 0:
                    wt = np.full(ok.shape, hk, F32)
                else:
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
                    ok &= mat[q] == mat[p]
                ok &= wt > 0
                assert wt.dtype == F32
                sw[p] = np.where(ok, sw[p] + wt, sw[p])
                sc[p] = np.where(ok[..., None], sc[p] + wt[..., None] * c[q], sc[p])
        out = sc / sw[..., None]
    assert out.dtype == F32
    # a centre that is not finite keeps its input's bits
    return np.where(fin[..., None], out.view(U32), np.ascontiguousarray(c, F32).view(U32)).view(F32)


def denoise(rgb, n_t, p_mat, miss_material, iterations, normal_power_log2, sigma_plane):
    """the filtered image [h][w][3] of rgb [h][w][3] (row 0 = top), no tone mapping"""
    c = np.ascontiguousarray(rgb, F32)
    h, w = c.shape[:2]
    G = guides(n_t, p_mat, w, h, miss_material)
    for i in range(iterations):
        c = level(c, G, 1 << i, normal_power_log2, sigma_plane)
    return c


def plane_gbuffer(w, h, normal=(0.0, 0.0, 2.0), material=0, t=5.0, spacing=0.01):
    """(n_t, p_mat) of a plane z = 0 seen head on: P = (x, y, 0) * spacing, one normal (unnormalised), one material"""
    n_t = np.zeros((h, w, 4), F32)
    p_mat = np.zeros((h, w, 4), F32)
    n_t[..., :3], n_t[..., 3] = normal, t
    ys, xs = np.mgrid[0:h, 0:w]
    p_mat[..., 0], p_mat[..., 1] = xs * F32(spacing), ys * F32(spacing)
    p_mat[..., 3] = np.array([material], U32).view(F32)[0]
    return n_t.reshape(-1, 4), p_mat.reshape(-1, 4)


def set_material(p_mat, w, h, mask_image_rows, material):
    """material of the pixels mask_image_rows [h][w] (row 0 = top) selects, in place"""
    pm = p_mat.reshape(h, w, 4)
    pm[..., 3][mask_image_rows[::-1]] = np.array([material], U32).view(F32)[0]
