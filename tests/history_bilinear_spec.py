"""The specification of the image history's bilinear gather (include/restir_c.h "The gather of restir_history_advance") in
numpy: one whole advance -- map, gather and fold.  Every numpy step is one float32 operation, divide correctly rounded,
nothing contracted, in csrc/history.h history_gather_bilinear's order.  It builds on tests/history_spec.py (the accept
tests' expressions, the fold) and on tests/test_reproject_host.py np_source's expressions, which np_source_at repeats to
return the continuous source position.  Helpers of tests/test_history_bilinear_host.py and
tests/test_gpu_history_bilinear.py; no test lives here.

Rows: G-buffer records and the map are in G-buffer rows (y = 0 bottom), images and state in image rows (row 0 = top)."""
import numpy as np

import history_spec as hs
from test_reproject_host import BEHIND, DEPTH, MISS, NONE, NORMAL, OFF_SCREEN, PREV_MISS, np_source, qrotate

F32, U32, I64 = np.float32, np.uint32, np.int64
NEAREST, BILINEAR = 0, 1


def np_source_at(cf, W, H, P):
    """np_source with the continuous position: (x, y, d, why, cfx, cfy); cfx = cfy = 0 where why is not NONE"""
    P = np.ascontiguousarray(P, F32)
    o = [F32(v) for v in cf.origin]
    q = [F32(v) for v in cf.quat]
    hw, hh = F32(cf.half_w), F32(cf.half_h)
    one, half = F32(1.0), F32(0.5)
    with np.errstate(all="ignore"):
        v = [P[:, a] - o[a] for a in range(3)]
        d = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        cx, cy, cz = qrotate((-q[0], -q[1], -q[2], q[3]), v)
        front = cz > F32(0.0)
        r = cx / cz
        nx = (-r) / hw
        s = cy / cz
        ny = s / hh
        cfx = ((nx + one) * half) * F32(W)
        cfy = ((ny + one) * half) * F32(H)
        fx = np.floor(cfx + half)
        fy = np.floor(cfy + half)
        on = (fx >= F32(0.0)) & (fx < F32(W)) & (fy >= F32(0.0)) & (fy < F32(H))
    why = np.where(~front, U32(BEHIND), np.where(~on, U32(OFF_SCREEN), U32(NONE))).astype(U32)
    ok = why == NONE
    x = np.where(ok, fx, 0).astype(U32)
    y = np.where(ok, fy, 0).astype(U32)
    assert d.dtype == F32 and cfx.dtype == F32 and fx.dtype == F32
    x0, y0, d0, why0 = np_source(cf, W, H, P)
    assert (x == x0).all() and (y == y0).all() and (why == why0).all() and (d.view(U32) == d0.view(U32)).all()
    return x, y, d, why, np.where(ok, cfx, F32(0.0)).astype(F32), np.where(ok, cfy, F32(0.0)).astype(F32)


def accept(kn, kmat, kcount, q, cn, cmat, d, miss_material):
    """history_accept of the kept records at flat G-buffer indices q against every current pixel: NONE or the reason"""
    with np.errstate(all="ignore"):
        depth = np.abs(F32(1.0) - kn[q, 3] / d) > F32(0.1)
        dot = (kn[q, 0] * cn[:, 0] + kn[q, 1] * cn[:, 1]) + kn[q, 2] * cn[:, 2]
        normal = dot < F32(0.90630778703)
    return np.where(kmat[q] == miss_material, PREV_MISS,
                    np.where(depth, DEPTH, np.where(normal, NORMAL,
                                                    np.where(kmat[q] != cmat, hs.MATERIAL,
                                                             np.where(kcount[q] == 0, hs.NO_HISTORY, NONE))))).astype(I64)


def advance(cf_prev, w, h, gb_cur, kept, mean, S, n, x, miss_material, max_frames, gather=BILINEAR, info=None):
    """One restir_history_advance.  gb_cur = (n_t, p_mat) [px][4] of the new camera; kept = (n_t [px][4], material [px]
    uint32), G-buffer rows, or None: nothing kept; mean, S [h][w][3], n [h][w]: the kept state, image rows; x [h][w][3]: the
    image.  Returns (mean, S, n, map [h][w]).  info (a dict, optional) receives per pixel of the G-buffer: "taps" (the number
    of contributing taps, 0 where the pixel is rejected), "rescued" (the nearest tap is rejected, another contributes) and
    "outside" (reasons 0 - 2 passed and a tap lies outside the image)."""
    cn, cp = gb_cur
    px = w * h
    n = np.asarray(n, U32).reshape(h, w)
    if kept is None:
        m = np.full(px, NONE - hs.NO_HISTORY, U32)
        return (*hs.fold(mean, S, n, m, x, max_frames), m.reshape(h, w))
    if gather == NEAREST:
        m = hs.np_map(cf_prev, w, h, gb_cur, (kept[0], kept[1], n), miss_material)
        return (*hs.fold(mean, S, n, m, x, max_frames), m.reshape(h, w))
    kn = np.ascontiguousarray(kept[0], F32).reshape(px, 4)
    kmat = np.minimum(np.asarray(kept[1], U32).reshape(-1), U32(miss_material))
    kcount = hs.flip(n, w, h).reshape(-1)                                       # -> G-buffer rows
    km = hs.flip(np.ascontiguousarray(mean, F32).reshape(h, w, 3), w, h).reshape(px, 3)
    ks = hs.flip(np.ascontiguousarray(S, F32).reshape(h, w, 3), w, h).reshape(px, 3)
    cmat = hs.material(cp, miss_material)
    sx, sy, d, why0, cfx, cfy = np_source_at(cf_prev, w, h, cp[:, :3])
    why0 = np.where(cmat == miss_material, MISS, why0).astype(I64)
    ok = why0 == NONE
    one = F32(1.0)
    x0f, y0f = np.floor(cfx), np.floor(cfy)
    fx, fy = cfx - x0f, cfy - y0f
    gx, gy = one - fx, one - fy
    x0, y0 = x0f.astype(I64), y0f.astype(I64)
    wt = [gx * gy, fx * gy, gx * fy, fx * fy]
    assert all(a.dtype == F32 for a in wt)
    jn = (sx.astype(I64) - x0) + 2 * (sy.astype(I64) - y0)
    assert ((jn[ok] >= 0) & (jn[ok] <= 3)).all(), "the nearest pixel is one of the four taps"
    contrib, tq = [], []
    why_n = np.full(px, hs.NO_HISTORY, I64)
    total = np.zeros(px, F32)
    outside = np.zeros(px, bool)
    for j in range(4):
        tx, ty = x0 + (j & 1), y0 + (j >> 1)
        inside = (tx >= 0) & (ty >= 0) & (tx < w) & (ty < h)
        outside |= ok & ~inside
        cand = ok & inside & (wt[j] > F32(0.0))
        q = np.where(cand, ty * w + tx, 0)
        why = accept(kn, kmat, kcount, q, cn, cmat, d, miss_material)
        why_n = np.where(cand & (jn == j), why, why_n)
        c = cand & (why == NONE)
        total = np.where(c, total + wt[j], total).astype(F32)
        contrib.append(c), tq.append(q)
    count = sum(c.astype(I64) for c in contrib)
    accepted = count > 0
    gm, gs = np.zeros((px, 3), F32), np.zeros((px, 3), F32)
    nf = np.zeros(px, F32)
    first = np.ones(px, bool)
    best = np.zeros(px, F32)
    bj = np.zeros(px, I64)
    with np.errstate(all="ignore"):
        for j in range(4):
            c, q = contrib[j], tq[j]
            v = wt[j] / total
            vv = v * v
            tm, ts, tn = v[:, None] * km[q], vv[:, None] * ks[q], v * kcount[q].astype(F32)
            init, more = (c & first)[:, None], (c & ~first)[:, None]
            gm = np.where(init, tm, np.where(more, gm + tm, gm))
            gs = np.where(init, ts, np.where(more, gs + ts, gs))
            nf = np.where(c & first, tn, np.where(c & ~first, nf + tn, nf))
            first &= ~c
            up = c & (wt[j] > best)
            best = np.where(up, wt[j], best)
            bj = np.where(up, j, bj)
        assert gm.dtype == F32 and gs.dtype == F32 and nf.dtype == F32
        gn = np.where(accepted, np.maximum(np.floor(nf + F32(0.5)), one), F32(0.0)).astype(U32)
    near_in = np.zeros(px, bool)
    for j in range(4):
        near_in |= contrib[j] & (jn == j)
    pick = np.where(near_in, jn, bj)
    src = (y0 + (pick >> 1)) * w + (x0 + (pick & 1))
    why = np.where(ok, np.where(accepted, NONE, why_n), why0)
    m = np.where(why == NONE, src, NONE - why).astype(U32)
    if info is not None:
        info.update(taps=count, rescued=accepted & ~near_in, outside=outside)
    # the fold of the gathered state: history_spec.fold over the gathered planes with the identity in place of the map
    ident = np.where(why == NONE, np.arange(px), NONE - why).astype(U32)
    acc = accepted[:, None]
    gm_i = hs.flip(np.where(acc, gm.view(U32), U32(0)).view(F32), w, h)
    gs_i = hs.flip(np.where(acc, gs.view(U32), U32(0)).view(F32), w, h)
    return (*hs.fold(gm_i, gs_i, hs.flip(gn, w, h), ident, x, max_frames), m.reshape(h, w))
