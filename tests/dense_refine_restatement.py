"""imageanalysis_amd/dense.py's REFINEMENT RULES restated in numpy on dense_restatement's aggregate:
the guide (a coarse depth map -> the window table) and the guided sweep.  csrc/dense_refine.hip and the
guided form of csrc/dense_sweep.hip are held to these functions bit for bit."""
import numpy as np

import dense_restatement as dr

F32 = dr.F32
NAN32 = dr.NAN32
TILE_W, TILE_H = 32, 16


def tiles(h, w):
    return (h + TILE_H - 1) // TILE_H, (w + TILE_W - 1) // TILE_W


def _spans(n, nc, tile, r):
    """per tile along one axis: the inclusive range of coarse pixels"""
    t = np.arange((n + tile - 1) // tile, dtype=np.int64)
    a0 = np.maximum(tile * t - r, 0)
    a1 = np.minimum(tile * t + tile - 1 + r, n - 1)
    c0 = np.maximum(((2 * a0 + 1) * nc) // (2 * n) - 1, 0)
    c1 = np.minimum(((2 * a1 + 1) * nc) // (2 * n) + 1, nc - 1)
    return c0, c1


def guide(coarse_depth, fine_hw, w_far, w_near, total, radius=3, pad=0):
    """-> windows int32 [tiles_y, tiles_x, 2] = (first, count)"""
    Dc = np.asarray(coarse_depth, F32)
    hc, wc = Dc.shape
    h, w = fine_hw
    step = dr.plane_step(w_far, w_near, total)
    with np.errstate(invalid='ignore', divide='ignore'):
        ok = np.isfinite(Dc) & (Dc > 0)
        wv = 1.0 / np.where(ok, Dc, F32(1)).astype(np.float64)
    lo_src, hi_src = np.where(ok, wv, np.inf), np.where(ok, wv, -np.inf)
    (r0, r1), (c0, c1) = _spans(h, hc, TILE_H, radius), _spans(w, wc, TILE_W, radius)
    out = np.zeros(tiles(h, w) + (2,), np.int32)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            box = (slice(r0[ty], r1[ty] + 1), slice(c0[tx], c1[tx] + 1))
            wmin, wmax = lo_src[box].min(), hi_src[box].max()
            if not wmin < np.inf:
                continue
            with np.errstate(over='ignore'):
                lo = np.floor((wmin - w_far) / step) - float(pad)
                hi = np.ceil((wmax - w_far) / step) + float(pad)
            lo, hi = int(min(max(lo, 0.0), total - 1.0)), int(min(max(hi, 0.0), total - 1.0))
            out[ty, tx] = (lo, hi - lo + 1)
    return out


def per_pixel(windows, h, w):
    """the table spread over the pixels -> first, end int32 [h, w] (end = first + count)"""
    windows = np.asarray(windows)
    assert windows.shape == tiles(h, w) + (2,)
    px = np.repeat(np.repeat(windows, TILE_H, 0), TILE_W, 1)[:h, :w]
    return px[:, :, 0].astype(np.int32), (px[:, :, 0] + px[:, :, 1]).astype(np.int32)


def sweep_guided(ref, nbs, w_far, w_near, total, windows, radius=3, min_var=4.0, min_score=0.6):
    """-> plane int32, score, depth float32 [h, w], around float32 [h, w, 3]; dr.sweep with the planes
    outside a pixel's window invalid, and the window-edge rule in front of the depth"""
    shape = np.asarray(ref.G).shape
    first, end = per_pixel(windows, *shape)
    step = dr.plane_step(w_far, w_near, total)
    best = -np.ones(shape, np.int32)
    s0, sm, sp, prev = (np.full(shape, NAN32, F32) for _ in range(4))
    live = end > first
    d_lo, d_hi = (int(first[live].min()), int(end[live].max())) if live.any() else (0, 0)
    for d in range(d_lo, d_hi):                            # (a plane in no window changes nothing)
        S = dr.aggregate(ref, nbs, 1.0 / (w_far + d * step), radius, min_var)
        S = np.where((d >= first) & (d < end), S, NAN32).astype(F32)
        with np.errstate(invalid='ignore'):
            win = ~np.isnan(S) & ((best < 0) | (S > s0))
        after = ~win & (best >= 0) & (best == d - 1)
        sm = np.where(win, prev, sm)
        sp = np.where(win, NAN32, np.where(after, S, sp))
        s0 = np.where(win, S, s0)
        best = np.where(win, d, best).astype(np.int32)
        prev = S
    with np.errstate(invalid='ignore', divide='ignore'):
        den = (sm - F32(2) * s0) + sp
        curved = (best >= 0) & ~np.isnan(sm) & ~np.isnan(sp) & (den < 0)
        off = (F32(0.5) * (sm - sp)) / den
        off = np.where(curved, np.minimum(np.maximum(off, F32(-0.5)), F32(0.5)), F32(0)).astype(F32)
        clipped = ((best == first) & (first > 0)) | ((best == end - 1) & (end < total))
        kept = (best >= 0) & (s0 >= F32(min_score)) & ~clipped
        depth = (1.0 / (w_far + (best.astype(np.float64) + off.astype(np.float64)) * step)).astype(F32)
    depth = np.where(kept, depth, NAN32).astype(F32)
    return best, s0.astype(F32), depth, np.stack([sm, s0, sp], 2).astype(F32)


def refine(fine_views, neighbours, ranges, coarse_depth, coarse_keep, planes, ratio=4, pad=None, radius=3,
           min_var=4.0, min_score=0.6, eps=0.01, min_agree=2):
    """dense.refine through the restatements -> dict(windows, plane, score, depth, keep, ned, total)"""
    V = len(fine_views)
    h, w = np.asarray(fine_views[0].G).shape
    total = (planes - 1) * ratio + 1
    pad = ratio if pad is None else pad
    windows = np.zeros((V,) + tiles(h, w) + (2,), np.int32)
    plane = -np.ones((V, h, w), np.int32)
    score = np.full((V, h, w), NAN32, F32)
    depth = np.full((V, h, w), NAN32, F32)
    for i in range(V):
        if ranges[i] is None or not neighbours[i]:
            continue
        w_far, w_near = 1.0 / float(ranges[i][1]), 1.0 / float(ranges[i][0])
        g = np.where(np.asarray(coarse_keep[i]) != 0, np.asarray(coarse_depth[i], F32), NAN32).astype(F32)
        windows[i] = guide(g, (h, w), w_far, w_near, total, radius, pad)
        plane[i], score[i], depth[i], _ = sweep_guided(fine_views[i], [fine_views[j] for j in neighbours[i]], w_far,
                                                       w_near, total, windows[i], radius, min_var, min_score)
    keep, ned = dr.check(depth, fine_views, neighbours, eps, min_agree)
    return dict(windows=windows, plane=plane, score=score, depth=depth, keep=keep, ned=ned, total=total)
