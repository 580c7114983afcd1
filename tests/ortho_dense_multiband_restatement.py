"""The true orthophoto's blend (imageanalysis_amd/ortho.py, THE TRUE-ORTHO RULES, "multiband": owner,
layer, pyramids) restated in numpy.  Heights, projection, sample and mode best's ownership are
tests/ortho_dense_restatement.py's, levels, reduce, expand and the quotient
tests/ortho_multiband_restatement.py's; this file only puts them together.  Imports nothing from the
package.

Every image is computed over the WHOLE mosaic here: the device works on each image's work box and on
the extents that follow from it, and equality with this is what checks both.

A camera is ortho_dense_restatement's (K4 at the frame's size, dist5, R, C)."""
import numpy as np

import ortho_dense_restatement as dr
import ortho_multiband_restatement as mb

F32 = np.float32


def cover(dsm, x0, y1, gsd, ss, cam, frame_hw):
    """the cover rule over the whole mosaic -> (bool [H ss][W ss], fx_, fy_)"""
    Z32 = np.asarray(dsm, F32)
    H, W = Z32.shape
    g = gsd / ss
    h = dr.heights(Z32, ss)
    e = (x0 + (np.arange(W * ss, dtype=np.float64) + 0.5) * g)[None, :]
    n = (y1 - (np.arange(H * ss, dtype=np.float64) + 0.5) * g)[:, None]
    h_s, w_s = frame_hw
    _d0, _d1, Zc, fu, fv = dr.project(cam, n, e, h)
    dh = (-cam[3][2]) - h
    with np.errstate(invalid='ignore'):
        on = ~np.isnan(h) & (Zc > 0) & (fu >= 0) & (fu <= w_s - 1) & (fv >= 0) & (fv <= h_s - 1) & (dh > 0)
    return on, fu, fv


def layer(k, on, fu, fv, index, frame):
    """-> C_k float32 [Ho][Wo][3] (the sample wherever `on`, 0 elsewhere), A_k float32 [Ho][Wo][1]"""
    C = np.zeros(on.shape + (3,), F32)
    C[on] = dr.sample(frame, fu[on], fv[on]).astype(F32)
    return C, (index == k).astype(F32)[:, :, None]


def compose(dsm, x0, y1, gsd, cams, frames, bands=5, ss=1, bias=None, visible_only=False):
    """-> dict(bgr uint8 [Ho][Wo][3], index int32, count uint16, bands=L, N: [L] float32 [H_l][W_l][3],
    D: [L] float32 [H_l][W_l][1]).  visible_only: the layer's colour only where the image also SEES
    the pixel -- not the rule; tests use it to show what the rule is for."""
    if isinstance(bands, bool) or int(bands) != bands:
        raise ValueError("bands is an integer 1 .. 16")
    best = dr.compose(dsm, x0, y1, gsd, cams, frames, 'best', ss=ss, bias=bias)     # (and its argument checks)
    index, count = best['index'], best['count']
    Ho, Wo = index.shape
    sizes = mb.levels(Ho, Wo, int(bands))
    L = len(sizes)
    N = [np.zeros((h, w, 3), F32) for h, w in sizes]
    D = [np.zeros((h, w, 1), F32) for h, w in sizes]
    for k, (cam, frame) in enumerate(zip(cams, frames)):
        on, fu, fv = cover(dsm, x0, y1, gsd, ss, cam, np.shape(frame)[:2])
        if visible_only:
            on = best['visible'][k]
        if not on.any() and not (index == k).any():
            continue                                    # (an all-zero layer adds +0 everywhere)
        GC, GA = [None] * L, [None] * L
        GC[0], GA[0] = layer(k, on, fu, fv, index, frame)
        for l in range(L - 1):
            GC[l + 1], GA[l + 1] = mb.reduce(GC[l]), mb.reduce(GA[l])
        for l in range(L):
            LP = GC[l] - mb.expand(GC[l + 1], *sizes[l]) if l < L - 1 else GC[l]
            N[l] = N[l] + GA[l] * LP
            D[l] = D[l] + GA[l]
    M = mb.quotient(N[L - 1], D[L - 1])
    for l in range(L - 2, -1, -1):
        M = mb.quotient(N[l], D[l]) + mb.expand(M, *sizes[l])
    bgr = np.floor(np.minimum(np.maximum(M, F32(0.0)), F32(255.0)) + mb.HALF).astype(np.uint8)
    bgr[count == 0] = 0
    return dict(bgr=bgr, index=index, count=count, bands=L, N=N, D=D)
