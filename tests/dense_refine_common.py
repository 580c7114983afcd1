"""The scenes of the coarse-to-fine dense tests: dense_common's four cameras (same seeds, poses,
distortion and range) rendered at a fine size, and their coarse views as the float32 2 x 2 mean.  The
restated results that more than one test needs are computed once here and shared."""
import functools

import numpy as np

import dense_common as dc
import dense_restatement as dr
from imageanalysis_amd import dense

F32 = np.float32
W, H, FOCAL = 128, 96, 86.0
COARSE_PLANES = dc.PLANES                # 13 planes at 64 x 48
NEIGHBOURS = [[1, 2, 3], [0, 2, 3], [0, 1], [0]]


def fine_view(surface, k, h=H, w=W, focal=FOCAL):
    """camera k of dense_common at h x w -> (View, true depth)"""
    rng = np.random.default_rng(11 + 101 * k)
    R = dc._rot(*rng.uniform(-0.04, 0.04, 3)).dot(dc.NADIR)
    c = dc.CENTRES[k]
    C = np.array([c[0], c[1], -dc.ALTITUDE])
    K = np.array([focal, focal, (w - 1) / 2.0, (h - 1) / 2.0])
    G, rays, t = dc.render(surface, R, C, K, dc.DIST, h, w)
    return dense.View(G, K, dc.DIST, R, C, rays=rays, name='%s%d' % (surface, k)), t


def halve(v):
    """the coarse view of an even-sized view: the float32 2 x 2 mean, K by dense.scaled_K"""
    G = np.asarray(v.G, F32)
    h, w = G.shape
    assert h % 2 == 0 and w % 2 == 0
    g = ((G[0::2, 0::2] + G[0::2, 1::2]) + (G[1::2, 0::2] + G[1::2, 1::2])) * F32(0.25)
    K = dense.scaled_K(v.K, w, h, w // 2, h // 2)
    return dense.View(g.astype(F32), K, v.dist, v.R, v.C, rays=dc.host_rays(K, v.dist, h // 2, w // 2), name=v.name)


@functools.lru_cache(maxsize=None)
def scene(surface, h=H, w=W, focal=FOCAL):
    """-> (fine views, true depths) of the four cameras"""
    made = [fine_view(surface, k, h, w, focal) for k in range(len(dc.CENTRES))]
    return [m[0] for m in made], [m[1] for m in made]


@functools.lru_cache(maxsize=None)
def coarse_scene(surface):
    """-> the 64 x 48 views under scene(surface)"""
    return [halve(v) for v in scene(surface)[0]]


@functools.lru_cache(maxsize=None)
def coarse_sweep(surface):
    """the restated 13-plane sweep of coarse view 0 against views 1 - 3 -> plane, score, depth, around"""
    cv = coarse_scene(surface)
    return dr.sweep(cv[0], cv[1:], dc.W_FAR, dc.W_NEAR, COARSE_PLANES, radius=3)


@functools.lru_cache(maxsize=None)
def guided(surface, ratio):
    """fine view 0 against views 1 - 3, guided by coarse_sweep(surface) with pad = ratio
    -> (windows, (plane, score, depth, around))"""
    import dense_refine_restatement as rr
    fv, _ = scene(surface)
    T = dense.refine_planes(COARSE_PLANES, ratio)
    windows = rr.guide(coarse_sweep(surface)[2], (H, W), dc.W_FAR, dc.W_NEAR, T, radius=3, pad=ratio)
    return windows, rr.sweep_guided(fv[0], fv[1:], dc.W_FAR, dc.W_NEAR, T, windows, radius=3)


@functools.lru_cache(maxsize=None)
def fine_sweep(surface, planes):
    """the restated plain sweep of fine view 0 against views 1 - 3"""
    fv, _ = scene(surface)
    return dr.sweep(fv[0], fv[1:], dc.W_FAR, dc.W_NEAR, planes, radius=3)


def guide_cases():
    """(name, coarse depth map, (h, w), T, radius, pad) of the guide's tests: NaN holes, a tile whose
    whole box is NaN, depths on and beyond the range's ends, no pad and a large one, partial tiles and a
    size ratio that is not 2"""
    rng = np.random.default_rng(7)
    cases = []

    def depths(hc, wc, holes):
        wv = rng.uniform(dc.W_FAR, dc.W_NEAR, (hc, wc))
        d = (1.0 / wv).astype(F32)
        d[rng.uniform(size=d.shape) < holes] = np.nan
        return d

    d = depths(48, 64, 0.3)
    d[:14, :22] = np.nan                                   # the whole box of tile (0, 0)
    cases.append(('holes', d, (96, 128), 97, 3, 8))
    cases.append(('no pad', d, (96, 128), 97, 3, 0))
    cases.append(('large pad', d, (96, 128), 49, 2, 60))
    e = depths(48, 64, 0.0)
    e[0:20, 0:30] = F32(dc.Z_FAR)                          # on the ends of the range
    e[30:48, 40:64] = F32(dc.Z_NEAR)
    e[20:30, :] = F32(1e-30)                               # far beyond them
    e[0, 0], e[47, 63], e[25, 5], e[25, 6] = F32(1e30), F32(-5.0), F32(0.0), F32(np.inf)
    cases.append(('range ends', e, (96, 128), 97, 3, 0))
    cases.append(('range ends padded', e, (96, 128), 13, 7, 2))
    cases.append(('partial tiles', depths(25, 35, 0.2), (50, 70), 49, 2, 4))
    cases.append(('ratio not 2', depths(22, 30, 0.2), (55, 75), 49, 3, 4))
    # camera 0 over the roof at 75 x 55 (f = 50.4) and, by dense.scaled_K, at 30 x 22 (f = 20.16): its true depths
    cases.append(('rendered 30 x 22', fine_view('roof', 0, 22, 30, 20.16)[1].astype(F32), (55, 75), 49, 3, 4))
    cases.append(('one coarse pixel', depths(1, 1, 0.0), (17, 33), 2, 1, 0))
    cases.append(('all NaN', np.full((22, 30), np.nan, F32), (55, 75), 25, 3, 1))
    return cases
