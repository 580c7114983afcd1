"""CPU: the coarse-to-fine rules of imageanalysis_amd/dense.py (REFINEMENT RULES) as restated by
tests/dense_refine_restatement.py -- the guide against a per-tile loop written from the rules, the guided
sweep against the plain one, what the refinement buys on the scenes' true depths, and the argument checks."""
import math

import numpy as np
import pytest

import dense_common as dc
import dense_refine_common as rc
import dense_refine_restatement as rr
import dense_restatement as dr
from imageanalysis_amd import dense, kernels


def _loop_guide(Dc, fine_hw, w_far, w_near, T, r, pad):
    """the Guide rule, tile by tile and pixel by pixel, in Python's integers and doubles"""
    hc, wc = Dc.shape
    h, w = fine_hw
    step = (w_near - w_far) / (T - 1)
    tiles_y, tiles_x = -(-h // 16), -(-w // 32)
    out = np.zeros((tiles_y, tiles_x, 2), np.int32)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            x0, x1 = max(32 * tx - r, 0), min(32 * tx + 31 + r, w - 1)
            y0, y1 = max(16 * ty - r, 0), min(16 * ty + 15 + r, h - 1)
            c0, c1 = max(((2 * x0 + 1) * wc) // (2 * w) - 1, 0), min(((2 * x1 + 1) * wc) // (2 * w) + 1, wc - 1)
            r0, r1 = max(((2 * y0 + 1) * hc) // (2 * h) - 1, 0), min(((2 * y1 + 1) * hc) // (2 * h) + 1, hc - 1)
            wv = [1.0 / float(Dc[y, x]) for y in range(r0, r1 + 1) for x in range(c0, c1 + 1)
                  if math.isfinite(Dc[y, x]) and Dc[y, x] > 0]
            if not wv:
                continue
            lo = math.floor((min(wv) - w_far) / step) - pad
            hi = math.ceil((max(wv) - w_far) / step) + pad
            lo, hi = min(max(lo, 0), T - 1), min(max(hi, 0), T - 1)
            out[ty, tx] = (lo, hi - lo + 1)
    return out


@pytest.mark.parametrize('case', rc.guide_cases(), ids=lambda c: c[0])
def test_guide_against_a_loop(case):
    name, Dc, fine_hw, T, r, pad = case
    got = rr.guide(Dc, fine_hw, dc.W_FAR, dc.W_NEAR, T, radius=r, pad=pad)
    want = _loop_guide(Dc, fine_hw, dc.W_FAR, dc.W_NEAR, T, r, pad)
    assert got.dtype == np.int32 and got.shape == rr.tiles(*fine_hw) + (2,)
    assert np.array_equal(got, want)
    first, count = got[..., 0], got[..., 1]
    assert (first >= 0).all() and (count >= 0).all() and (first + count <= T).all()
    if name == 'holes':
        assert tuple(got[0, 0]) == (0, 0) and (count[1:, 1:] > 0).all()
    if name == 'all NaN':
        assert not got.any()
    if name == 'range ends':
        assert tuple(got[0, 0]) == (0, 1)                   # (1e30 m: beyond the far end, clamped onto it)
        assert (first + count == T)[2].all()                # (1e-30 m in coarse rows 20 - 29: beyond the near end)
    if name == 'large pad':
        assert (got[count > 0] == (0, T)).all()


@pytest.mark.parametrize('T', [13, 2])
def test_full_windows_are_the_plain_sweep(T):
    views, _ = dc.scene('roof')
    windows = np.zeros(rr.tiles(dc.H, dc.W) + (2,), np.int32)
    windows[..., 1] = T
    got = rr.sweep_guided(views[0], views[1:], dc.W_FAR, dc.W_NEAR, T, windows, radius=3)
    want = dr.sweep(views[0], views[1:], dc.W_FAR, dc.W_NEAR, T, radius=3)
    assert (want[0] >= 0).any() and np.isfinite(want[2]).any()
    for g, e in zip(got, want):
        assert g.dtype == e.dtype and np.array_equal(dc.bits(g), dc.bits(e))


def _errors(depth, truth, step):
    kept = ~np.isnan(depth)
    return kept, np.abs(1.0 / depth[kept].astype(np.float64) - 1.0 / truth[kept]) / step


@pytest.mark.parametrize('surface, ratio, share', [('slope', 8, 0.99), ('roof', 8, 0.93), ('slope', 4, 0.99),
                                                   ('roof', 4, 0.93)])
def test_refinement_finds_the_surface_in_fine_steps(surface, ratio, share):
    """Fine view 0 (128 x 96) against views 1 - 3, guided by the 13-plane sweep of the 64 x 48 views, held
    to the true depth in FINE plane steps; beside it the plain 13-plane sweep of the fine views.
    Measured by the restatements (guided: within one fine step / median error in fine steps / kept of 10980
    interior pixels; plain 13 planes: median error in fine steps):
        slope, ratio 8 (T = 97)   0.9995   0.125   10974     0.550
        roof,  ratio 8 (T = 97)   0.9530   0.075   10883     0.678
        slope, ratio 4 (T = 49)   0.9999   0.066   10974     0.275
        roof,  ratio 4 (T = 49)   0.9709   0.043   10875     0.339"""
    T = dense.refine_planes(rc.COARSE_PLANES, ratio)
    step = dr.plane_step(dc.W_FAR, dc.W_NEAR, T)
    truth = rc.scene(surface)[1][0]
    _windows, (_plane, _score, depth, _around) = rc.guided(surface, ratio)
    inside = dc.interior(rc.H, rc.W, 3)
    kept, err = _errors(depth, truth, step)
    _kept13, err13 = _errors(rc.fine_sweep(surface, rc.COARSE_PLANES)[2], truth, step)
    within = float((err <= 1.0).mean())
    print('%s, ratio %d (T = %d): within a fine step %.4f, median %.3f fine steps, kept %d of %d interior pixels; '
          'plain %d planes: median %.3f' % (surface, ratio, T, within, float(np.median(err)), int(kept.sum()),
                                            int(inside.sum()), rc.COARSE_PLANES, float(np.median(err13))))
    assert not kept[~inside].any()
    assert within >= share
    assert np.median(err) <= 0.5 * np.median(err13)
    assert kept.sum() >= 0.9 * inside.sum()


@pytest.mark.parametrize('surface, ratio', [('slope', 8), ('roof', 8), ('slope', 4), ('roof', 4)])
def test_guided_agrees_with_the_exhaustive_fine_sweep(surface, ratio):
    """Where the guided sweep and the plain sweep of all T planes both keep a pixel, the depth bits are equal.
    Measured: slope 8: 1.0, 26.6 of 97 planes per tile; roof 8: 0.99991, 25.9; slope 4: 1.0, 14.2 of 49;
    roof 4: 0.99991, 13.9."""
    T = dense.refine_planes(rc.COARSE_PLANES, ratio)
    windows, (_plane, _score, depth, _around) = rc.guided(surface, ratio)
    full = rc.fine_sweep(surface, T)[2]
    both = ~np.isnan(depth) & ~np.isnan(full)
    same = float((dc.bits(depth)[both] == dc.bits(full)[both]).mean())
    count = windows[..., 1]
    print('%s, ratio %d: equal bits on %.5f of %d pixels, %.1f of %d planes per tile (least %d, most %d)'
          % (surface, ratio, same, int(both.sum()), float(count.mean()), T, int(count.min()), int(count.max())))
    assert both.sum() >= 0.9 * dc.interior(rc.H, rc.W, 3).sum()
    assert same >= 0.999
    assert (count > 0).all()
    assert count.mean() < T / 2.0


# ---- argument checks: a ValueError before any device call (there is no device here) ----
def test_refine_planes():
    assert dense.refine_planes(13, 8) == 97 and dense.refine_planes(64, 4) == 253 and dense.refine_planes(2, 1) == 2
    for planes, ratio in ((13, 0), (13, -2), (1, 4), (4096, 17), (65536, 2)):
        with pytest.raises(ValueError):
            dense.refine_planes(planes, ratio)
    assert dense.refine_planes(65536, 1) == kernels.DENSE_GUIDED_MAX_PLANES == 65536


def test_argument_checks():
    fv, _ = rc.scene('slope')
    ref, nbs = fv[0], fv[1:]
    shape = rr.tiles(rc.H, rc.W) + (2,)
    full = np.zeros(shape, np.int32)
    full[..., 1] = 49
    ok = dict(w_far=dc.W_FAR, w_near=dc.W_NEAR, total=49, windows=full)
    bad_tables = [full[:-1], full[:, :-1], full[..., :1], full.astype(np.int64), full.astype(np.float32), full.reshape(-1)]
    for field, value in ((0, -1), (1, -1), (1, 50), (0, 1)):
        t = full.copy()
        t[2, 1, field] = value                              # (first 1 with count 49 leaves the 49 planes)
        bad_tables.append(t)
    t = full.copy()
    t[0, 0] = (2 ** 31 - 1, 2 ** 31 - 1)                    # (a sum that does not fit an int32)
    bad_tables.append(t)
    for t in bad_tables:
        with pytest.raises(ValueError, match='window'):
            kernels.dense_sweep_guided(ref, nbs, **dict(ok, windows=t))
    for bad in (dict(total=1), dict(total=kernels.DENSE_GUIDED_MAX_PLANES + 1), dict(radius=0), dict(radius=8),
                dict(w_near=dc.W_FAR), dict(total=48)):
        with pytest.raises(ValueError):
            kernels.dense_sweep_guided(ref, nbs, **dict(ok, **bad))
    with pytest.raises(ValueError):
        kernels.dense_sweep_guided(ref, [], **ok)
    coarse = np.full((48, 64), 100.0, np.float32)
    gok = dict(fine_hw=(rc.H, rc.W), w_far=dc.W_FAR, w_near=dc.W_NEAR, total=49)
    for bad in (dict(total=1), dict(total=65537), dict(radius=0), dict(radius=8), dict(pad=-1), dict(w_far=0.0),
                dict(w_near=dc.W_FAR), dict(fine_hw=(0, 5)), dict(fine_hw=(5, 16385))):
        with pytest.raises(ValueError):
            kernels.dense_guide(coarse, **dict(gok, **bad))
    with pytest.raises(ValueError):
        kernels.dense_guide(coarse.reshape(-1), **gok)
    # refine
    nb, ranges = rc.NEIGHBOURS, [(dc.Z_NEAR, dc.Z_FAR)] * 4
    maps = dense.DepthMaps(depth=np.zeros((4, 48, 64), np.float32), keep=np.zeros((4, 48, 64), np.uint8))
    for bad in (dict(ratio=0), dict(ratio=-1), dict(planes=1), dict(planes=4096, ratio=17), dict(pad=-1), dict(radius=8)):
        with pytest.raises(ValueError):
            dense.refine(fv, nb, ranges, maps, **dict(dict(planes=13), **bad))
    three = dense.DepthMaps(depth=np.zeros((3, 48, 64), np.float32), keep=np.zeros((3, 48, 64), np.uint8))
    with pytest.raises(ValueError, match='views'):
        dense.refine(fv, nb, ranges, three, 13)
    with pytest.raises(ValueError):
        dense.refine(fv, nb[:3], ranges, maps, 13)
    with pytest.raises(ValueError):
        dense.refine(fv, nb, [(140.0, 60.0)] * 4, maps, 13)
    with pytest.raises(ValueError):
        dense.refine(fv, nb, ranges, dense.DepthMaps(depth=maps.depth, keep=maps.keep[:, :-1]), 13)


def test_entry_points_check_their_arguments_without_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    one = _lib.c_void_p(16)                                 # (never dereferenced: every call below is refused)
    g = L.iamx_dense_guide
    assert g(one, 64, 48, 128, 96, 0.01, 0.02, 1, 3, 0, one, None) == -1
    assert g(one, 64, 48, 128, 96, 0.01, 0.02, 65537, 3, 0, one, None) == -1
    assert g(one, 64, 48, 128, 96, 0.01, 0.02, 49, 0, 0, one, None) == -1
    assert g(one, 64, 48, 128, 96, 0.01, 0.02, 49, 8, 0, one, None) == -1
    assert g(one, 64, 48, 128, 96, 0.01, 0.02, 49, 3, -1, one, None) == -1
    assert g(one, 0, 48, 128, 96, 0.01, 0.02, 49, 3, 0, one, None) == -1
    assert g(one, 64, 48, 128, 16385, 0.01, 0.02, 49, 3, 0, one, None) == -1
    assert g(one, 64, 48, 128, 96, 0.02, 0.01, 49, 3, 0, one, None) == -1
    assert g(None, 64, 48, 128, 96, 0.01, 0.02, 49, 3, 0, one, None) == -1
    assert g(one, 64, 48, 128, 96, 0.01, 0.02, 49, 3, 0, None, None) == -1
    s = L.iamx_dense_sweep_guided
    front, back = (one, one, one, one, one), (one, one, one, one, None)
    assert s(*(front + (4, 4, 1, 1, 0.01, 0.02, 3, 4.0, 0.6, one) + back)) == -1
    assert s(*(front + (4, 4, 1, 65537, 0.01, 0.02, 3, 4.0, 0.6, one) + back)) == -1
    assert s(*(front + (4, 4, 1, 49, 0.01, 0.02, 8, 4.0, 0.6, one) + back)) == -1
    assert s(*(front + (4, 4, 17, 49, 0.01, 0.02, 3, 4.0, 0.6, one) + back)) == -1
    assert s(*(front + (4, 4, 1, 49, 0.02, 0.01, 3, 4.0, 0.6, one) + back)) == -1
    assert s(*(front + (4, 4, 1, 49, 0.01, 0.02, 3, 4.0, 0.6, None) + back)) == -1
    assert s(*((None,) + front[1:] + (4, 4, 1, 49, 0.01, 0.02, 3, 4.0, 0.6, one) + back)) == -1
