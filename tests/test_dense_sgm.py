"""CPU: the SEMI-GLOBAL RULES of imageanalysis_amd/dense.py.  The numpy restatement
(tests/dense_sgm_restatement.py) against a per-pixel Python loop of the recurrence, its properties, what
it buys over winner-take-all on four synthetic inputs, and the argument checks."""
import numpy as np
import pytest

import dense_common as dc
import dense_restatement as dr
import dense_sgm_common as sc
import dense_sgm_restatement as ds
from imageanalysis_amd import dense, kernels


# ---- the restatement against the loop ----
def loop_path_cost(vol, direction, p1, p2, c_invalid):
    """L_r by the rule's own words: one pixel, one plane at a time, along every path from its start"""
    h, w, planes = vol.shape
    dx, dy = direction
    L = {}

    def cost(x, y, d):
        c = int(vol[y, x, d])
        return c if c < 255 else c_invalid

    def at(x, y):
        if (x, y) in L:
            return L[(x, y)]
        xp, yp = x - dx, y - dy
        if not (0 <= xp < w and 0 <= yp < h):
            out = [cost(x, y, d) for d in range(planes)]
        else:
            prev = at(xp, yp)
            m = min(prev)
            out = []
            for d in range(planes):
                cand = [prev[d], m + p2]
                if d - 1 >= 0:
                    cand.append(prev[d - 1] + p1)
                if d + 1 < planes:
                    cand.append(prev[d + 1] + p1)
                out.append(cost(x, y, d) + min(cand) - m)
        L[(x, y)] = out
        return out

    # (from the far end of every path backwards would recurse h + w deep: walk in path order instead)
    xs = range(w) if dx >= 0 else range(w - 1, -1, -1)
    ys = range(h) if dy >= 0 else range(h - 1, -1, -1)
    for y in ys:
        for x in xs:
            at(x, y)
    return np.array([[L[(x, y)] for x in range(w)] for y in range(h)], np.int64)


def random_volume(h, w, planes, seed):
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, 255, (h, w, planes), dtype=np.uint8)
    vol[rng.uniform(size=vol.shape) < 0.15] = 255
    if h * w > 4:
        vol[h // 2, w // 2, :] = 255                         # a pixel without a valid plane
    vol[0, 0, 0], vol[h - 1, w - 1, planes - 1] = 255, 17
    return vol


SHAPES = [(1, 1, 2), (1, 9, 3), (7, 1, 5), (5, 8, 64), (8, 5, 17)]


@pytest.mark.parametrize('paths', [4, 8])
@pytest.mark.parametrize('p1, p2', [(0, 40), (24, 24), (8, 255)])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_restatement_against_the_loop(shape, p1, p2, paths):
    vol = random_volume(*shape, seed=sum(shape) + p1)
    assert (vol == 255).any() and (vol < 255).any()
    want = np.zeros(shape, np.int64)
    for r in ds.DIRECTIONS[:paths]:
        one = loop_path_cost(vol, r, p1, p2, 99)
        assert np.array_equal(ds.path_cost(vol, r, p1, p2, 99), one), r
        want += one
    got = ds.aggregate(vol, paths, p1, p2, 99)
    assert got.dtype == np.uint16 and np.array_equal(got, want)


# ---- properties ----
def _select(vol, T, max_cost=254):
    return ds.select(T, vol, dc.W_FAR, dr.plane_step(dc.W_FAR, dc.W_NEAR, vol.shape[2]), max_cost)


@pytest.mark.parametrize('paths', [4, 8])
def test_one_plane_everywhere(paths):
    """C = 40 at plane 4 and 90 elsewhere, at every pixel, P1 = 10, P2 = 30.  A path starts with L = C.
    One step on m = 40: L(4) = 40 + min(40, ...) - 40 = 40; L(3) = L(5) = 90 + min(90, 40 + P1, 40 + P2)
    - 40 = 100; every other plane 90 + min(90, 90 + P1, 40 + P2) - 40 = 120, and these values repeat from
    there on.  So T(4) = 40 paths is the minimum everywhere, 90 paths <= T(d) <= 120 paths elsewhere,
    T_m = T_p by symmetry, off = 0 and the depth is plane 4's own."""
    h, w, planes = 6, 7, 9
    vol = np.full((h, w, planes), 90, np.uint8)
    vol[:, :, 4] = 40
    T = ds.aggregate(vol, paths, 10, 30, 127)
    assert (T[:, :, 4] == 40 * paths).all()
    assert (T[0, 0, [0, 8]] >= 90 * paths).all() and T.max() <= 120 * paths
    plane, cost, tot0, depth = _select(vol, T)
    assert (plane == 4).all() and (cost == 40).all() and (tot0 == 40 * paths).all()
    step = dr.plane_step(dc.W_FAR, dc.W_NEAR, planes)
    assert np.array_equal(dc.bits(depth), dc.bits(np.full((h, w), 1.0 / (dc.W_FAR + 4 * step), np.float32)))


@pytest.mark.parametrize('paths', [4, 8])
def test_all_invalid_volume(paths):
    vol = np.full((5, 6, 7), 255, np.uint8)
    T = ds.aggregate(vol, paths, 8, 64, 100)
    assert (T == paths * 100).all()
    plane, cost, tot0, depth = _select(vol, T)
    assert (plane == 0).all() and (cost == 255).all() and (tot0 == paths * 100).all()
    assert np.array_equal(dc.bits(depth), np.full((5, 6), 0x7fc00000, np.uint32))


def test_no_penalty_is_the_raw_argmin():
    """P1 = P2 = 0: min(..., m + 0) - m = 0, so L_r = C' on every path and T = paths C'"""
    vol = random_volume(9, 11, 13, seed=4)
    for paths in (4, 8):
        T = ds.aggregate(vol, paths, 0, 0, 127)
        Cw = np.where(vol == 255, 127, vol).astype(np.int64)
        assert np.array_equal(T, paths * Cw)
        plane = _select(vol, T)[0]
        low = Cw.min(axis=2, keepdims=True)
        unique = (Cw == low).sum(axis=2) == 1
        assert unique.sum() > 50 and np.array_equal(plane[unique], Cw.argmin(axis=2)[unique])


@pytest.mark.parametrize('p2', [0, 64, 255])
def test_total_stays_in_its_bound(p2):
    rng = np.random.default_rng(8)
    vol = rng.choice(np.array([0, 254, 255], np.uint8), (12, 10, 16))
    for paths in (4, 8):
        T = ds.aggregate(vol, paths, min(p2, 8), p2, 254)
        assert int(T.max()) <= paths * (254 + p2) <= 4072 and T.dtype == np.uint16


def test_select_rule():
    """ties to the smallest plane; best at an end: off = 0; the raw cost decides what is kept.  (With the
    smallest plane winning a tie, T_m > T_0 at an inner winner, so den > 0 there: den = 0 cannot be
    reached from a total; the kernel's branch for it is the rule's.)"""
    planes = 5
    step = dr.plane_step(dc.W_FAR, dc.W_NEAR, planes)
    T = np.array([[[7, 3, 3, 9, 9],        # a tie: plane 1; den = (7 - 6) + 3 = 4, off = (7 - 3) / 8 = 0.5
                   [2, 5, 5, 5, 5],        # best at plane 0
                   [9, 9, 9, 9, 1],        # best at the last plane
                   [4, 4, 4, 4, 4],        # all equal: plane 0
                   [9, 4, 4, 4, 9],        # best 1, den = (9 - 8) + 4 = 5 > 0
                   [5, 5, 3, 5, 5]]],      # den = 4, off = 0
                 np.uint16)
    vol = np.full(T.shape, 10, np.uint8)
    vol[0, 4, 1] = 255                     # the winner of pixel 4 was never measured
    vol[0, 5, 2] = 52
    plane, cost, tot0, depth = ds.select(T, vol, dc.W_FAR, step, 51)
    assert plane.tolist() == [[1, 0, 4, 0, 1, 2]] and tot0.tolist() == [[3, 2, 1, 4, 4, 3]]
    assert cost.tolist() == [[10, 10, 10, 10, 255, 52]]
    off = [0.5, 0.0, 0.0, 0.0]
    want = [np.float32(1.0 / (dc.W_FAR + (b + o) * step)) for b, o in zip([1, 0, 4, 0], off)]
    assert np.array_equal(dc.bits(depth[0, :4]), dc.bits(np.array(want, np.float32)))
    assert np.isnan(depth[0, 4]) and np.isnan(depth[0, 5])
    assert not np.isnan(ds.select(T, vol, dc.W_FAR, step, 52)[3][0, 5])
    assert ds.max_cost_of(0.6) == dense.sgm_max_cost(0.6) == 51 and dense.sgm_max_cost(1.0) == 0
    assert dense.sgm_max_cost(-1.0) == 254 and dense.sgm_max_cost(-3.0) == 254


def test_cost_formula():
    S = np.array([1.0, 0.0, -1.0, 1.5, -2.0, np.nan, 0.5, -0.5, 0.6, 0.515625], np.float32)
    # 0.5 127 = 63.5 -> 64 and 1.5 127 = 190.5 -> 190: half goes to even; the clamp comes after the rounding
    assert ds.cost_of(S).tolist() == [0, 127, 254, 0, 254, 255, 64, 190, 51, 62]


# ---- quality against winner-take-all ----
# measured by the restatement (13 planes, r = 3, 8 paths, P1 = 16, P2 = 128): share of the kept pixels
# within one plane step / kept pixels, winner-take-all -> semi-global
#   slope       0.9996 / 2432 -> 1.0000 / 2432        roof       0.9893 / 2422 -> 0.9913 / 2421
#   hard-slope  0.9855 / 1515 -> 0.9974 / 1529        hard-roof  0.9746 / 1455 -> 0.9939 / 1469
# the margin asserted on a hard scene is half of the gain measured there
MARGIN = {'slope': 0.0, 'roof': 0.0, 'hard-slope': 0.5 * (0.9974 - 0.9855), 'hard-roof': 0.5 * (0.9939 - 0.9746)}
CLEAN = {'hard-slope': 0.9996, 'hard-roof': 0.9893}


@pytest.mark.parametrize('name', sc.INPUTS)
def test_sgm_is_no_worse_than_winner_take_all(name):
    S, truth = sc.scores(name)
    wta_plane, _score, wta_depth = ds.winner_of_scores(S, dc.W_FAR, dc.W_NEAR)
    if not name.startswith('hard-'):                      # the shared stack gives dr.sweep's winner
        views, _ = dc.scene(name)
        ref = dr.sweep(views[0], views[1:], dc.W_FAR, dc.W_NEAR, dc.PLANES, radius=sc.RADIUS)
        assert np.array_equal(ref[0], wta_plane) and np.array_equal(dc.bits(ref[2]), dc.bits(wta_depth))
    plane, cost, total, depth = ds.sgm_of_scores(S, dc.W_FAR, dc.W_NEAR, p1=dense.SGM_P1, p2=dense.SGM_P2)
    wta, wta_kept = sc.quality(wta_depth, truth)
    sgm, sgm_kept = sc.quality(depth, truth)
    print('%s: within a step %.4f of %d kept (winner-take-all) -> %.4f of %d kept (semi-global)'
          % (name, wta, wta_kept, sgm, sgm_kept))
    if name in CLEAN:
        assert wta <= CLEAN[name] - 0.01                  # the hard scene is hard for winner-take-all
    assert sgm >= wta + MARGIN[name]
    assert sgm_kept >= 0.9 * wta_kept
    assert (plane >= 0).all() and not np.isfinite(depth[cost > ds.max_cost_of(0.6)]).any()


# ---- argument checks: a ValueError before any device call (there is no device here) ----
def test_argument_checks():
    views, _ = dc.scene('slope')
    nb, ranges = [[1], [0], [0], [0]], [(60.0, 140.0)] * 4
    for bad in (dict(planes=1), dict(planes=65), dict(paths=6), dict(p1=9, p2=8), dict(p2=256), dict(p1=-1),
                dict(c_invalid=255), dict(c_invalid=-1)):
        with pytest.raises(ValueError):
            dense.depth_maps(views, nb, ranges, **dict(dict(planes=13, regularize='sgm'), **bad))
    with pytest.raises(ValueError, match='regularize'):
        dense.depth_maps(views, nb, ranges, planes=13, regularize='semi')
    vol = np.zeros((4, 5, 13), np.uint8)
    for bad in (dict(paths=6), dict(p1=9, p2=8), dict(c_invalid=255), dict(direction=8)):
        with pytest.raises(ValueError):
            kernels.dense_sgm_paths(vol, **bad)
    for shape in ((4, 5, 1), (4, 5, 65), (4, 5)):
        with pytest.raises(ValueError):
            kernels.dense_sgm_paths(np.zeros(shape, np.uint8))
    with pytest.raises(ValueError):
        kernels.dense_sgm_select(np.zeros((4, 5, 12), np.uint16), vol, dc.W_FAR, dc.W_NEAR, 51)
    with pytest.raises(ValueError):
        kernels.dense_sgm_select(np.zeros(vol.shape, np.uint16), vol, dc.W_FAR, dc.W_NEAR, 255)
    with pytest.raises(ValueError):
        kernels.dense_sgm_select(np.zeros(vol.shape, np.uint16), vol, dc.W_NEAR, dc.W_FAR, 51)
    ref, nbs = views[0], views[1:]
    for planes in (1, 65):
        with pytest.raises(ValueError, match='semi-global'):
            kernels.dense_sweep(ref, nbs, dc.W_FAR, dc.W_NEAR, planes, volume=vol)
    assert dense.sgm_parameters(64, 'sgm') == (64, 8, dense.SGM_P1, dense.SGM_P2, 127)
    assert dense.sgm_parameters(4096, 'none', p1=9, p2=8) is None          # (not read without the mode)


def test_entry_points_check_their_arguments_without_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    one = _lib.c_void_p(16)                                 # (never dereferenced: every call below is refused)
    assert L.iamx_dense_sgm_paths(one, 4, 4, 65, 8, 8, 64, 127, one, None) == -1
    assert L.iamx_dense_sgm_paths(one, 4, 4, 1, 8, 8, 64, 127, one, None) == -1
    assert L.iamx_dense_sgm_paths(one, 4, 4, 8, 6, 8, 64, 127, one, None) == -1
    assert L.iamx_dense_sgm_paths(one, 4, 4, 8, 8, 65, 64, 127, one, None) == -1
    assert L.iamx_dense_sgm_paths(one, 4, 4, 8, 8, 8, 64, 255, one, None) == -1
    assert L.iamx_dense_sgm_paths(None, 4, 4, 8, 8, 8, 64, 127, one, None) == -1
    assert L.iamx_dense_sgm_direction(one, 4, 4, 8, 8, 0, 8, 64, 127, one, None) == -1
    assert L.iamx_dense_sgm_select(one, one, 4, 4, 8, 0.01, 0.001, 255, one, one, one, one, None) == -1
    assert L.iamx_dense_sgm_select(one, one, 4, 4, 8, 0.01, 0.001, 51, one, one, one, None, None) == -1
    assert L.iamx_dense_sweep_volume(one, one, one, one, one, 4, 4, 1, 65, 0.01, 0.02, 3, 4.0, 0.6, one, one, one, one,
                                     one, None) == -1
    assert L.iamx_dense_sweep_volume(one, one, one, one, one, 4, 4, 1, 8, 0.01, 0.02, 3, 4.0, 0.6, one, one, one, one,
                                     None, None) == -1
