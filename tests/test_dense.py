"""CPU: the dense-surface rules do stereo (the numpy restatement against the scenes' true depths), the
host logic of imageanalysis_amd/dense.py against brute-force loops, and the argument checks."""
import numpy as np
import pytest

import dense_common as dc
import dense_restatement as dr
from imageanalysis_amd import dense, kernels


@pytest.fixture(scope='module')
def swept():
    out = {}
    for surface in ('slope', 'roof'):
        views, truth = dc.scene(surface)
        out[surface] = (dr.sweep(views[0], views[1:], dc.W_FAR, dc.W_NEAR, dc.PLANES, radius=3), truth[0])
    return out


@pytest.mark.parametrize('surface, share', [('slope', 0.99), ('roof', 0.93)])
def test_the_rules_find_the_surface(swept, surface, share):
    """Of the kept pixels, the share within one plane step of the true inverse depth; of the interior
    pixels, the share kept.  Measured by this restatement (13 planes, r = 3): slope 0.9996 within a step,
    median error 0.064 steps, 2432 of 2436 interior pixels kept; roof 0.9893, 0.087 steps, 2422."""
    (plane, score, depth, around), truth = swept[surface]
    step = dr.plane_step(dc.W_FAR, dc.W_NEAR, dc.PLANES)
    inside = dc.interior(dc.H, dc.W, 3)
    kept = ~np.isnan(depth)
    assert not kept[~inside].any()
    err = np.abs(1.0 / depth[kept].astype(np.float64) - 1.0 / truth[kept])
    within = float((err <= step).mean())
    print('%s: within a step %.4f, median %.3f steps, kept %d of %d interior pixels'
          % (surface, within, float(np.median(err)) / step, int(kept.sum()), int(inside.sum())))
    assert within >= share
    assert kept.sum() >= 0.9 * inside.sum()


def test_restatement_outputs_hang_together(swept):
    (plane, score, depth, around), _ = swept['roof']
    assert plane.dtype == np.int32 and score.dtype == depth.dtype == around.dtype == np.float32
    assert np.array_equal(dc.bits(score), dc.bits(around[:, :, 1]))
    assert np.array_equal(plane < 0, np.isnan(score))
    with np.errstate(invalid='ignore'):
        assert not (around[:, :, 0] > score).any() and not (around[:, :, 2] > score).any()
    assert np.isnan(around[:, :, 0][plane == 0]).all() and np.isnan(around[:, :, 2][plane == dc.PLANES - 1]).all()


# ---- host logic on a stand-in project ----
def _stand_in(seed=5, n_img=9, n_chains=400):
    rng = np.random.default_rng(seed)
    poses = []
    for k in range(n_img):
        C = np.array([25.0 * (k // 3) + rng.normal(0, 2), 30.0 * (k % 3) + rng.normal(0, 2), -100.0 + rng.normal(0, 3)])
        poses.append((dc._rot(*rng.uniform(-0.05, 0.05, 3)).dot(dc.NADIR), C))
    group = [7, 3, 11, 4, 0, 9, 12, 5, 2]                  # project indices, group order
    matches = []
    for c in range(n_chains):
        X = [rng.uniform(-40, 90), rng.uniform(-40, 100), rng.normal(0, 4)]
        near = sorted(range(n_img), key=lambda k: np.hypot(poses[k][1][0] - X[0], poses[k][1][1] - X[1]))
        members = [group[k] for k in near[:rng.integers(2, 6)]]
        if c % 17 == 0:
            members.append(99)                              # an image outside the group
        if c % 23 == 0:
            members.append(members[0])                      # a repeated member counts once
        m = [None if c % 13 == 0 else X, 0] + [[i, [0.0, 0.0]] for i in members]
        matches.append(m)
    matches.append([[0.0, 0.0, -500.0], 0, [group[0], [0, 0]], [group[1], [0, 0]]])      # behind the cameras
    return matches, group, poses


def _brute_neighbours(matches, group, poses, n):
    V = len(group)
    out = []
    for i in range(V):
        cand = []
        for j in range(V):
            if j == i:
                continue
            depths = []
            for m in matches:
                imgs = set(p[0] for p in m[2:])
                if m[0] is not None and group[i] in imgs and group[j] in imgs:
                    d = np.asarray(m[0], float) - poses[i][1]
                    R = poses[i][0]
                    depths.append((R[2, 0] * d[0] + R[2, 1] * d[1]) + R[2, 2] * d[2])
            if not depths:
                continue
            depths.sort()
            k = len(depths)
            med = 0.5 * (depths[(k - 1) // 2] + depths[k // 2])
            d = poses[i][1] - poses[j][1]
            base = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if med > 0 and dense.NEIGHBOUR_RATIO[0] <= base / med <= dense.NEIGHBOUR_RATIO[1]:
                cand.append((-k, j))
        out.append([j for _, j in sorted(cand)[:n]])
    return out


@pytest.mark.parametrize('n', [1, 4, 8])
def test_choose_neighbours_against_brute_force(n):
    matches, group, poses = _stand_in()
    got = dense.choose_neighbours(matches, group, poses, n=n)
    want = _brute_neighbours(matches, group, poses, n)
    assert got == want
    assert any(len(x) == n for x in got) and all(i not in x for i, x in enumerate(got))


def test_choose_neighbours_keeps_the_ratio_band():
    matches, group, poses = _stand_in()
    far = [(R, C * np.array([20.0, 20.0, 1.0])) for R, C in poses]       # baselines far above 0.6 depths
    assert dense.choose_neighbours(matches, group, far, n=4) == _brute_neighbours(matches, group, far, 4)
    same = [(R, poses[0][1]) for R, _ in poses]                          # no baseline at all
    assert dense.choose_neighbours(matches, group, same, n=4) == [[] for _ in group]
    assert dense.choose_neighbours([], group, poses) == [[] for _ in group]


def test_depth_range_against_brute_force():
    matches, group, poses = _stand_in()
    got = dense.depth_range(matches, group, poses)
    for k, g in enumerate(group):
        zs = []
        for m in matches:
            if m[0] is not None and g in set(p[0] for p in m[2:]):
                d = np.asarray(m[0], float) - poses[k][1]
                R = poses[k][0]
                z = (R[2, 0] * d[0] + R[2, 1] * d[1]) + R[2, 2] * d[2]
                if z > 0:
                    zs.append(z)
        assert got[k] == (0.9 * min(zs), 1.1 * max(zs))
    assert dense.depth_range([[None, 0, [group[0], [0, 0]]]], group, poses) == [None] * len(group)


def test_frame_and_ply():
    x0, y1, W, H = dense.frame_of(-3.2, 7.9, 1.1, 5.0, 0.5)
    assert (x0, y1, W, H) == (-3.5, 5.0, 23, 8)
    with pytest.raises(ValueError):
        dense.frame_of(0, 1, 0, 1, 0.0)
    blob = dense.ply_bytes(np.array([[1, 2, 3], [4, 5, 6]], np.float32), [7, 8])
    head, body = blob.split(b'end_header\n')
    assert b'element vertex 2' in head and b'binary_little_endian' in head and len(body) == 2 * 13
    assert np.frombuffer(body[:12], '<f4').tolist() == [1.0, 2.0, 3.0] and body[12] == 7
    K = dense.scaled_K(np.array([[800.0, 0, 319.5], [0, 800.0, 239.5], [0, 0, 1]]), 640, 480, 80, 60)
    assert np.allclose(K, [100.0, 100.0, 39.5, 29.5])


# ---- argument checks: a ValueError before any device call (there is no device here) ----
def test_argument_checks():
    views, _ = dc.scene('slope')
    ref, nbs = views[0], views[1:]
    ok = dict(w_far=dc.W_FAR, w_near=dc.W_NEAR, planes=13)
    for bad in (dict(planes=0), dict(radius=0), dict(radius=8), dict(w_near=dc.W_FAR), dict(w_near=dc.W_FAR / 2)):
        with pytest.raises(ValueError):
            kernels.dense_sweep(ref, nbs, **dict(ok, **bad))
    small, _ = dc.make_view('slope', 1, h=29, w=37)
    with pytest.raises(ValueError, match='one size'):
        kernels.dense_sweep(ref, [nbs[0], small], **ok)
    with pytest.raises(ValueError):
        kernels.dense_sweep(ref, [], **ok)
    with pytest.raises(ValueError):
        kernels.dense_check(np.zeros((4, dc.H, dc.W), np.float32), views, [[1], [0], [0]])
    with pytest.raises(ValueError):
        kernels.dense_check(np.zeros((4, dc.H, dc.W), np.float32), views, [[0], [0], [0], [0]])
    with pytest.raises(ValueError):
        kernels.dense_splat(np.zeros((3, 3)), None, 0.0, 0.0, 0.0, 4, 4)
    with pytest.raises(ValueError):
        dense.depth_maps(views, [[1]] * 4, [(60.0, 140.0)] * 3)
    with pytest.raises(ValueError):
        dense.depth_maps(views, [[1], [0], [0], [0]], [(140.0, 60.0)] * 4)
