"""Host: the restatement the kernels of csrc/chain_surface.hip are held to (tests/surface_cull_restatement.py)
against scipy's cKDTree and np.polyfit and on a planted scene, and the Python layer of the 4c twins
(observation table, weak images, mark order, marking on list and array chains) with the device calls
replaced by the restatement.  No GPU."""
import importlib.util
import os
import pickle

import numpy as np
import pytest

import chain_tools_common as ct
import surface_cull_restatement as sr


def _project(cam, names=None):
    from imageanalysis_amd.hostlib.image_pose import PoseProject
    names = names or ['IMG_%02d' % i for i in range(len(cam))]
    proj = PoseProject(names)
    for im, p in zip(proj.image_list, cam):
        im.set_camera_pose([float(v) for v in p], 0.0, 0.0, 0.0)
        im.set_camera_pose([float(v) for v in p], 0.0, 0.0, 0.0, opt=True)
    return proj, [names]


def _rows(matches):
    """plain lists of list chains or of a Chains, without touching the Chains"""
    return pickle.loads(pickle.dumps(matches))


def _in_group(proj, group_list, group_index):
    names = set(group_list[group_index])
    return np.array([im.name in names for im in proj.image_list], np.uint8)


@pytest.fixture(scope='module')
def scene():
    return sr.planted_scene()


@pytest.fixture(scope='module')
def scene_rounds(scene):
    matches, cam, _planted = scene
    return sr.cull_surface(matches, np.ones(len(cam), np.uint8), 0)


# ---------------------------------------------------------------------------------------------
# the restatement against scipy and numpy
# ---------------------------------------------------------------------------------------------
def test_neighbour_sets_equal_ckdtree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(11)
    for n, k in ((200, 30), (31, 30), (12, 30), (50, 5)):
        uv = rng.uniform(0, 4000, (n, 2))
        tree = cKDTree(uv)
        for i in range(n):
            idx, d2 = sr.neighbours(uv, i, min(k, n))
            assert np.all(np.diff(d2) > 0)                       # no ties in this input
            dist, want = tree.query(uv[i], k=min(k, n))
            assert idx.tolist() == np.atleast_1d(want).tolist(), (n, i)
            assert np.allclose(np.sqrt(d2), np.atleast_1d(dist), rtol=1e-12, atol=0)


def test_line_equals_polyfit():
    rng = np.random.default_rng(12)
    worst = 0.0
    for m in (2, 3, 11, 22, 30):
        for _ in range(20):
            x = np.concatenate([np.zeros(rng.integers(1, 4)), rng.uniform(1, 300, m)])
            y = 0.03 * x + rng.normal(0, 0.2, len(x)) + 0.5
            a, b = sr.line(x.tolist(), y.tolist())
            z = np.polyfit(x, y, 1)
            worst = max(worst, abs(a - z[0]) / abs(z[0]), abs(b - z[1]) / abs(z[1]))
    print('worst relative difference to np.polyfit: %.3g' % worst)
    assert worst <= 1e-9
    assert sr.line([0.0, 0.0, 0.0], [0.0, 1.0, 2.0]) is None     # no neighbour at a distance


def test_walk_is_the_references_double_loop():
    d2 = np.array([0.0] * 12 + list(range(1, 19)), np.float64)   # 12 duplicates, 18 positives listed
    assert sr.walk(d2, 10) == 22                                 # stops in front of the eleventh positive
    assert sr.walk(np.array([0.0] + list(range(1, 11)), np.float64), 10) == 11     # ends with the list
    assert sr.walk(np.zeros(30), 10) == 30
    assert sr.walk(np.array([0.0, 1.0, 2.0, 3.0]), 2) == 3


def test_planted_scene_culls_the_planted_chains_and_stops(scene, scene_rounds):
    """12 nadir cameras on a 3 x 4 grid at 100 m, 600 ground points, 6 chains displaced vertically by
    15 .. 40 m.  (default_rng(7) of this generator culls one unplanted chain in its second round at
    5 deviations; the seed was changed, not the margin.)"""
    matches, cam, planted = scene
    assert len(cam) == 12 and len(planted) == 6
    for r in scene_rounds:
        print('culled %d, average %.4f, deviation %.4f, margin %.3g' % (len(r['culled']), r['average'],
                                                                         r['stddev'], r['margin']))
        assert r['margin'] >= 1e-6
    assert [len(r['culled']) for r in scene_rounds] == [5, 1, 0]
    assert sorted(c for r in scene_rounds for c in r['culled']) == planted
    assert all(r['n_small'] == 0 and r['n_flat'] == 0 and r['n_uncounted'] == 0 for r in scene_rounds)


# ---------------------------------------------------------------------------------------------
# the observation table and the weak-image rule (host code of the package)
# ---------------------------------------------------------------------------------------------
def _mixed_chains(scene):
    """the planted scene with another group's chain, an ungrouped one, a member outside the group"""
    matches, cam, _ = scene
    rows = _rows(matches[:200])
    rows.append([[1.0, 2.0, 3.0], 1, [0, [5.0, 6.0]], [1, [7.0, 8.0]]])
    rows.append([None, -1, [2, [5.0, 6.0]], [3, [7.0, 8.0]]])
    rows[3].append([12, [100.0, 200.0]])                         # image 12 is not in the group
    cam = np.concatenate([cam, [[500.0, 500.0, -100.0]]])
    return rows, cam


@pytest.mark.parametrize('as_arrays', [False, True], ids=['lists', 'chains'])
def test_observation_table_equals_restatement(scene, as_arrays):
    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd.match_cleanup import Chains
    rows, cam = _mixed_chains(scene)
    proj, group_list = _project(cam)
    group_list = [group_list[0][:12], group_list[0][12:]]
    in_group = _in_group(proj, group_list, 0)
    alive = np.ones(len(rows), bool)
    alive[[5, 17]] = False
    matches = Chains.from_lists(_rows(rows)) if as_arrays else rows
    for min_members, chains in ((1, None), (2, sr.depth_chains(rows, in_group, 0))):
        t = cull.observation_table(proj, matches, group_list, 0, alive if chains is None else None, min_members)
        want = sr.observation_table(rows, in_group, 0, alive if chains is None else None, chains)
        for got, ref in zip((t.img_ptr, t.uv, t.ned, t.chain, t.chain_ptr, t.chain_obs), want):
            assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes()
        looked = np.zeros(len(rows), bool)
        looked[chains if chains is not None else sr.looked_at(rows, 0, alive)] = True
        assert np.array_equal(t.looked, looked)
    assert not as_arrays or matches.untouched()
    assert t.img_ptr[12] == t.img_ptr[13]                        # nothing of the image outside the group


def test_observation_table_error_paths(scene):
    from imageanalysis_amd import match_culling as cull
    rows, cam = _mixed_chains(scene)
    proj, group_list = _project(cam)
    with pytest.raises(IndexError, match='group 2 of 1'):
        cull.observation_table(proj, rows, group_list, 2)
    bad = _rows(rows)
    bad[7][3][0] = 13
    with pytest.raises(IndexError, match='chain 7 refers to image 13, the project has 13 images'):
        cull.observation_table(proj, bad, group_list, 0)
    bad = _rows(rows)
    bad[9][2][0] = -1
    with pytest.raises(IndexError, match='chain 9 refers to image -1'):
        cull.observation_table(proj, bad, group_list, 0)
    bad = _rows(rows)
    bad[-2][2][0] = 10 ** 6                                      # another group's chain is never looked at
    cull.observation_table(proj, bad, group_list, 0)
    bad = _rows(rows)
    bad[11][0] = None
    with pytest.raises(ValueError, match='chain 11 of group 0 has no position'):
        cull.observation_table(proj, bad, group_list, 0)
    alive = np.ones(len(bad), bool)
    alive[11] = False                                            # ... unless it is not alive
    cull.observation_table(proj, bad, group_list, 0, alive)


@pytest.mark.parametrize('min_features', [25, 3, 1])
def test_weak_images_list_and_array_paths_agree(scene, min_features):
    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd.match_cleanup import Chains
    matches, cam, _ = scene
    rows = _rows(matches[:40]) + [[[0.0, 0.0, 0.0], 0, [12, [1.0, 2.0]], [13, [3.0, 4.0]], [0, [5.0, 6.0]]]]
    chains = Chains.from_lists(_rows(rows))
    for marks in ([], [[0, 1], [40, 0], [7, 0]]):
        for c, j in marks:
            cull.mark_feature(rows, c, j, '-', quiet=True)
            cull.mark_feature(chains, c, j, '-', quiet=True)
        want = sr.weak_images(rows, 14, min_features)
        assert cull.weak_images(rows, 14, min_features) == want
        assert cull.weak_images(chains, 14, min_features) == want and chains.untouched()
        if min_features == 25 and not marks:
            assert [40, 0] in want and [40, 1] in want           # images 12 and 13 hold one member each
        if min_features == 1:
            assert want == []
    with pytest.raises(IndexError):
        cull.weak_images(rows, 12, min_features)
    with pytest.raises(IndexError):
        cull.weak_images(chains, 12, min_features)


# ---------------------------------------------------------------------------------------------
# the loops and the mark order, the device calls replaced by the restatement
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    from imageanalysis_amd import match_culling as cull

    def surface_consistency(proj, matches, group_list, group_index, k=30, positives=10, alive=None):
        rows = _rows(matches)
        img_ptr, uv, ned, chain, _cp, _co = sr.observation_table(rows, _in_group(proj, group_list, group_index),
                                                                 group_index, alive)
        tgt, val, _used, _fit, status = sr.knn_fit(img_ptr, uv, ned, chain, k, positives)
        _total, count, metric = sr.chain_metric(tgt, val, len(rows))
        looked = np.zeros(len(rows), bool)
        looked[sr.looked_at(rows, group_index, alive)] = True
        return cull.SurfaceReport(metric=metric, count=count, looked=looked, table=None,
                                  n_small=int(np.sum(status == sr.SKIPPED_SMALL)),
                                  n_flat=int(np.sum(status == sr.SKIPPED_FLAT)),
                                  n_uncounted=int(np.sum(looked & (count == 0))), n_looked=int(looked.sum()))

    def outlier_stats(metric, looked, factor, two_sided):
        average, dev, flag, _margin = sr.outlier_stats(metric, looked, factor, two_sided)
        idx = np.nonzero(flag)[0]
        return idx.astype(np.int64), np.asarray(metric)[idx], average, dev

    def chain_depths(proj, matches, group_list, group_index):
        rows = _rows(matches)
        in_group = _in_group(proj, group_list, group_index)
        pos = np.array([im.get_camera_pose(opt=True)[0] for im in proj.image_list])
        img_ptr, _uv, ned, _chain, chain_ptr, chain_obs = sr.observation_table(
            rows, in_group, group_index, chains=sr.depth_chains(rows, in_group, group_index))
        _depth, z, metric, looked = sr.chain_depths(img_ptr, ned, pos, chain_ptr, chain_obs)
        return cull.DepthReport(metric=metric, looked=looked, z=z, table=None)

    monkeypatch.setattr(cull, 'surface_consistency', surface_consistency)
    monkeypatch.setattr(cull, 'outlier_stats', outlier_stats)
    monkeypatch.setattr(cull, 'chain_depths', chain_depths)
    return cull


@pytest.mark.parametrize('as_arrays', [False, True], ids=['lists', 'chains'])
def test_cull_surface_marks_whole_chains(stubbed, scene, scene_rounds, as_arrays, capsys):
    from imageanalysis_amd.match_cleanup import Chains
    matches, cam, planted = scene
    proj, group_list = _project(cam)
    work = Chains.from_lists(_rows(matches)) if as_arrays else _rows(matches)
    rounds = stubbed.cull_surface(proj, work, group_list, 0)
    assert rounds == [r['culled'] for r in scene_rounds]
    out = capsys.readouterr().out
    assert out.count('culled') == 3 and 'outlier - match index' not in out      # a line per round, none per chain
    if as_arrays:
        assert work.untouched()
        for c in range(len(matches)):
            assert work.marked[work.ptr[c]:work.ptr[c + 1]].all() == (c in planted)
    else:
        for c, m in enumerate(work):
            assert (m[2:] == [[-1, -1]] * (len(m) - 2)) == (c in planted)
    stubbed.delete_marked_features(work, 3)
    assert _rows(work) == [m for c, m in enumerate(matches) if c not in planted]
    # max_rounds ends the loop early: only the first round's chains go
    work = _rows(matches)
    assert stubbed.cull_surface(proj, work, group_list, 0, max_rounds=1) == [scene_rounds[0]['culled']]


def test_surface_outliers_order(stubbed):
    metric = np.array([1.0, 50.0, 1.1, -50.0, 0.9, 50.0, 1.0, 1.0, 70.0] + [1.0] * 60)
    looked = np.ones(len(metric), bool)
    looked[8] = False
    report = stubbed.SurfaceReport(metric=metric, looked=looked)
    idx, average, dev = stubbed.surface_outliers(report, 3)
    assert idx.tolist() == [1, 3, 5]                             # descending |metric|, ties in chain order
    want = sr.outlier_stats(metric, looked, 3, True)
    assert (average, dev) == want[:2]


@pytest.mark.parametrize('as_arrays', [False, True], ids=['lists', 'chains'])
def test_depth_outliers_mark_order(stubbed, scene, as_arrays, capsys):
    from imageanalysis_amd.match_cleanup import Chains
    matches, cam, planted = scene
    proj, group_list = _project(cam)
    work = Chains.from_lists(_rows(matches)) if as_arrays else _rows(matches)
    marks, rows = stubbed.depth_outliers(proj, work, group_list, 0, 3)
    want, z, average, dev, margin = sr.depth_outliers(matches, np.ones(12, np.uint8), 0, cam, 3)
    assert margin >= 1e-6
    # (one-sided at 3 deviations the depth rule finds the larger of the planted displacements)
    assert marks == want and len(marks) >= 3 and set(m[0] for m in marks) <= set(planted) and all(m[1] == 0 for m in marks)
    assert rows == [(im.name, int(r[2]), float(r[0]), float(r[1])) for im, r in zip(proj.image_list, z)]
    assert 'mean = %.4f stddev = %.4f' % (average, dev) in capsys.readouterr().out
    stubbed.mark_using_list(marks, work)
    stubbed.delete_marked_features(work, 3)                      # pair-wise chains: one mark removes the chain
    assert _rows(work) == [m for c, m in enumerate(matches) if c not in set(k[0] for k in marks)]
    assert not as_arrays or work.untouched()


def test_depth_rows_of_an_image_without_depths(stubbed, scene):
    matches, cam, _ = scene
    cam = np.concatenate([cam, [[900.0, 900.0, -100.0]]])
    proj, group_list = _project(cam)
    _marks, rows = stubbed.depth_outliers(proj, _rows(matches[:100]), group_list, 0, 3)
    assert rows[12] == ('IMG_12', 0, None, None)


# ---------------------------------------------------------------------------------------------
# the scripts' arguments
# ---------------------------------------------------------------------------------------------
def _script(name):
    path = os.path.join(ct.REPO, 'imageanalysis_amd', 'scripts', name)
    spec = importlib.util.spec_from_file_location(name.replace('-', '_').replace('.py', ''), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                 # (lib.* is imported by main() only)
    return mod


def test_script_arguments():
    a = _script('4c-surface-outliers.py').parse_args(['PROJ'])
    assert (a.project, a.group, a.stddev, a.neighbors, a.positives, a.max_rounds) == ('PROJ', 0, 5, 30, 10, None)
    a = _script('4c-surface-outliers.py').parse_args(['P', '--group', '1', '--stddev', '4.5', '--neighbors', '20',
                                                      '--positives', '8', '--max-rounds', '2'])
    assert (a.group, a.stddev, a.neighbors, a.positives, a.max_rounds) == (1, 4.5, 20, 8, 2)
    for flag in ('--show', '--checkpoint'):
        with pytest.raises(SystemExit):
            _script('4c-surface-outliers.py').parse_args(['P', flag])
    b = _script('4c-by-depth.py').parse_args(['PROJ'])
    assert (b.project, b.group, b.stddev, b.strong, b.min_features, b.interactive) == ('PROJ', 0, 3, False, 25, False)
    b = _script('4c-by-depth.py').parse_args(['P', '--group', '1', '--stddev', '2', '--strong', '--min-features', '0',
                                              '--interactive'])
    assert (b.group, b.stddev, b.strong, b.min_features, b.interactive) == (1, 2.0, True, 0, True)
