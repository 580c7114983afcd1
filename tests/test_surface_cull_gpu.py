"""GPU: the kernels of csrc/chain_surface.hip through the C ABI against tests/surface_cull_restatement.py
(neighbour lists, walks and fits bit for bit; per-chain sums bit for bit; the statistics and the depth
means within 1e-12), then the Python layer and the two 4c script twins on a planted scene and on a
project built from a tests/golden/chain_colocated_* record."""
import ctypes
import json
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import chain_tools_common as ct
import surface_cull_restatement as sr

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device='cuda:0')


def abi_knn_fit(img_ptr, uv, ned, chain, k=30, n_pos=10):
    """-> tgt, val, used, fit, status; every output prefilled with a sentinel"""
    import torch
    from imageanalysis_amd import _lib
    n = len(chain)
    m = max(n, 1)
    d_in = [_dev(a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)) for a in (uv, ned, chain)]
    d_ptr = _dev(img_ptr)
    tgt, val = _full((m, k), -77, torch.int32), _full((m, k), -7.5, torch.float64)
    used, fit, status = _full((m,), -77, torch.int32), _full((m, 2), -7.5, torch.float64), _full((m,), -77, torch.int32)
    _lib.check(_lib.lib().iamx_surface_knn_fit(_p(d_ptr), _p(d_in[0]), _p(d_in[1]), _p(d_in[2]), len(img_ptr) - 1,
                                               n, k, n_pos, _p(tgt), _p(val), _p(used), _p(fit), _p(status),
                                               _lib.stream_ptr()), 'iamx_surface_knn_fit')
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (tgt, val, used, fit, status)]


def abi_chain_metric(tgt, val, status, looked, n_chains):
    """-> sum, count, metric, counters"""
    import torch
    from imageanalysis_amd import _lib
    n_obs, k = tgt.shape
    m = max(n_chains, 1)
    d_tgt, d_val, d_status = (_dev(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)) for a in (tgt, val, status))
    d_looked = _dev(looked.astype(np.uint8) if n_chains else np.zeros(1, np.uint8))
    total, count = _full((m,), -7.5, torch.float64), _full((m,), -77, torch.int32)
    metric, counters = _full((m,), -7.5, torch.float64), _full((4,), -77, torch.int64)
    off, order = _full((m + 1,), -1, torch.int64), _full((max(n_obs * k, 1),), -1, torch.int32)
    _lib.check(_lib.lib().iamx_surface_chain_metric(_p(d_tgt), _p(d_val), _p(d_status), n_obs, k, _p(d_looked),
                                                    n_chains, _p(total), _p(count), _p(metric), _p(counters),
                                                    _p(off), _p(order), _lib.stream_ptr()),
               'iamx_surface_chain_metric')
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (total, count, metric, counters)]


def abi_outlier_stats(metric, looked, factor, two_sided):
    """-> stats [4], flag, flagged chains, their metric"""
    import torch
    from imageanalysis_amd import _lib
    n = len(metric)
    tiles = (n + 255) // 256
    d_metric, d_looked = _dev(metric), _dev(looked.astype(np.uint8))
    stats, flag = _full((4,), -7.5, torch.float64), _full((n,), 9, torch.uint8)
    idx, sel, n_flagged = _full((n,), -77, torch.int32), _full((n,), -7.5, torch.float64), _full((1,), -77, torch.int64)
    part, cnt, off = _full((tiles,), -7.5, torch.float64), _full((tiles,), -77, torch.int32), _full((tiles + 1,), -77, torch.int64)
    _lib.check(_lib.lib().iamx_chain_outlier_stats(_p(d_metric), _p(d_looked), n, float(factor), int(two_sided),
                                                   _p(stats), _p(flag), _p(idx), _p(sel), _p(n_flagged), _p(part),
                                                   _p(cnt), _p(off), _lib.stream_ptr()), 'iamx_chain_outlier_stats')
    torch.cuda.synchronize()
    nf = int(n_flagged.item())
    assert np.all(idx.cpu().numpy()[nf:] == -77)                 # nothing is written past the count
    return stats.cpu().numpy(), flag.cpu().numpy(), idx.cpu().numpy()[:nf], sel.cpu().numpy()[:nf]


def abi_chain_depths(img_ptr, ned, pos, chain_ptr, chain_obs):
    import torch
    from imageanalysis_amd import _lib
    n_obs, n_img, n_chains = len(ned), len(img_ptr) - 1, len(chain_ptr) - 1
    d_ptr, d_ned, d_pos, d_cptr, d_cobs = (_dev(a) for a in (img_ptr, ned, pos, chain_ptr, chain_obs))
    depth, z = _full((n_obs,), -7.5, torch.float64), _full((n_img, 3), -7.5, torch.float64)
    metric, looked = _full((n_chains,), -7.5, torch.float64), _full((n_chains,), 9, torch.uint8)
    _lib.check(_lib.lib().iamx_chain_depths(_p(d_ptr), _p(d_ned), n_img, n_obs, _p(d_pos), _p(d_cptr), _p(d_cobs),
                                            n_chains, _p(depth), _p(z), _p(metric), _p(looked), _lib.stream_ptr()),
               'iamx_chain_depths')
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (depth, z, metric, looked)]


# ---------------------------------------------------------------------------------------------
# iamx_surface_knn_fit
# ---------------------------------------------------------------------------------------------
def _table(images, seed=1, n_chains=50):
    """images: one uv array [n, 2] per image -> img_ptr, uv, ned, chain with random positions / chains"""
    rng = np.random.default_rng(seed)
    img_ptr = np.zeros(len(images) + 1, np.int64)
    np.cumsum([len(u) for u in images], out=img_ptr[1:])
    uv = np.concatenate([np.asarray(u, np.float64).reshape(-1, 2) for u in images]) if images else np.zeros((0, 2))
    n = len(uv)
    ned = np.stack([uv[:, 1] * 0.03, uv[:, 0] * 0.03, np.zeros(n)], 1) + rng.normal(0, 0.5, (n, 3))
    return img_ptr, uv, ned, rng.integers(0, n_chains, n).astype(np.int32)


def _random_uv(n, seed):
    return np.random.default_rng(seed).uniform(0, 4000, (n, 2))


def _dup_image(n_dup, n_other, seed):
    uv = _random_uv(n_other + 1, seed)
    return np.random.default_rng(seed).permutation(np.concatenate([np.repeat(uv[:1], n_dup, 0), uv[1:]]))


KNN_CASES = {
    'sizes_0_1_2': (lambda: [_random_uv(0, 1), _random_uv(1, 2), _random_uv(2, 3)], 30, 10),
    'n3': (lambda: [_random_uv(3, 4)], 30, 10),
    'n29': (lambda: [_random_uv(29, 5)], 30, 10),
    'n30': (lambda: [_random_uv(30, 6)], 30, 10),
    'n31': (lambda: [_random_uv(31, 7)], 30, 10),
    'n300': (lambda: [_random_uv(300, 8)], 30, 10),
    'lattice_6x6': (lambda: [np.array([[100.0 + 3 * i, 200.0 + 3 * j] for i in range(6) for j in range(6)])], 30, 10),
    'dup12_plus_25': (lambda: [_dup_image(12, 25, 9)], 30, 10),
    'dup31_plus_5': (lambda: [_dup_image(31, 5, 10)], 30, 10),
    'ten_positives': (lambda: [_random_uv(11, 11)], 30, 10),
    'mixed_images': (lambda: [_random_uv(5, 12), _random_uv(0, 13), _random_uv(140, 14), _random_uv(2, 15),
                              _dup_image(4, 33, 16), _random_uv(1, 17), _random_uv(64, 18)], 30, 10),
    'k5_pos2': (lambda: [_random_uv(40, 19), _random_uv(3, 20), _dup_image(3, 6, 21)], 5, 2),
    'k32_pos32': (lambda: [_random_uv(70, 22)], 32, 32),
}


@pytest.mark.parametrize('case', sorted(KNN_CASES))
def test_knn_fit_equals_restatement(case):
    images, k, n_pos = KNN_CASES[case]
    img_ptr, uv, ned, chain = _table(images())
    want = sr.knn_fit(img_ptr, uv, ned, chain, k, n_pos)
    got = abi_knn_fit(img_ptr, uv, ned, chain, k, n_pos)
    w_tgt, w_val, w_used, w_fit, w_status = want
    # what the case is there for
    if case == 'sizes_0_1_2':
        assert np.all(w_status == sr.SKIPPED_SMALL) and len(w_status) == 3
    elif case == 'dup12_plus_25':
        q = int(np.argmax(np.sum(np.all(uv[:, None] == uv[None], 2), 1)))       # one of the twelve
        assert w_used[q] == 12 + 10                              # 18 positives listed, the walk stops on the eleventh
    elif case == 'dup31_plus_5':
        assert int(np.sum(w_status == sr.SKIPPED_FLAT)) == 31 and int(np.sum(w_status == sr.FITTED)) == 5
    elif case == 'ten_positives':
        assert np.all(w_used == 11)                              # the walk ends with the list
    elif case == 'lattice_6x6':
        d = uv[0] - uv
        assert len(np.unique(d[:, 0] ** 2 + d[:, 1] ** 2)) < 30  # ties: the index decides
    elif case == 'n300':
        assert len(uv) > 256                                     # more than one tile, more than one query block
    for name, g, w in zip(('tgt', 'val', 'used', 'fit', 'status'), got, want):
        assert g[:len(w)].tobytes() == np.ascontiguousarray(w).tobytes(), name
    # unused slots: tgt -1, val 0 (the restatement starts from them; said once more for the sentinel)
    slot = np.arange(k)[None, :] >= got[2][:len(w_used), None]
    assert np.all(got[0][:len(w_used)][slot] == -1) and np.all(got[1][:len(w_used)][slot] == 0.0)


def test_knn_fit_no_observations_and_bad_arguments():
    from imageanalysis_amd import _lib
    img_ptr, uv, ned, chain = _table([_random_uv(0, 1), _random_uv(0, 2)])
    got = abi_knn_fit(img_ptr, uv, ned, chain)
    assert np.all(got[0] == -77) and np.all(got[4] == -77)      # no launch
    L = _lib.lib()
    one = ctypes.c_void_p(8)
    for k, n_pos, n in ((0, 10, 5), (33, 10, 5), (30, 0, 5), (30, 33, 5), (30, 10, -1), (30, 10, 2 ** 31 // 30 + 1)):
        assert L.iamx_surface_knn_fit(one, one, one, one, 1, n, k, n_pos, one, one, one, one, one, None) == -1
    assert L.iamx_surface_knn_fit(None, one, one, one, 1, 5, 30, 10, one, one, one, one, one, None) == -1
    assert L.iamx_surface_chain_metric(one, one, one, 5, 0, one, 3, one, one, one, one, one, one, None) == -1
    assert L.iamx_surface_chain_metric(one, one, one, 5, 30, None, 3, one, one, one, one, one, one, None) == -1
    assert L.iamx_chain_outlier_stats(None, one, 3, 5.0, 1, one, one, one, one, one, one, one, one, None) == -1
    assert L.iamx_chain_outlier_stats(one, one, 3, float('nan'), 1, one, one, one, one, one, one, one, one, None) == -1
    assert L.iamx_chain_depths(None, one, 2, 5, one, one, one, 3, one, one, one, one, None) == -1
    assert L.iamx_chain_depths(one, one, 0, 5, one, one, one, 3, one, one, one, one, None) == -1


# ---------------------------------------------------------------------------------------------
# iamx_surface_chain_metric
# ---------------------------------------------------------------------------------------------
def test_chain_metric_equals_restatement():
    img_ptr, uv, ned, chain = _table([_random_uv(60, 31), _random_uv(45, 32), _random_uv(2, 33), _random_uv(80, 34)],
                                     n_chains=40)
    n_chains = 44
    chain[[3, 60 + 7, 107 + 11]] = 41                            # a target from three images
    chain[105:107] = 42                                          # only in the image of two observations
    tgt, val, _used, _fit, status = sr.knn_fit(img_ptr, uv, ned, chain)
    looked = np.ones(n_chains, bool)
    looked[40] = False                                           # (43 is looked at and never a target)
    w_sum, w_count, w_metric = sr.chain_metric(tgt, val, n_chains)
    assert w_count[41] >= 3 and w_count[42] == 0 and w_count[43] == 0 and w_metric[43] == 0.0
    queries = np.nonzero(np.any(tgt == 41, 1))[0]
    assert set((np.searchsorted(img_ptr, queries, side='right') - 1).tolist()) == {0, 1, 3}
    g_sum, g_count, g_metric, counters = abi_chain_metric(tgt, val, status, looked, n_chains)
    assert g_sum.tobytes() == w_sum.tobytes() and np.array_equal(g_count, w_count)
    assert g_metric.tobytes() == w_metric.tobytes()
    assert counters.tolist() == [2, int(np.sum(status == sr.SKIPPED_FLAT)), int(np.sum(looked & (w_count == 0))), 43]
    # and again: the fill's atomics may fall differently, the sums may not
    again = abi_chain_metric(tgt, val, status, looked, n_chains)
    assert again[0].tobytes() == g_sum.tobytes()


def test_chain_metric_without_observations():
    looked = np.array([1, 0, 1, 1, 0], bool)
    g_sum, g_count, g_metric, counters = abi_chain_metric(np.zeros((0, 30), np.int32), np.zeros((0, 30)),
                                                          np.zeros(0, np.int32), looked, 5)
    assert np.all(g_sum == 0.0) and np.all(g_count == 0) and np.all(g_metric == 0.0)
    assert counters.tolist() == [0, 0, 3, 3]
    g = abi_chain_metric(np.zeros((0, 30), np.int32), np.zeros((0, 30)), np.zeros(0, np.int32), looked[:0], 0)
    assert np.all(g[0] == -7.5) and np.all(g[3] == -77)          # no chains: no launch


# ---------------------------------------------------------------------------------------------
# iamx_chain_outlier_stats
# ---------------------------------------------------------------------------------------------
def _stats_input(case):
    rng = np.random.default_rng(41)
    if case == 'one':
        return np.array([3.25]), np.ones(1, bool)
    if case == 'equal':
        return np.full(700, 0.125), np.ones(700, bool)
    n = 1000 if case == 'thousand' else 70000                    # 70000: more tiles than one workgroup folds at once
    metric = np.abs(rng.normal(0.2, 0.05, n))
    metric[rng.choice(n, 9, replace=False)] = rng.uniform(2.0, 9.0, 9)
    metric[rng.choice(n, 3, replace=False)] = 0.0
    looked = rng.uniform(size=n) < 0.9
    return metric, looked


@pytest.mark.parametrize('two_sided', [True, False], ids=['two_sided', 'one_sided'])
@pytest.mark.parametrize('case', ['one', 'equal', 'thousand', 'seventy_thousand'])
def test_outlier_stats_equal_restatement(case, two_sided):
    metric, looked = _stats_input(case)
    factor = 5.0 if two_sided else 3.0
    average, stddev, flag, margin = sr.outlier_stats(metric, looked, factor, two_sided)
    assert margin > 1e-9                                         # no chain sits on its threshold
    stats, g_flag, idx, sel = abi_outlier_stats(metric, looked, factor, two_sided)
    assert abs(stats[0] - average) <= 1e-12 * abs(average)
    assert abs(stats[1] - stddev) <= 1e-12 * abs(stddev)
    assert stats[2] == looked.sum()
    assert np.array_equal(g_flag != 0, flag)
    assert idx.tolist() == np.nonzero(flag)[0].tolist() and sel.tobytes() == metric[flag].tobytes()
    if case in ('one', 'equal'):
        assert stats[1] == 0.0 and not flag.any()
    else:
        assert flag.any() and not flag.all()
    again = abi_outlier_stats(metric, looked, factor, two_sided)
    assert again[0].tobytes() == stats.tobytes() and again[1].tobytes() == g_flag.tobytes()


def test_outlier_stats_nobody_looked_at():
    stats, flag, idx, _sel = abi_outlier_stats(np.array([1.0, 200.0, 3.0]), np.zeros(3, bool), 5.0, True)
    assert stats[:3].tolist() == [0.0, 0.0, 0.0] and not flag.any() and len(idx) == 0


# ---------------------------------------------------------------------------------------------
# iamx_chain_depths
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene():
    return sr.planted_scene()


def test_chain_depths_equal_restatement(scene):
    matches, cam, _ = scene
    rows = pickle.loads(pickle.dumps(matches[:500]))
    rows.append([[10.0, 20.0, 1.0], 0, [3, [5.0, 6.0]]])                      # one member: not looked at
    rows.append([[30.0, 40.0, 0.5], 0, [2, [5.0, 6.0]], [12, [7.0, 8.0]]])    # one member in the group
    cam = np.concatenate([cam, [[700.0, 700.0, -100.0]], [[800.0, 800.0, -100.0]]])
    in_group = np.array([1] * 12 + [0, 1], np.uint8)                          # image 13: in the group, no observation
    img_ptr, _uv, ned, _chain, chain_ptr, chain_obs = sr.observation_table(rows, in_group, 0)
    assert img_ptr[13] == img_ptr[14] and np.diff(chain_ptr)[-2:].tolist() == [1, 1]
    w_depth, w_z, w_metric, w_looked = sr.chain_depths(img_ptr, ned, cam, chain_ptr, chain_obs)
    g_depth, g_z, g_metric, g_looked = abi_chain_depths(img_ptr, ned, cam, chain_ptr, chain_obs)
    assert g_depth.tobytes() == w_depth.tobytes()
    assert np.array_equal(g_looked != 0, w_looked) and not w_looked[-1] and not w_looked[-2]
    assert np.all(np.abs(g_z - w_z) <= 1e-12 * np.abs(w_z)) and g_z[13].tolist() == [0.0, 0.0, 0.0]
    assert np.all(np.abs(g_metric - w_metric) <= 1e-12 * np.abs(w_metric)) and w_metric.max() > 0
    assert np.all(g_metric[~w_looked] == 0.0)
    assert img_ptr[-1] > 256 and int(np.diff(img_ptr).max()) < 256
    # an image with more observations than one workgroup has threads: every chain seen by one camera
    big_ptr = np.array([0, len(ned)], np.int64)
    w = sr.chain_depths(big_ptr, ned, cam[:1], chain_ptr, chain_obs)
    g = abi_chain_depths(big_ptr, ned, cam[:1], chain_ptr, chain_obs)
    assert g[0].tobytes() == w[0].tobytes() and np.all(np.abs(g[1] - w[1]) <= 1e-12 * np.abs(w[1]))
    # here a chain's metric is a few metres against depths of hundreds: it is a difference from the image
    # mean and inherits that mean's absolute error (within 1e-12 of the MEAN, asserted above), whatever
    # the order its own few terms are added in
    assert np.all(np.abs(g[2] - w[2]) <= 1e-12 * (np.abs(w[2]) + w[1][0, 0]))


# ---------------------------------------------------------------------------------------------
# the whole flow
# ---------------------------------------------------------------------------------------------
def _project(cam):
    from imageanalysis_amd.hostlib.image_pose import PoseProject
    names = ['IMG_%02d' % i for i in range(len(cam))]
    proj = PoseProject(names)
    for im, p in zip(proj.image_list, cam):
        im.set_camera_pose([float(v) for v in p], 0.0, 0.0, 0.0)
        im.set_camera_pose([float(v) for v in p], 0.0, 0.0, 0.0, opt=True)
    return proj, [names]


@pytest.mark.parametrize('as_arrays', [False, True], ids=['lists', 'chains'])
def test_planted_scene_through_the_python_layer(scene, as_arrays):
    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd.match_cleanup import Chains
    matches, cam, planted = scene
    proj, group_list = _project(cam)
    in_group = np.ones(len(cam), np.uint8)
    want = sr.cull_surface(matches, in_group, 0)
    assert all(r['margin'] >= 1e-6 for r in want)
    work = pickle.loads(pickle.dumps(matches))
    work = Chains.from_lists(work) if as_arrays else work
    report = cull.surface_consistency(proj, work, group_list, 0)
    assert report.metric.cpu().numpy().tobytes() == want[0]['metric'].tobytes()
    assert np.array_equal(report.count.cpu().numpy(), want[0]['count'])
    assert (report.n_small, report.n_flat, report.n_uncounted, report.n_looked) == (0, 0, 0, len(matches))
    idx, average, dev = cull.surface_outliers(report, 5)
    assert idx.tolist() == want[0]['culled']
    assert abs(average - want[0]['average']) <= 1e-12 * average and abs(dev - want[0]['stddev']) <= 1e-12 * dev
    rounds = cull.cull_surface(proj, work, group_list, 0)
    assert rounds == [r['culled'] for r in want] and sorted(c for r in rounds for c in r) == planted
    w_marks, w_z, _avg, _dev, margin = sr.depth_outliers(matches, in_group, 0, cam, 3)
    assert margin >= 1e-6
    fresh = pickle.loads(pickle.dumps(matches))
    marks, rows = cull.depth_outliers(proj, Chains.from_lists(fresh) if as_arrays else fresh, group_list, 0, 3)
    assert marks == w_marks and len(marks) >= 3
    assert [r[1] for r in rows] == w_z[:, 2].astype(int).tolist()
    assert np.allclose([r[2] for r in rows], w_z[:, 0], rtol=1e-12, atol=0)
    cull.delete_marked_features(work, 3)
    assert pickle.loads(pickle.dumps(work)) == [m for c, m in enumerate(matches) if c not in planted]
    assert not as_arrays or work.untouched()


def test_python_layer_error_paths(scene):
    from imageanalysis_amd import match_culling as cull
    matches, cam, _ = scene
    proj, group_list = _project(cam)
    rows = pickle.loads(pickle.dumps(matches[:50]))
    with pytest.raises(IndexError, match='group 1 of 1'):
        cull.surface_consistency(proj, rows, group_list, 1)
    with pytest.raises(IndexError, match='group 1 of 1'):
        cull.depth_outliers(proj, rows, group_list, 1)
    rows[4][2][0] = 12
    with pytest.raises(IndexError, match='chain 4 refers to image 12, the project has 12 images'):
        cull.cull_surface(proj, rows, group_list, 0)
    with pytest.raises(IndexError, match='chain 4 refers to image 12'):
        cull.depth_outliers(proj, rows, group_list, 0)
    rows[4][2][0] = 1
    rows[6][0] = None
    with pytest.raises(ValueError, match='chain 6 of group 0 has no position'):
        cull.cull_surface(proj, rows, group_list, 0)
    with pytest.raises(ValueError, match='chain 6 of group 0 has no position'):
        cull.depth_outliers(proj, rows, group_list, 0)
    with pytest.raises(ValueError, match='within 1..32'):
        cull.surface_consistency(proj, rows, group_list, 0, k=33)
    assert cull.cull_surface(proj, [], group_list, 0) == [[]]    # no chains: one empty round


# the script twins, run the way a user runs them (stand-ins for the reference's lib.project / lib.groups)
LIB_STANDIN = {
    '__init__.py': '',
    'groups.py': textwrap.dedent('''\
        import json, os
        def load(path):
            return json.load(open(os.path.join(path, 'groups.json')))
        '''),
    'project.py': textwrap.dedent('''\
        import os, pickle, sys
        sys.path.insert(0, os.environ['IAMX_TEST_DIR'])
        import chain_tools_common as ct
        class ProjectMgr(object):
            """stand-in: the poses / camera of the golden record in the project directory"""
            def __init__(self, project_dir):
                self.analysis_dir = os.path.join(project_dir, 'ImageAnalysis')
                self._g = pickle.load(open(os.path.join(project_dir, 'record.pkl'), 'rb'))
            def load_images_info(self):
                self.image_list = ct.project(self._g).image_list
        '''),
}


def _run_twin(script, g, matches_bytes, tmp_path, argv, answer):
    lib = tmp_path / 'standin' / 'lib'
    lib.mkdir(parents=True, exist_ok=True)
    for name, text in LIB_STANDIN.items():
        (lib / name).write_text(text)
    proj = tmp_path / ('project_' + answer.strip())
    (proj / 'ImageAnalysis').mkdir(parents=True)
    (proj / 'ImageAnalysis' / 'matches_grouped').write_bytes(matches_bytes)
    (proj / 'ImageAnalysis' / 'groups.json').write_text(json.dumps(g['groups']))
    rec = {k: v for k, v in g.items() if k not in ('matches_in', 'matches_out', 'stdout')}
    (proj / 'record.pkl').write_bytes(pickle.dumps(rec))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / 'standin'), ct.REPO]),
               IAMX_TEST_DIR=os.path.dirname(os.path.abspath(__file__)))
    cmd = ['timeout', '-k', '10', '300', sys.executable,
           os.path.join(ct.REPO, 'imageanalysis_amd', 'scripts', script), str(proj)] + argv
    p = subprocess.run(cmd, input=answer, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout, (proj / 'ImageAnalysis' / 'matches_grouped').read_bytes()


@pytest.fixture(scope='module')
def golden_project():
    """a chain_colocated record's inputs (matches_in, poses_opt, groups) with a few positions displaced"""
    g = ct.load([p for p in ct.COLO_CASES if 'mid_default' in p][0])
    rows = pickle.loads(g['matches_in'])
    sc = ct.Scene(g, 0)
    mine = [c for c, m in enumerate(rows) if m[1] == 0]
    displaced = mine[5::97][:5]
    for n, c in enumerate(displaced):
        rows[c][0] = [rows[c][0][0], rows[c][0][1], rows[c][0][2] + (25.0 + 5 * n) * (-1) ** n]
    return g, rows, sc, displaced


def test_surface_script_twin(golden_project, tmp_path):
    g, rows, sc, displaced = golden_project
    rounds = sr.cull_surface(rows, sc.in_group, 0)
    assert all(r['margin'] >= 1e-6 for r in rounds)
    culled = sorted(c for r in rounds for c in r['culled'])
    assert culled and set(displaced) & set(culled)
    data = pickle.dumps(rows)
    stdout, written = _run_twin('4c-surface-outliers.py', g, data, tmp_path, [], 'y\n')
    assert pickle.loads(written) == [m for c, m in enumerate(rows) if c not in culled]
    lines = stdout.splitlines()
    assert sum('culled' in l for l in lines) == len(rounds)
    assert 'Outliers to remove from match lists: %d' % len(culled) in lines
    assert not any('outlier - match index' in l for l in lines)
    assert 'average value = %.2f' % rounds[0]['average'] in lines
    _stdout, kept = _run_twin('4c-surface-outliers.py', g, data, tmp_path, [], 'n\n')
    assert kept == data


def _expected_after_depth(rows, marks, n_images, min_features, min_chain_len, strong):
    work = pickle.loads(pickle.dumps(rows))
    for c, j in marks:
        work[c][2 + j] = [-1, -1]
    if min_features > 0:
        for c, j in sr.weak_images(work, n_images, min_features):
            work[c][2 + j] = [-1, -1]
    out = []
    for m in work:
        members = [p for p in m[2:] if p != [-1, -1]]
        if len(members) == len(m) - 2:
            out.append(m)
        elif not strong and len(members) >= min_chain_len:
            out.append(m[:2] + members)
    return out


@pytest.mark.parametrize('argv,min_features,strong', [([], 25, False), (['--min-features', '0', '--strong'], 0, True)],
                         ids=['default', 'strong_no_weak'])
def test_depth_script_twin(golden_project, tmp_path, argv, min_features, strong):
    g, rows, sc, displaced = golden_project
    marks, z, average, dev, margin = sr.depth_outliers(rows, sc.in_group, 0, sc.pos, 3)
    assert margin >= 1e-6 and marks and set(m[0] for m in marks) & set(displaced)
    want = _expected_after_depth(rows, marks, len(sc.pos), min_features, g['min_chain_len'], strong)
    assert 0 < len(want) < len(rows)
    data = pickle.dumps(rows)
    stdout, written = _run_twin('4c-by-depth.py', g, data, tmp_path, argv, 'y\n')
    assert pickle.loads(written) == want
    lines = stdout.splitlines()
    assert 'mean = %.4f stddev = %.4f' % (average, dev) in lines
    assert sum(' features: ' in l and ' avg: ' in l for l in lines) == len(sc.pos)
    assert any(l.startswith('weak images:') for l in lines) == (min_features > 0)
    _stdout, kept = _run_twin('4c-by-depth.py', g, data, tmp_path, argv, 'n\n')
    assert kept == data
