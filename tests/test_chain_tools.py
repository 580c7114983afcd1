"""CPU: the chain tools' host side -- the restatements (tests/undistort_restatement.py,
tests/chain_tools_common.py) against the reference's own runs (tests/golden/chain_*.pkl.gz,
tools/gen_chain_tools_golden.py), the mark bookkeeping (per-member counts -> mark_list order and
duplicates -> delete_marked_features) on both chain representations, and the new exports' argument
checks, which need no GPU."""
import contextlib
import ctypes
import io
import os
import pickle

import numpy as np
import pytest

import chain_tools_common as ct
import undistort_restatement as ur


def test_goldens_are_all_there():
    names = sorted(os.path.basename(p) for p in ct.TRI_CASES + ct.COLO_CASES)
    want = ['chain_colocated_%s_%s.pkl.gz' % (s, c) for s in ('dist', 'mid')
            for c in ('close', 'default', 'group1', 'wide')] + \
           ['chain_triangulate_%s_%s.pkl.gz' % (s, c) for s in ('dist', 'mid') for c in ('default', 'group1')]
    assert names == sorted(want)
    for p in ct.TRI_CASES + ct.COLO_CASES:
        assert ct.load(p)['margin'] >= 1e-6 and os.path.getsize(p) < (1 << 20)


# ---------------------------------------------------------------------------------------------
# undistort restatement
# ---------------------------------------------------------------------------------------------
def _distort(xy, K, dist):
    """the forward model (what redistort / cv2.projectPoints apply), f64"""
    k1, k2, p1, p2, k3 = dist
    x = (xy[:, 0] - K[0, 2]) / K[0, 0]
    y = (xy[:, 1] - K[1, 2]) / K[1, 1]
    r2 = x * x + y * y
    rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], 1)


def test_undistort_restatement_zero_distortion_is_float32_identity():
    g = ct.load([p for p in ct.TRI_CASES if 'mid_default' in p][0])
    K = np.array(g['camera']['K_opt']).reshape(3, 3)
    uv = np.array([p[1] for m in pickle.loads(g['matches_in']) for p in m[2:]], np.float32)
    out = ur.undistort_points(uv, K, np.zeros(5))
    assert out.dtype == np.float32 and out.shape == uv.shape
    # (u - cx)/fx*fx + cx in f64, rounded to f32: within one f32 ulp of u
    assert np.all(np.abs(out.astype(np.float64) - uv) <= np.spacing(np.abs(uv)))


def test_undistort_restatement_inverts_the_lens_model():
    g = ct.load([p for p in ct.TRI_CASES if 'dist_default' in p][0])
    K = np.array(g['camera']['K_opt']).reshape(3, 3)
    dist = np.array(g['camera']['dist_opt'])
    assert np.any(dist != 0)
    uv = np.array([p[1] for m in pickle.loads(g['matches_in']) for p in m[2:]], np.float32)
    und = ur.undistort_points(uv, K, dist)
    back = _distort(und.astype(np.float64), K, dist)
    # five fixed-point rounds on this lens (|k1| r^2 < 0.1 inside the frame) contract to well under
    # 0.05 px; the f32 rounding of the output adds 2^-12 px
    assert np.max(np.abs(back - uv)) < 0.05
    assert np.max(np.abs(und - uv)) > 1.0                       # and it is not the identity here


def test_undistort_restatement_negative_icdist_falls_back():
    K = np.array([[100.0, 0, 50], [0, 100.0, 50], [0, 0, 1]])
    dist = np.array([-1.0, 0, 0, 0, 0])                         # 1 + k1 r^2 < 0 beyond r = 1
    uv = np.array([[50, 50], [60, 55], [400, 50], [50, -300]], np.float32)
    out = ur.undistort_points(uv, K, dist)
    assert np.array_equal(out[2:], uv[2:])                      # x0, y0 come back
    assert np.array_equal(out[0], uv[0]) and not np.array_equal(out[1], uv[1])
    assert ur.cv2_undistortPoints(uv.reshape(-1, 1, 2), K, dist, P=K).shape == (4, 1, 2)
    assert ur.undistort_points(np.zeros((0, 2), np.float32), K, dist).shape == (0, 2)


# ---------------------------------------------------------------------------------------------
# restatements against the reference's runs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ct.TRI_CASES, ids=os.path.basename)
def test_triangulate_restatement_matches_reference(path):
    g = ct.load(path)
    sc = ct.Scene(g, ct.group_of(g), 'initial')
    matches = pickle.loads(g['matches_in'])
    ref = pickle.loads(g['matches_out'])
    res = ct.triangulate_restatement(sc, matches)
    assert sorted(res) == g['written'] and len(g['written']) > 0
    for (c, (x, cond, s, _rho)), cond_ref in zip(sorted(res.items()), g['cond']):
        assert abs(cond - cond_ref) <= 1e-9 * cond_ref
        x_ref = np.array(ref[c][0])
        assert np.linalg.norm(x - x_ref) <= ct.triangulate_bound(cond_ref, s, x_ref), c
    assert sum(x[2] > 0 for x, _c, _s, _r in res.values()) == g['n_whoa']
    for c, (a, b) in enumerate(zip(matches, ref)):
        if c not in res:
            assert a == b                                       # untouched chains: unchanged


@pytest.mark.parametrize('path', ct.COLO_CASES, ids=os.path.basename)
def test_pair_angle_restatement_matches_reference(path):
    g = ct.load(path)
    sc = ct.Scene(g, g['group_index'])
    marks, margin, pairs = ct.pair_angles_restatement(sc, pickle.loads(g['matches_in']), g['min_angle'])
    assert marks == [list(m) for m in g['marked']] and pairs == g['n_pairs']
    assert abs(margin - g['margin']) <= 1e-9 * g['margin']


def test_close_goldens_hold_the_three_situations():
    for path in [p for p in ct.COLO_CASES if '_close' in p]:
        g = ct.load(path)
        before, after = pickle.loads(g['matches_in']), pickle.loads(g['matches_out'])
        marked = [tuple(m) for m in g['marked']]
        assert len(after) < len(before)                                        # a deleted chain
        assert len(set(marked)) < len(marked)                                  # a member marked twice
        lost = {}
        for k, i in set(marked):
            lost[k] = lost.get(k, 0) + 1
        assert any(len(before[k]) - 2 - n >= g['min_chain_len'] for k, n in lost.items())
    for path in [p for p in ct.COLO_CASES if '_default' in p]:
        g = ct.load(path)
        assert g['marked'] == [] and g['matches_out'] is None                  # not rewritten


# ---------------------------------------------------------------------------------------------
# mark bookkeeping
# ---------------------------------------------------------------------------------------------
def _reference_tail(g):
    """the reference's stdout from the first mark on"""
    lines = g['stdout'].splitlines()
    at = lines.index('Scanning match pair angles:')
    return lines[at + 1:]


@pytest.mark.parametrize('as_arrays', [False, True], ids=['lists', 'chains'])
@pytest.mark.parametrize('path', [p for p in ct.COLO_CASES if ct.load(p)['marked']], ids=os.path.basename)
def test_counts_to_marks_to_deletion(path, as_arrays):
    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd.match_cleanup import Chains
    g = ct.load(path)
    rows = pickle.loads(g['matches_in'])
    ptr = ct.flatten(rows)[0]
    marked = [list(m) for m in g['marked']]
    count = ct.counts_from_marks(ptr, marked)
    assert count.max() > 1 or '_close' not in path
    mark_list = cull.marks_from_counts(ptr, count)
    assert mark_list == marked                                  # order and duplicates
    matches = Chains.from_lists(rows) if as_arrays else rows
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        cull.mark_using_list(mark_list, matches)
        print('Outliers to remove from match lists:', len(mark_list))
        print('Save these changes? (y/n):', end='')
        cull.delete_marked_features(matches, g['min_chain_len'])
        print("Writing original matches:", 'matches_grouped')
    if as_arrays:
        # (a Chains pickles as list(rows): the same lists, behind a different first opcode)
        assert matches.untouched()
        back = pickle.loads(pickle.dumps(matches))
        assert type(back) is list and back == pickle.loads(g['matches_out'])
    else:
        assert pickle.dumps(matches) == g['matches_out']
    assert out.getvalue().splitlines() == _reference_tail(g)


def test_marks_from_counts_edges():
    from imageanalysis_amd import match_culling as cull
    assert cull.marks_from_counts(np.array([0]), np.zeros(0, np.int32)) == []
    assert cull.marks_from_counts(np.array([0, 2, 2, 5]), np.zeros(5, np.int32)) == []
    assert cull.marks_from_counts(np.array([0, 2, 2, 5]), np.array([0, 1, 3, 0, 1])) == \
        [[0, 1], [2, 0], [2, 0], [2, 0], [2, 2]]


# ---------------------------------------------------------------------------------------------
# argument checks (no GPU)
# ---------------------------------------------------------------------------------------------
def test_abi_argument_checks_need_no_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    k4 = (ctypes.c_double * 4)(100, 100, 50, 50)
    d5 = (ctypes.c_double * 5)()
    one = ctypes.c_void_p(8)                                    # never dereferenced: the checks come first
    # n == 0: 0 without a launch, whatever the other pointers are
    assert L.iamx_undistort_points(None, 0, k4, d5, None, None) == 0
    assert L.iamx_chain_triangulate(None, None, None, None, 0, 0, None, None, None, 0, k4, d5,
                                    None, None, None) == 0
    assert L.iamx_chain_pair_angles(None, None, None, None, 0, 0, None, None, 0, 1.0,
                                    None, None, None, None) == 0
    # null pointers and bad sizes
    assert L.iamx_undistort_points(None, 4, k4, d5, one, None) == -1 and b'null pointer' in L.iamx_last_error()
    assert L.iamx_undistort_points(one, 4, None, d5, one, None) == -1
    assert L.iamx_undistort_points(one, -1, k4, d5, one, None) == -1 and b'bad size' in L.iamx_last_error()
    k0 = (ctypes.c_double * 4)(0, 100, 50, 50)
    assert L.iamx_undistort_points(one, 4, k0, d5, one, None) == -1 and b'focal' in L.iamx_last_error()
    args = [one, one, one, one, 3, 0, one, one, one, 2, k4, d5, one, one, None]
    for k in (0, 1, 2, 3, 6, 7, 8, 10, 11, 12, 13):
        a = list(args)
        a[k] = None
        assert L.iamx_chain_triangulate(*a) == -1, k
    a = list(args)
    a[4] = -1
    assert L.iamx_chain_triangulate(*a) == -1 and b'bad size' in L.iamx_last_error()
    a = list(args)
    a[9] = -2
    assert L.iamx_chain_triangulate(*a) == -1
    args = [one, one, one, one, 3, 0, one, one, 2, 1.0, one, one, one, None]
    for k in (0, 1, 2, 3, 6, 7, 10, 11, 12):
        a = list(args)
        a[k] = None
        assert L.iamx_chain_pair_angles(*a) == -1, k
    a = list(args)
    a[4] = -5
    assert L.iamx_chain_pair_angles(*a) == -1


def test_python_argument_checks_and_empty_inputs():
    from imageanalysis_amd import match_cleanup, undistort
    from imageanalysis_amd import match_culling as cull
    g = ct.load([p for p in ct.COLO_CASES if 'dist_default' in p][0])
    proj = ct.project(g)
    K = np.array(g['camera']['K_opt']).reshape(3, 3)
    # n == 0 everywhere: no device needed
    out = undistort.undistort_points(np.zeros((0, 2)), K, g['camera']['dist_opt'])
    assert out.shape == (0, 2) and out.dtype == np.float32
    assert undistort.undistort_uvlist(proj, proj.image_list[0], []) == []
    assert undistort.undistort_image_keypoints(proj, proj.image_list[0]) is None
    res = match_cleanup.triangulate_rays(proj, [], g['groups'], 0)
    assert len(res.written) == 0 and len(res.below) == 0
    assert cull.colocated_features(proj, [], g['groups'], 0, 1.0) == []
    empty = match_cleanup.Chains(np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros(1, np.int64))
    assert cull.colocated_features(proj, empty, g['groups'], 0, 1.0) == []
    assert len(match_cleanup.triangulate_rays(proj, empty, g['groups'], 0).written) == 0
    # argument errors come before any device work
    with pytest.raises(ValueError):
        undistort.undistort_points(np.zeros((3, 3)), K, np.zeros(5))
    with pytest.raises(ValueError):
        undistort.undistort_points(np.zeros((3, 2)), np.zeros((2, 2)), np.zeros(5))
    with pytest.raises(ValueError):
        undistort.undistort_points(np.zeros((3, 2)), K, np.zeros(4))
    with pytest.raises(ValueError):
        undistort.undistort_points(np.zeros((3, 2)), [0.0, 1.0, 2.0, 3.0], np.zeros(5))
    matches = pickle.loads(g['matches_in'])
    with pytest.raises(ValueError):
        match_cleanup.triangulate_rays(proj, matches, g['groups'], 0, attitude='refined')
    with pytest.raises(IndexError):
        match_cleanup.triangulate_rays(proj, matches, g['groups'], 7)
    with pytest.raises(IndexError):
        cull.colocated_features(proj, matches, g['groups'], -1, 1.0)
    with pytest.raises(ValueError):
        cull.colocated_features(proj, matches, g['groups'], 0, float('nan'))
    k = [i for i, m in enumerate(matches) if m[1] == 0][3]
    matches[k][0] = None
    with pytest.raises(ValueError, match='chain %d of group 0 has no position' % k):
        cull.colocated_features(proj, matches, g['groups'], 0, 1.0)


def test_chain_arrays_of_both_representations_agree():
    from imageanalysis_amd import match_cleanup
    g = ct.load([p for p in ct.TRI_CASES if 'dist_default' in p][0])
    rows = pickle.loads(g['matches_in'])
    rows[5][0] = None
    a = match_cleanup.chain_arrays(rows)
    b = match_cleanup.chain_arrays(match_cleanup.Chains.from_lists(rows))
    c = ct.flatten(rows)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z) and x.dtype == y.dtype == z.dtype


def test_install_hook_puts_the_three_methods_on_a_class():
    from imageanalysis_amd import undistort

    class ProjectMgr(object):
        pass
    undistort.install(ProjectMgr)
    for name in ('undistort_uvlist', 'undistort_image_keypoints', 'undistort_keypoints'):
        assert getattr(ProjectMgr, name) is getattr(undistort, name)
