"""GPU: the kernels of csrc/chain_geom.hip through the C ABI -- iamx_undistort_points bit for bit
against tests/undistort_restatement.py, iamx_chain_triangulate against the reference's own output
(tests/golden/chain_triangulate_*.pkl.gz) and a numpy restatement, iamx_chain_pair_angles and the
4b-colocated-feats flow against the reference's marks, bytes and stdout
(tests/golden/chain_colocated_*.pkl.gz)."""
import contextlib
import ctypes
import io
import os
import json
import pickle
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest

import chain_tools_common as ct
import undistort_restatement as ur

pytestmark = pytest.mark.gpu

UNTOUCHED, WRITTEN, BELOW, SINGULAR, BAD_IMAGE = range(5)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0') for a in arrays]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def abi_undistort(uv, k4, dist):
    import torch
    from imageanalysis_amd import _lib
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    n = len(uv)
    k4, dist = np.ascontiguousarray(k4, np.float64), np.ascontiguousarray(dist, np.float64)
    d_src, = _dev(uv if n else np.zeros((1, 2), np.float32))
    d_dst = torch.full_like(d_src, -7.0)
    _lib.check(_lib.lib().iamx_undistort_points(_p(d_src), n, _hp(k4), _hp(dist), _p(d_dst), _lib.stream_ptr()),
               'iamx_undistort_points')
    torch.cuda.synchronize()
    return d_dst.cpu().numpy()[:n] if n else d_dst.cpu().numpy()


def abi_triangulate(sc, arrays):
    """-> (ned after, status)"""
    import torch
    from imageanalysis_amd import _lib
    ptr, img, uv, group, ned, _has = arrays
    n = len(ptr) - 1
    d_ptr, d_img, d_uv, d_group, d_M, d_pos, d_in, d_ned = _dev(
        ptr, img if len(img) else np.zeros(1, np.int32), uv if len(uv) else np.zeros((1, 2)),
        group if n else np.zeros(1, np.int32), sc.M, sc.pos, sc.in_group, ned if n else np.zeros((1, 3)))
    d_status = torch.full((max(n, 1),), -9, dtype=torch.int32, device='cuda:0')
    _lib.check(_lib.lib().iamx_chain_triangulate(
        _p(d_ptr), _p(d_img), _p(d_uv), _p(d_group), n, sc.group_index, _p(d_M), _p(d_pos), _p(d_in),
        len(sc.pos), _hp(sc.k4), _hp(sc.dist), _p(d_ned), _p(d_status), _lib.stream_ptr()),
        'iamx_chain_triangulate')
    torch.cuda.synchronize()
    return d_ned.cpu().numpy()[:n], d_status.cpu().numpy()[:n] if n else d_status.cpu().numpy()


def abi_pair_angles(sc, arrays, min_angle):
    """-> (count per member, total, status)"""
    import torch
    from imageanalysis_amd import _lib
    ptr, img, _uv, group, ned, _has = arrays
    n = len(ptr) - 1
    d_ptr, d_img, d_group, d_ned, d_pos, d_in = _dev(
        ptr, img if len(img) else np.zeros(1, np.int32), group if n else np.zeros(1, np.int32),
        ned if n else np.zeros((1, 3)), sc.pos, sc.in_group)
    d_count = torch.full((max(len(img), 1),), -9, dtype=torch.int32, device='cuda:0')
    d_total = torch.full((1,), -9, dtype=torch.int64, device='cuda:0')
    d_status = torch.full((max(n, 1),), -9, dtype=torch.int32, device='cuda:0')
    _lib.check(_lib.lib().iamx_chain_pair_angles(
        _p(d_ptr), _p(d_img), _p(d_group), _p(d_ned), n, sc.group_index, _p(d_pos), _p(d_in), len(sc.pos),
        float(min_angle), _p(d_count), _p(d_total), _p(d_status), _lib.stream_ptr()), 'iamx_chain_pair_angles')
    torch.cuda.synchronize()
    return d_count.cpu().numpy()[:len(img)], int(d_total.item()), d_status.cpu().numpy()[:max(n, 1)]


# ---------------------------------------------------------------------------------------------
# undistort
# ---------------------------------------------------------------------------------------------
def _golden_points():
    """every member uv of the goldens, the four corners and the principal point"""
    pts = []
    for path in ct.TRI_CASES:
        g = ct.load(path)
        pts.append(np.array([p[1] for m in pickle.loads(g['matches_in']) for p in m[2:]], np.float32))
    g = ct.load(ct.TRI_CASES[0])
    w, h = g['width'], g['height']
    K = g['camera']['K_opt']
    pts.append(np.array([[0, 0], [w, 0], [0, h], [w, h], [K[2], K[5]]], np.float32))
    return np.concatenate(pts)


def _lenses():
    out = {}
    for path in ct.TRI_CASES:
        g = ct.load(path)
        K = g['camera']['K_opt']
        out[g['scene']] = (np.array([K[0], K[4], K[2], K[5]]), np.array(g['camera']['dist_opt']))
    k4 = out['dist'][0]
    out['zero'] = (k4, np.zeros(5))
    return out


@pytest.mark.parametrize('lens', ['mid', 'dist', 'zero'])
def test_undistort_equals_restatement_bit_for_bit(lens):
    k4, dist = _lenses()[lens]
    assert lens != 'dist' or np.all(dist != 0)
    pts = _golden_points()
    want = ur.undistort_points(pts, k4, dist)
    got = abi_undistort(pts, k4, dist)
    assert got.tobytes() == want.tobytes()
    for n in (1, 255, 256, 257):
        assert abi_undistort(pts[:n], k4, dist).tobytes() == want[:n].tobytes(), n
    # n == 0: no launch, the output is not touched
    assert np.all(abi_undistort(pts[:0], k4, dist) == -7.0)


def test_undistort_fallback_branch_and_python_layer():
    from imageanalysis_amd import undistort
    k4 = np.array([100.0, 100.0, 50.0, 50.0])
    dist = np.array([-1.0, 0.0, 0.01, -0.02, 0.0])              # 1 + k1 r^2 < 0 beyond r = 1
    rng = np.random.default_rng(3)
    pts = rng.uniform(-80, 180, (700, 2)).astype(np.float32)
    want = ur.undistort_points(pts, k4, dist)
    assert np.any(np.all(want == pts, axis=1)) and np.any(np.any(want != pts, axis=1))   # both branches
    assert abi_undistort(pts, k4, dist).tobytes() == want.tobytes()
    K = np.array([[100.0, 0, 50], [0, 100.0, 50], [0, 0, 1]])
    assert undistort.undistort_points(pts, K, dist).tobytes() == want.tobytes()
    assert undistort.undistort_points(pts.reshape(-1, 1, 2), K, dist).shape == (700, 1, 2)


def test_project_methods_fill_uv_list():
    from imageanalysis_amd import undistort
    g = ct.load([p for p in ct.TRI_CASES if 'dist_default' in p][0])
    proj = ct.project(g)
    K, dist = np.array(g['camera']['K']).reshape(3, 3), np.array(g['camera']['dist'])
    Ko, disto = np.array(g['camera']['K_opt']).reshape(3, 3), np.array(g['camera']['dist_opt'])

    class KP(object):
        def __init__(self, pt):
            self.pt = pt
    rng = np.random.default_rng(8)
    for k, im in enumerate(proj.image_list[:4]):
        im.kp_list = [KP((float(u), float(v))) for u, v in rng.uniform(0, 3600, (k * 130, 2))]
    undistort.undistort_keypoints(proj, optimized=True)
    for k, im in enumerate(proj.image_list[:4]):
        pts = np.array([kp.pt for kp in im.kp_list], np.float32).reshape(-1, 2)
        if k == 0:
            assert len(im.uv_list) == 0
            continue
        want = ur.undistort_points(pts, Ko, disto)
        assert isinstance(im.uv_list, np.ndarray) and im.uv_list.dtype == np.float32
        assert im.uv_list.tobytes() == want.tobytes() and len(im.uv_list) == len(pts)
        assert tuple(im.uv_list[3]) == tuple(want[3])
    im = proj.image_list[2]
    undistort.undistort_image_keypoints(proj, im)               # the initial calibration
    pts = np.array([kp.pt for kp in im.kp_list], np.float32)
    assert im.uv_list.tobytes() == ur.undistort_points(pts, K, dist).tobytes()
    got = undistort.undistort_uvlist(proj, im, [list(p) for p in pts[:7]])
    assert np.asarray(got).tobytes() == ur.undistort_points(pts[:7], K, dist).tobytes()


# ---------------------------------------------------------------------------------------------
# triangulate
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ct.TRI_CASES, ids=os.path.basename)
def test_triangulate_initial_matches_reference(path):
    g = ct.load(path)
    sc = ct.Scene(g, ct.group_of(g), 'initial')
    matches = pickle.loads(g['matches_in'])
    ref = pickle.loads(g['matches_out'])
    arrays = ct.flatten(matches)
    ned, status = abi_triangulate(sc, arrays)
    written = np.nonzero((status == WRITTEN) | (status == BELOW))[0].tolist()
    assert written == g['written']                              # no chain left out, none added
    assert int(np.sum(status == BELOW)) == g['n_whoa']
    assert set(status.tolist()) <= {UNTOUCHED, WRITTEN, BELOW}
    ptr, img = arrays[0], arrays[1]
    worst = 0.0
    for c, cond in zip(written, g['cond']):
        x_ref = np.array(ref[c][0])
        members = img[ptr[c]:ptr[c + 1]]
        members = members[sc.in_group[members] != 0]
        s = max(1.0, float(np.max(np.linalg.norm(sc.pos[members], axis=1))))
        err, bound = float(np.linalg.norm(ned[c] - x_ref)), ct.triangulate_bound(cond, s, x_ref)
        worst = max(worst, err / bound)
        assert err <= bound, (c, err, bound)
    print('worst error / bound: %.3g' % worst)
    keep = np.ones(len(matches), bool)
    keep[written] = False
    assert ned[keep].tobytes() == arrays[4][keep].tobytes()     # untouched chains: bit for bit
    # the Python layer on both chain representations writes the same positions
    from imageanalysis_amd import match_cleanup
    proj = ct.project(g)
    chains = match_cleanup.Chains.from_lists(pickle.loads(g['matches_in']))
    res = match_cleanup.triangulate_rays(proj, chains, g['groups'], ct.group_of(g))
    assert chains.untouched() and res.written.tolist() == written and len(res.below) == g['n_whoa']
    assert chains.ned.tobytes() == ned.tobytes()
    before = [m[0] for m in matches]
    res = match_cleanup.triangulate_rays(proj, matches, g['groups'], ct.group_of(g), attitude='initial')
    assert res.new.tobytes() == ned[written].tobytes()
    for c, m in enumerate(matches):
        assert m[0] == (ned[c].tolist() if not keep[c] else before[c])
    assert np.array_equal(np.nan_to_num(res.old), arrays[4][written])


@pytest.mark.parametrize('scene', ['mid', 'dist'])
def test_triangulate_optimized_matches_restatement(scene):
    from imageanalysis_amd import match_cleanup
    g = ct.load([p for p in ct.TRI_CASES if '%s_default' % scene in p][0])
    sc = ct.Scene(g, 0, 'optimized')
    matches = pickle.loads(g['matches_in'])
    want = ct.triangulate_restatement(sc, matches)
    res = match_cleanup.triangulate_rays(ct.project(g), matches, g['groups'], 0, attitude='optimized')
    assert res.written.tolist() == sorted(want) == g['written']
    for c, x in zip(res.written.tolist(), res.new):
        x_ref, cond, s, _rho = want[c]
        assert np.linalg.norm(x - x_ref) <= ct.triangulate_bound(cond, s, x_ref), c
    assert res.below.tolist() == [c for c in sorted(want) if want[c][0][2] > 0]
    # and it is not the 'initial' answer (the reference's mixed poses move the points by metres)
    ini = pickle.loads(g['matches_out'])
    assert np.median([np.linalg.norm(x - np.array(ini[c][0])) for c, x in zip(res.written.tolist(), res.new)]) > 0.1


def test_triangulate_optimized_recovers_projected_points():
    """zero distortion: points projected through the optimised poses come back within
    cond_2(r) rho 2^-12 / f per chain (rho the chain's longest ray, f the focal length): the f32
    rounding of a pixel coordinate below 8192."""
    g = ct.load([p for p in ct.TRI_CASES if 'mid_default' in p][0])
    assert not np.any(np.array(g['camera']['dist_opt']))
    sc = ct.Scene(g, 0, 'optimized')
    matches = pickle.loads(g['matches_in'])
    ref = pickle.loads(g['matches_out'])
    truth = {}
    for c in g['written']:
        X = np.array(ref[c][0])
        for m in matches[c][2:]:
            if not sc.in_group[m[0]]:
                continue
            cam = sc.R[m[0]].T.dot(X - sc.pos[m[0]])
            assert cam[2] > 1.0                                  # in front of the camera
            uvh = sc.K.dot(cam / cam[2])
            assert abs(uvh[0]) < 8192 and abs(uvh[1]) < 8192
            m[1] = [float(uvh[0]), float(uvh[1])]
        truth[c] = X
    want = ct.triangulate_restatement(sc, matches)
    ned, status = abi_triangulate(sc, ct.flatten(matches))
    assert np.nonzero((status == WRITTEN) | (status == BELOW))[0].tolist() == g['written']
    f = min(sc.k4[0], sc.k4[1])
    worst = 0.0
    for c, X in truth.items():
        _x, cond, _s, rho = want[c]
        bound = cond * rho * 2.0 ** -12 / f
        worst = max(worst, float(np.linalg.norm(ned[c] - X)) / bound)
        assert np.linalg.norm(ned[c] - X) <= bound, c
    print('worst error / bound: %.3g' % worst)


# ---------------------------------------------------------------------------------------------
# colocated
# ---------------------------------------------------------------------------------------------
def _tail(text):
    lines = text.splitlines()
    return lines[lines.index('Scanning match pair angles:'):]


@pytest.mark.parametrize('as_arrays', [False, True], ids=['lists', 'chains'])
@pytest.mark.parametrize('path', ct.COLO_CASES, ids=os.path.basename)
def test_colocated_matches_reference(path, as_arrays):
    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd.match_cleanup import Chains
    g = ct.load(path)
    proj = ct.project(g)
    matches = pickle.loads(g['matches_in'])
    if as_arrays:
        matches = Chains.from_lists(matches)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):                       # the twin script's flow from the scan on
        print("Scanning match pair angles:")
        mark_list = cull.colocated_features(proj, matches, g['groups'], g['group_index'], g['min_angle'])
        cull.mark_using_list(mark_list, matches)
        if len(mark_list) > 0:
            print('Outliers to remove from match lists:', len(mark_list))
            print('Save these changes? (y/n):', end='')
            cull.delete_marked_features(matches, g['min_chain_len'])
            print("Writing original matches:", 'matches_grouped')
    assert mark_list == [list(m) for m in g['marked']]
    assert out.getvalue().splitlines() == _tail(g['stdout'])
    if g['matches_out'] is None:
        assert not mark_list
    elif as_arrays:
        assert matches.untouched()
        assert pickle.loads(pickle.dumps(matches)) == pickle.loads(g['matches_out'])
    else:
        assert pickle.dumps(matches) == g['matches_out']


@pytest.mark.parametrize('path', [p for p in ct.COLO_CASES if '_close' in p or '_wide' in p],
                         ids=os.path.basename)
def test_pair_angle_counts_through_the_abi(path):
    g = ct.load(path)
    sc = ct.Scene(g, g['group_index'])
    arrays = ct.flatten(pickle.loads(g['matches_in']))
    count, total, status = abi_pair_angles(sc, arrays, g['min_angle'])
    assert np.array_equal(count, ct.counts_from_marks(arrays[0], g['marked']))
    assert total == len(g['marked']) == int(count.sum())
    assert np.array_equal(status == WRITTEN, arrays[3] == g['group_index'])
    assert set(status.tolist()) <= {UNTOUCHED, WRITTEN}


def test_same_image_twice_is_marked():
    g = ct.load([p for p in ct.COLO_CASES if 'dist_default' in p][0])
    sc = ct.Scene(g, 0)
    a, b = [int(i) for i in np.nonzero(sc.in_group)[0][:2]]
    f = (sc.pos[a] + sc.pos[b]) / 2 + [0, 0, 100.0]
    matches = [[f.tolist(), 0, [a, [10.0, 20.0]], [b, [30.0, 40.0]], [a, [11.0, 21.0]]]]
    count, total, status = abi_pair_angles(sc, ct.flatten(matches), 1.0)
    assert count.tolist() == [1, 0, 0] and total == 1 and status.tolist() == [WRITTEN]
    # a position ON a camera: 0 / 0 is NaN and never marks; min_angle = 180.1 marks every real angle
    matches = [[sc.pos[a].tolist(), 0, [a, [1.0, 2.0]], [b, [3.0, 4.0]], [b, [5.0, 6.0]]]]
    count, total, _ = abi_pair_angles(sc, ct.flatten(matches), 180.1)
    assert count.tolist() == [0, 1, 0] and total == 1


# ---------------------------------------------------------------------------------------------
# shapes for the two chain kernels
# ---------------------------------------------------------------------------------------------
def _shape_chains(g, sc, n_chains):
    """golden chains repeated up to n_chains, then: lengths 2, 3, 19 and 64 (members of the group, an
    image may repeat), a chain with one in-group member, a chain of another group, an ungrouped one"""
    base = [m for m in pickle.loads(g['matches_in']) if m[0] is not None]
    first = [k for k, m in enumerate(base) if m[1] == sc.group_index][0]
    base = base[first:] + base[:first]                          # (a single chain is one of the group)
    rows = [pickle.loads(pickle.dumps(base[k % len(base)])) for k in range(n_chains)]
    rng = np.random.default_rng(17)
    inside = np.nonzero(sc.in_group)[0]
    outside = np.nonzero(sc.in_group == 0)[0]
    X = np.array([40.0, 45.0, 3.0])

    def member(i, jitter=4.0):
        cam = sc.R[i].T.dot(X + rng.uniform(-jitter, jitter, 3) - sc.pos[i])
        uvh = sc.K.dot(cam / cam[2])
        return [int(i), [float(uvh[0]), float(uvh[1])]]
    if n_chains > 1:
        for length in (2, 3, 19, 64):
            rows.append([X.tolist(), sc.group_index] + [member(inside[k % len(inside)]) for k in range(length)])
        rows.append([X.tolist(), sc.group_index, member(inside[0]), member(outside[0]), member(outside[1])])
        rows.append([X.tolist(), sc.group_index + 1, member(inside[0]), member(inside[1]), member(inside[2])])
        rows.append([X.tolist(), -1, member(inside[0]), member(inside[1])])
    return rows


@pytest.mark.parametrize('n_chains', [0, 1, 257])
def test_chain_kernel_shapes(n_chains):
    g = ct.load([p for p in ct.COLO_CASES if 'dist_wide' in p][0])
    sc = ct.Scene(g, 0, 'optimized')
    rows = _shape_chains(g, sc, n_chains)
    arrays = ct.flatten(rows)
    ned, status = abi_triangulate(sc, arrays)
    count, total, pstatus = abi_pair_angles(sc, arrays, 12.0)
    if n_chains == 0:
        assert len(ned) == 0 and total == -9 and np.all(status == -9) and np.all(pstatus == -9)   # no launch
        return
    want = ct.triangulate_restatement(sc, rows)
    written = np.nonzero((status == WRITTEN) | (status == BELOW))[0].tolist()
    assert written == sorted(want)
    for c in written:
        x_ref, cond, s, _rho = want[c]
        assert np.linalg.norm(ned[c] - x_ref) <= ct.triangulate_bound(cond, s, x_ref), c
        assert (status[c] == BELOW) == (x_ref[2] > 0)
    keep = np.ones(len(rows), bool)
    keep[written] = False
    assert ned[keep].tobytes() == arrays[4][keep].tobytes() and np.all(status[keep] == UNTOUCHED)
    marks, margin, _pairs = ct.pair_angles_restatement(sc, rows, 12.0)
    assert margin > 1e-6                                         # these inputs do not sit on the decision
    assert np.array_equal(count, ct.counts_from_marks(arrays[0], marks)) and total == len(marks)
    assert np.array_equal(pstatus == WRITTEN, arrays[3] == 0)
    if n_chains > 1:
        lens = np.diff(arrays[0])[n_chains:].tolist()
        assert lens == [2, 3, 19, 64, 3, 3, 2]
        assert status[n_chains:].tolist()[4:] == [UNTOUCHED] * 3 and all(c in want for c in range(n_chains, n_chains + 4))
        assert count[arrays[0][n_chains + 3]:arrays[0][n_chains + 4]].max() > 1     # the 64-member chain


def test_out_of_range_image_index():
    from imageanalysis_amd import match_cleanup
    from imageanalysis_amd import match_culling as cull
    g = ct.load([p for p in ct.COLO_CASES if 'dist_wide' in p][0])
    sc = ct.Scene(g, 0)
    n_img = len(sc.pos)
    rows = pickle.loads(g['matches_in'])
    ks = [i for i, m in enumerate(rows) if m[1] == 0][:3]
    rows[ks[0]][3][0] = n_img                                   # one past the end
    rows[ks[1]][2][0] = -1                                      # negative
    rows[ks[2]][-1][0] = 2 ** 31 - 1                            # far away
    other = [i for i, m in enumerate(rows) if m[1] != 0][0]
    rows[other][2][0] = 10 ** 6                                 # another group's chain is never looked at
    arrays = ct.flatten(rows)
    ned, status = abi_triangulate(sc, arrays)
    count, total, pstatus = abi_pair_angles(sc, arrays, 12.0)
    for k in ks:
        assert status[k] == BAD_IMAGE and pstatus[k] == BAD_IMAGE
        assert ned[k].tobytes() == arrays[4][k].tobytes()
        assert not count[arrays[0][k]:arrays[0][k + 1]].any()
    assert status[other] == UNTOUCHED and pstatus[other] == UNTOUCHED
    assert int(np.sum(status == BAD_IMAGE)) == 3 and total == int(count.sum())
    proj = ct.project(g)
    with pytest.raises(IndexError, match='chain %d refers to image %d' % (ks[0], n_img)):
        match_cleanup.triangulate_rays(proj, rows, g['groups'], 0)
    with pytest.raises(IndexError, match='chain %d refers to image %d' % (ks[0], n_img)):
        cull.colocated_features(proj, rows, g['groups'], 0, 12.0)
    assert rows[ks[0]][0] == arrays[4][ks[0]].tolist()          # nothing was written back


def test_zero_pivot_raises_linalg_error():
    from imageanalysis_amd import match_cleanup
    from imageanalysis_amd.hostlib import camera
    from imageanalysis_amd.hostlib.image_pose import PoseProject
    g = ct.load([p for p in ct.TRI_CASES if 'dist_default' in p][0])
    sc = ct.Scene(g, 0)
    rows = pickle.loads(g['matches_in'])
    k = g['written'][2]
    # a NaN observation: r is NaN, not singular -- numpy.linalg.solve answers NaN, and so does the kernel
    rows[k][2][1] = [float('nan'), 0.0]
    ned, status = abi_triangulate(sc, ct.flatten(rows))
    assert status[k] in (WRITTEN, BELOW) and np.isnan(ned[k]).all()
    # two level cameras looking along the same axis through their principal points: every ray is
    # exactly (1, 0, 0), r = 2 (I - e e^T) = diag(0, 2, 2), the first pivot is exactly zero.  All the
    # numbers on the way are exact in binary (f = 1024, c = (2048, 1024), identity attitude).
    proj = PoseProject(['SINGULAR_A', 'SINGULAR_B'])
    for im, ned0 in zip(proj.image_list, ([0.0, 0.0, -100.0], [0.0, 30.0, -100.0])):
        im.set_camera_pose(ned0, 0.0, 0.0, 0.0)
        im.set_camera_pose(ned0, 0.0, 0.0, 0.0, opt=True)
    camera.set_K(1024.0, 1024.0, 2048.0, 1024.0)
    camera.set_K(1024.0, 1024.0, 2048.0, 1024.0, optimized=True)
    camera.set_dist_coeffs([0.0] * 5)
    camera.set_dist_coeffs([0.0] * 5, optimized=True)
    chains = [[[1.0, 2.0, 3.0], 0, [0, [2048.0, 1024.0]], [1, [2048.0, 1024.0]]],
              [None, 0, [0, [2048.0, 1024.0]], [1, [1000.0, 1024.0]]]]
    with pytest.raises(np.linalg.LinAlgError, match='chain 0'):
        match_cleanup.triangulate_rays(proj, chains, [['SINGULAR_A', 'SINGULAR_B']], 0)
    assert chains[0][0] == [1.0, 2.0, 3.0] and chains[1][0] is None      # nothing written back
    with pytest.raises(np.linalg.LinAlgError):                           # and numpy says the same
        np.linalg.solve(np.diag([0.0, 2.0, 2.0]), np.zeros(3))
    M = np.identity(3).dot(ct.CAM2BODY).dot(np.linalg.inv(camera.get_K(True))).ravel()
    sc2 = types.SimpleNamespace(M=np.tile(M, (2, 1)), pos=np.array([[0.0, 0.0, -100.0], [0.0, 30.0, -100.0]]),
                                in_group=np.ones(2, np.uint8), group_index=0,
                                k4=np.array([1024.0, 1024.0, 2048.0, 1024.0]), dist=np.zeros(5))
    ned, status = abi_triangulate(sc2, ct.flatten(chains))
    assert status.tolist() == [SINGULAR, WRITTEN] and ned[0].tolist() == [1.0, 2.0, 3.0]


# ---------------------------------------------------------------------------------------------
# the script twins, run the way a user runs them (stand-ins for the reference's lib.project / lib.groups)
# ---------------------------------------------------------------------------------------------
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


def _run_twin(script, g, tmp_path, argv, answer='y\n'):
    lib = tmp_path / 'standin' / 'lib'
    lib.mkdir(parents=True)
    for name, text in LIB_STANDIN.items():
        (lib / name).write_text(text)
    proj = tmp_path / 'project'
    (proj / 'ImageAnalysis').mkdir(parents=True)
    (proj / 'ImageAnalysis' / 'matches_grouped').write_bytes(g['matches_in'])
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


def test_colocated_twin_script_equals_reference(tmp_path):
    g = ct.load([p for p in ct.COLO_CASES if 'dist_close' in p][0])
    stdout, written = _run_twin('4b-colocated-feats.py', g, tmp_path, g['argv'])
    assert written == g['matches_out']
    ours, theirs = stdout.splitlines(), g['stdout'].splitlines()
    at = 'Notice: min_chain_len is: 3'                          # (what comes before is ProjectMgr's own)
    assert ours[ours.index(at):] == theirs[theirs.index(at):]


def test_triangulation_twin_script(tmp_path):
    g = ct.load([p for p in ct.TRI_CASES if 'dist_default' in p][0])
    stdout, written = _run_twin('3c-match-triangulation.py', g, tmp_path,
                                ['--method', 'triangulate', '--verbose'] + g['argv'])
    ours, ref = pickle.loads(written), pickle.loads(g['matches_out'])
    assert len(ours) == len(ref)
    sc = ct.Scene(g, 0)
    for c, (a, b) in enumerate(zip(ours, ref)):
        if c in g['written']:
            assert np.linalg.norm(np.array(a[0]) - np.array(b[0])) <= ct.triangulate_bound(
                g['cond'][g['written'].index(c)], max(1.0, float(np.max(np.linalg.norm(sc.pos, axis=1)))), np.array(b[0]))
            assert a[1:] == b[1:]
        else:
            assert a == b
    lines = stdout.splitlines()
    assert 'Chains written: %d WHOA! (below the ground plane): %d' % (len(g['written']), g['n_whoa']) in lines
    assert [int(l.split()[0]) for l in lines if '>>>' in l] == g['written']
    assert sum(l.endswith('>>> WHOA!') for l in lines) == g['n_whoa']
    assert any('INITIAL attitudes' in l for l in lines)         # it says what it does
    assert lines[-1] == 'Writing: matches_grouped'
