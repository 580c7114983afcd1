"""The 'smart' strategy without a GPU: the numpy restatement (tests/smart_reference.py) against the
goldens of the reference's own smart_pair_matches / find_matches(strategy='smart')
(tools/gen_smart_golden.py), the pose prior and the pair loop of the package with the device part
replaced by the restatement inside the test, and the argument checks of the new entry points."""
import ctypes

import numpy as np
import pytest

import smart_reference as sr
from conftest import GOLDEN

PAIR_GOLDENS = sr.PAIR_CASES + ('guards',)


@pytest.mark.parametrize('name', PAIR_GOLDENS)
def test_restatement_equals_golden(name):
    g = sr.load_golden(name)
    res = sr.restate(g, sr.host_ransac(g['hypotheses'], g['seed']))
    assert len(res) == len(g['results'])
    for got, want in zip(res, g['results']):
        assert np.array_equal(got['fwd'], want['fwd']) and np.array_equal(got['rev'], want['rev'])
        assert len(got['passes']) == len(want['passes'])
        for a, b in zip(got['passes'], want['passes']):
            assert np.array_equal(a['stats'], b['stats']) and a['taken'] == b['taken']


def test_the_zero_case_raises_in_the_reference_and_in_the_restatement():
    g = sr.load_golden('zero')
    assert 'division by zero' in g['results'][0]['raised']
    with pytest.raises(ZeroDivisionError):
        sr.restate(g, sr.host_ransac(g['hypotheses'], g['seed']))


def test_goldens_show_what_their_names_say():
    res = {n: sr.load_golden(n)['results'] for n in PAIR_GOLDENS}
    taken = lambda r: [p['taken'] for p in r['passes']]
    assert taken(res['clean'][0]) == [1, 0] and len(res['clean'][0]['fwd']) == 300
    two = res['two_pass'][0]
    assert len(two['passes']) >= 3 and taken(two)[0] > taken(two)[1] > 0 == taken(two)[-1]
    assert two['passes'][1]['stats'][:, 2].max() > two['passes'][0]['stats'][:, 2].max() > 20
    # second_nn: the true match is neighbour 2 or 3 of 60 rows, which the nearest neighbour alone loses
    g = sr.load_golden('second_nn')
    p, fwd = g['pairs'][0], res['second_nn'][0]['fwd']
    idx, _d2 = sr.knn3_exact(p['des1'], p['des2'])
    col = np.array([list(idx[q]).index(t) for q, t in fwd])
    assert (col == 1).sum() >= 30 and (col == 2).sum() >= 15 and (col == 0).sum() == 30
    # sizes: exactly 1.25 kept, the next float32 above passed over
    g = sr.load_golden('sizes')
    p, fwd = g['pairs'][0], res['sizes'][0]['fwd']
    ratio = p['size2'][fwd[:, 1]].astype(np.float64) / p['size1'][fwd[:, 0]]
    assert (ratio == 1.25).sum() == 20 and ratio.max() == 1.25 and len(fwd) == 80
    first = sr.knn3_exact(p['des1'], p['des2'])[0][:, 0]
    above = p['size2'][first].astype(np.float64) / p['size1']
    assert ((above > 1.25) & (above < 1.2500002)).sum() == 40
    # cuts: 89999 looked at and 90000 not; 150 / 200 is not below 0.75, 150 / sqrt(40001) is
    g = sr.load_golden('cuts')
    p, fwd = g['pairs'][0], res['cuts'][0]['fwd']
    idx, d2 = sr.knn3_exact(p['des1'], p['des2'])
    got = {int(q): int(d2[q][list(idx[q]).index(t)]) for q, t in fwd}
    assert sorted(set(got.values()) & {89999, 90000, 40000, 40001}) == [40000, 89999]
    assert list(got.values()).count(89999) == 15 and list(got.values()).count(40000) == 10
    assert len(res['below20'][0]['fwd']) == 0 and res['below20'][0]['passes'][0]['stats'][:, 2].max() == 20
    assert len(res['twentyone'][0]['fwd']) == 21
    a, b = res['gates']
    assert a['passes'][0]['stats'][0].tolist() == [26, 26, 23] and taken(a) == [1, 0] and not len(a['fwd'])
    assert b['passes'][0]['stats'][3].tolist() == [27, 22, 22] and taken(b) == [4, 0] and not len(b['fwd'])
    d = res['dups'][0]
    assert d['passes'][0]['stats'][0].tolist() == [66, 66, 60] and len(d['fwd']) == 60
    assert len(sr.load_golden('two_rows')['pairs'][0]['des2']) == 2 and not len(res['two_rows'][0]['fwd'])
    shapes = [(None if p['des1'] is None else len(p['des1']), None if p['des2'] is None else len(p['des2']))
              for p in sr.load_golden('guards')['pairs']]
    assert shapes == [(0, 87), (29, 0), (1, 87), (29, 1), (None, 87), (29, None)]
    assert all(not len(r['fwd']) and not r['passes'] for r in res['guards'])


def test_constants_agree():
    from imageanalysis_amd import kernels, matcher
    assert list(matcher.SMART_CUTOFFS) == list(kernels.SMART_CUTOFFS) == sr.CUTOFFS
    assert matcher.SMART_MIN_UNIQUE == kernels.SMART_MIN_UNIQUE == sr.MIN_UNIQUE == 20
    assert (kernels.FIT_OK, kernels.FIT_TOO_FEW, kernels.FIT_DEGENERATE) == (sr.FIT_OK, sr.FIT_TOO_FEW, sr.FIT_DEGENERATE)
    assert np.array_equal(matcher.gen_grid(sr.W_PX, sr.H_PX, 8),
                          [[u, v] for v in np.linspace(0, sr.H_PX, 9) for u in np.linspace(0, sr.W_PX, 9)])


def test_restated_fit_against_its_longdouble_form():
    """the float64 fit stays within a millionth of a pixel of the same rule in longdouble, over the
    segment sizes the device test uses"""
    for n, seed in ((4, 41), (5, 42), (81, 45), (2049, 43)):
        pts = sr.vr.scene(n, 1.0, 0.0, seed)[0]
        H64, s64 = sr.fit(pts)
        Hld, sld = sr.fit(pts, dtype=np.longdouble)
        assert s64 == sld == sr.FIT_OK and H64[2, 2] == 1.0
        assert sr.transfer_error(H64, Hld, pts) < 1e-9
    assert sr.fit(pts[:3])[1] == sr.FIT_TOO_FEW and sr.fit(sr.vr.identical(9))[1] == sr.FIT_DEGENERATE


# ---------------------------------------------------------------------------------------------
# the package's prior and pair loop, the device part replaced by the restatement
# ---------------------------------------------------------------------------------------------
class _Kp(object):
    __slots__ = ('pt', 'size')

    def __init__(self, x, y, s):
        self.pt, self.size = (float(x), float(y)), float(s)


def attach(im, des, xy, size):
    im.des_list = None if des is None else np.asarray(des).astype(np.float32)
    im.kp_list = [_Kp(x, y, s) for (x, y), s in zip(np.asarray(xy, np.float32), np.asarray(size, np.float32))]


def pose_pair(pose, min_pairs=25, names=('A', 'B'), K=None):
    """two PoseImages with a golden's poses, the camera and the matcher nodes set as the generator does"""
    from imageanalysis_amd import matcher, smart
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd.hostlib import camera
    from imageanalysis_amd.hostlib.image_pose import PoseImage
    for n_ in list(getNode('/images', True).__dict__):
        del getNode('/images', True).__dict__[n_]
    smart.smart_node.__dict__.clear()
    smart.load(None)
    K = sr.vr.KMAT if K is None else K
    camera.set_K(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    camera.set_dist_coeffs([0.0, 0.0, 0.0, 0.0, 0.0])
    camera.set_image_params(sr.W_PX, sr.H_PX)
    camera.set_mount_params(0.0, -90.0, 0.0)
    matcher.detector_node.setString('detector', 'SIFT')
    matcher.detector_node.setFloat('scale', 0.4)
    matcher.matcher_node.__dict__.pop('ground_m', None)
    matcher.matcher_node.setFloat('match_ratio', sr.MATCH_RATIO)
    matcher.matcher_node.setInt('min_pairs', int(min_pairs))
    out = []
    for k, n_ in enumerate(names):
        im = PoseImage(n_)
        im.set_camera_pose(pose['ned%d' % (k + 1)], *pose['ypr%d' % (k + 1)])
        node = smart.smart_node.getChild(n_, True)
        node.setFloat('srtm_surface_m', pose['srtm'][k])
        if pose['yaw_error'][k] != 0.0:
            node.setFloat('yaw_error', pose['yaw_error'][k])
        out.append(im)
    if pose['forced_ground'] is not None:
        matcher.matcher_node.setFloat('ground_m', pose['forced_ground'])
    return out


@pytest.fixture
def host_hooks():
    """matcher's two module-level hooks set to the restatement, and everything they touch put back"""
    from imageanalysis_amd import matcher
    saved = {n: getattr(matcher, n) for n in ('smart_pair_hook', 'smart_prior_fit', 'the_matcher', 'max_distance',
                                                'min_pairs')}

    def fit(pts):
        H, st = sr.fit(pts)
        assert st == sr.FIT_OK
        return H

    def pair(i1, i2, H0, tol, match_ratio, hypotheses, seed):
        xy1, xy2 = matcher._kp_xy(i1), matcher._kp_xy(i2)
        idx, d2 = sr.knn3_exact(np.asarray(i1.des_list), np.asarray(i2.des_list))
        flag = np.zeros(2, np.int32)
        try:
            r = sr.smart_pair(idx, d2, xy1, xy2, matcher._kp_size(i1), matcher._kp_size(i2), len(xy1), len(xy2), H0,
                              tol, matcher.min_pairs, sr.host_ransac(hypotheses, seed, lean=True), match_ratio)
        except ZeroDivisionError:
            flag[0] = 1
            return np.zeros((0, 2), np.int32), [], [], flag, H0
        return r['fwd'], [p['stats'] for p in r['passes']], [p['taken'] for p in r['passes']], flag, r['H']
    matcher.smart_pair_hook, matcher.smart_prior_fit = pair, fit
    matcher.the_matcher = object()                    # configure() needs the GPU
    yield matcher
    for n, v in saved.items():
        setattr(matcher, n, v)
    matcher.matcher_node.__dict__.pop('ground_m', None)


def test_smart_prior_equals_the_reference_at_its_corners(host_hooks):
    """reproj within 1e-6 px of what the reference's own projectPoints call returned (the generator's
    recorded float64-vs-longdouble noise of the FIT is at most 1.2e-8 px and does not enter reproj),
    H0 as a transfer error over the 81 reprojected points"""
    matcher = host_hooks
    g = sr.load_golden('prior_edges')
    assert [e['what'] for e in g['edges']] == [w for w, _p in sr.prior_edges()]
    for e in g['edges']:
        i1, i2 = pose_pair(e['pose'])
        H0, ground_m, reproj = matcher.smart_prior(i1, i2, est_rotation=True)
        assert np.abs(reproj - e['reproj']).max() <= 1e-6, e['what']
        assert sr.transfer_error(H0, e['H0'], e['reproj']) <= max(1e-6, 1000 * e['noise']), e['what']
    by = {e['what']: e for e in g['edges']}
    i1, i2 = pose_pair(by['camera below the ground estimate']['pose'])
    assert matcher.smart_prior(i1, i2, True)[1] == -float(i2.get_camera_pose()[0][2]) - 2
    i1, i2 = pose_pair(by['forced ground']['pose'])
    assert matcher.smart_prior(i1, i2, True)[1] == -90.0
    i1, i2 = pose_pair(by['plain']['pose'])
    assert matcher.smart_prior(i1, i2, True)[1] == sr.GROUND_M
    # without est_rotation the yaw-error estimates are not applied
    i1, i2 = pose_pair(by['both have one']['pose'])
    assert np.abs(matcher.smart_prior(i1, i2, False)[2] - by['plain']['reproj']).max() < 1e-6
    assert np.abs(matcher.smart_prior(i1, i2, True)[2] - by['plain']['reproj']).max() > 10


@pytest.mark.parametrize('name', ['two_pass', 'gates', 'guards', 'zero'])
def test_smart_pair_matches_host_logic_equals_golden(host_hooks, name):
    matcher = host_hooks
    g = sr.load_golden(name)
    for p, want in zip(g['pairs'], g['results']):
        i1, i2 = pose_pair(p['pose'], g['min_pairs'])
        matcher.min_pairs = float(g['min_pairs'])
        attach(i1, p['des1'], p['xy1'], p['size1'])
        attach(i2, p['des2'], p['xy2'], p['size2'])
        if want['raised']:
            with pytest.raises(ZeroDivisionError):
                matcher.smart_pair_matches(i1, i2, False, True, hypotheses=g['hypotheses'], seed=g['seed'])
            continue
        fwd, rev = matcher.smart_pair_matches(i1, i2, False, True, hypotheses=g['hypotheses'], seed=g['seed'])
        assert np.array_equal(np.asarray(fwd, np.int32).reshape(-1, 2), want['fwd'])
        assert np.array_equal(np.asarray(rev, np.int32).reshape(-1, 2), want['rev'])
        if want['passes']:
            assert matcher.smart_last['passes'] == len(want['passes'])
            assert matcher.smart_last['taken'] == [q['taken'] for q in want['passes']]
            assert sr.transfer_error(matcher.smart_last['H0'], want['H0'], want['reproj']) < 1e-6


def strip_project(device):
    """the project of find_matches_strip.pkl with the keypoint sizes and the ground of smart_strip"""
    import pickle
    import os
    from imageanalysis_amd import matcher, smart
    from imageanalysis_amd.hostlib import camera
    import test_find_matches_loop as loop
    with open(os.path.join(GOLDEN, 'find_matches_strip.pkl'), 'rb') as f:
        g = pickle.load(f)
    s = sr.load_golden('strip')
    proj = loop.make_project(g, device)
    camera.set_dist_coeffs([0.0, 0.0, 0.0, 0.0, 0.0])
    matcher.matcher_node.__dict__.pop('ground_m', None)
    for im, des, xy, size in zip(proj.image_list, g['des'], g['xy'], s['sizes']):
        attach(im, des, xy, size)
        smart.smart_node.getChild(im.name, True).setFloat('srtm_surface_m', s['srtm_surface_m'])
    return g, s, proj, loop


def test_smart_matches_equals_the_reference_loop_host_logic(host_hooks, monkeypatch):
    """the pair loop of the package -- schedule, skip / retry, the prior from the poses and the /smart
    tree every earlier pair left, the feedback, the discard rule -- against the reference's
    find_matches(strategy='smart') on the strip, sort=False and a second call; the pair function, the
    triangulation and the similarity fit are oracle restatements inside the test.  sort=True is left
    to the device test (test_match_smart_gpu.py runs both orders): the order only changes which list
    _work_list hands over, which tests/test_find_matches_loop.py checks on the host for both, and one
    order costs 17 s of numpy consensus at 2048 hypotheses here."""
    from imageanalysis_amd import smart
    from imageanalysis_amd.hostlib import camera
    from oracle import smart_oracle
    matcher = host_hooks
    g, s, proj, loop = strip_project(device=False)
    matcher.min_pairs = float(g['min_pairs'])

    def triangulate_down(i1, i2, pairs):
        pr = np.asarray(pairs, np.int64).reshape(-1, 2)
        return smart_oracle.triangulate_down(smart.projection_matrix(i1), smart.projection_matrix(i2),
                                             camera.get_K(), matcher._kp_xy(i1)[pr[:, 0]], matcher._kp_xy(i2)[pr[:, 1]])

    def find_affine(i1, i2):
        if i1 == i2 or i2.name not in i1.match_list or len(i1.match_list[i2.name]) == 0:
            return None
        pr = np.asarray(i1.match_list[i2.name], np.int64).reshape(-1, 2)
        return smart_oracle.fit_similarity(matcher._kp_xy(i2)[pr[:, 1]], matcher._kp_xy(i1)[pr[:, 0]])
    monkeypatch.setattr(smart, 'triangulate_down', triangulate_down)
    monkeypatch.setattr(smart, 'find_affine', find_affine)
    for call in range(2):
        matcher.smart_matches(proj, None, sort=False)
        loop.check_against(g, s['runs'][False], call, proj)


# ---------------------------------------------------------------------------------------------
# the C ABI without a GPU
# ---------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    for name in ('iamx_knn3_l2_pairs', 'iamx_homography_fit', 'iamx_smart_stats', 'iamx_smart_select'):
        assert name in _lib.SIGNATURES and getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    assert '#define IAMX_SMART_BINS 7' in text and len(sr.CUTOFFS) == 7


def test_new_entries_check_their_arguments_without_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                  # (a 16-byte aligned address that is never read)
    assert p.value % 16 == 0
    call = lambda fn, spec, kw: fn(*[kw.get(k, d) for k, d in spec])
    knn3 = (('desc', p), ('norm_q', p), ('norm_t', p), ('img_off', p), ('img_n', p), ('pairs', p), ('wg_off', p),
            ('out_off', p), ('n_pairs', 1), ('total_wg', 1), ('out_idx', p), ('out_d2', p), ('stream', None))
    fit = (('pts', p), ('seg_off', p), ('mask', p), ('n_seg', 1), ('total', 4), ('H', p), ('status', p), ('stream', None))
    stats = (('idx', p), ('d2', p), ('row_off', p), ('pairs', p), ('kp_off', p), ('xy', p), ('size', p), ('H', p),
             ('active', p), ('n_pairs', 1), ('match_ratio', 0.75), ('min_pairs', 25.0), ('cap', 7), ('bin_cnt', p),
             ('seg_cnt', p), ('seg_off', p), ('pts', p), ('rows', p), ('flag', p), ('stream', None))
    select = (('pairs', p), ('kp_off', p), ('key2', p), ('active', p), ('n_pairs', 1), ('min_pairs', 25.0),
              ('bin_cnt', p), ('seg_cnt', p), ('seg_off', p), ('pts', p), ('rows', p), ('mask', p), ('vstatus', p),
              ('vmodel', p), ('cap', 7), ('stride', 1), ('tab_size', 64), ('work', p), ('best', p), ('improved', p),
              ('out_slots', p), ('out_cnt', p), ('out_off', p), ('out_rows', p), ('out_cap', 1), ('stats', p),
              ('H', p), ('fit_status', p), ('flag', p), ('stream', None))
    optional = {'mask', 'active', 'stream'}
    for fn, spec in ((L.iamx_knn3_l2_pairs, knn3), (L.iamx_homography_fit, fit), (L.iamx_smart_stats, stats),
                     (L.iamx_smart_select, select)):
        for name, d in spec:
            if d is p and name not in optional:
                assert call(fn, spec, {name: None}) == -1 and b'null pointer' in L.iamx_last_error(), name
        counts = [name for name, d in spec if isinstance(d, int) and name not in ('stride', 'tab_size')]
        for name in counts:
            assert call(fn, spec, {name: -1}) == -1, name
    odd = ctypes.c_void_p(p.value + 4)
    assert call(L.iamx_homography_fit, fit, {'pts': odd}) == -1 and b'aligned' in L.iamx_last_error()
    assert call(L.iamx_smart_stats, stats, {'pts': odd}) == -1 and call(L.iamx_smart_select, select, {'pts': odd}) == -1
    assert call(L.iamx_smart_stats, stats, {'match_ratio': float('nan')}) == -1
    sel = lambda **kw: call(L.iamx_smart_select, select, kw)
    assert sel(stride=0) == -1 and sel(tab_size=48) == -1 and sel(stride=64, tab_size=64) == -1
    assert sel(stride=(1 << 24) + 1, tab_size=1 << 26) == -1
    # nothing to do: no launch, no device needed
    assert call(L.iamx_knn3_l2_pairs, knn3, {'n_pairs': 0}) == 0 and call(L.iamx_homography_fit, fit, {'n_seg': 0}) == 0
    assert call(L.iamx_smart_stats, stats, {'n_pairs': 0}) == 0
