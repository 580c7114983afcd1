"""Host: the inputs of tests/test_pair_geometry_gpu.py are fair, and the float64 oracles
(oracle/smart_oracle.triangulate_down, fit_similarity) sit where the high-precision references of
tests/pair_geometry_reference.py say they should.

Measured here (numpy 80-bit longdouble, mpmath at 60 digits):

* similarity: the smallest |residual - threshold| over all cases, directions and re-fits is
  0.78 px (the condition is 1e-6 px); fit_similarity's error against longdouble is at most
  2.7e-16 (rotation/scale entries, translations over the largest coordinate).
* DLT: sigma3/sigma4 is at least 1.2e3 and |X_3| / ||X|| at least 9.9e-5 in the asserted
  families.  numpy's SVD (triangulate_down) is off by |z - z_ref| of 1.4e-12 m (nominal),
  2.1e-10 m (1e3 m from the origin), 1.6e-8 m (1e4 m), 6.2e-10 m (0.05 m baseline), 5.3e-12 m
  (oblique); its ||A x|| / ||x|| / sigma4 - 1 is 3.4e-15, 2.7e-9, 5.9e-5, 1.2e-9, 4.0e-15.
  At 1e5 m and 1e6 m (printed, not asserted): 1.3e-6 m and 9.6e-5 m, ratio - 1 of 0.58 and 77.
"""
import numpy as np
import pytest

import pair_geometry_reference as ref
from oracle.smart_oracle import triangulate_down

ASSERTED = [n for n, f in ref.FAMILIES.items() if f[3]]
PRINTED = [n for n, f in ref.FAMILIES.items() if not f[3]]


# ---- similarity ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.SIZE_CASES + ref.EDGE_CASES)
def test_similarity_inputs_are_clear_of_the_thresholds(name):
    """No residual of the longdouble reference lies within 1e-6 px of its re-fit's threshold, so
    no rounding of a float64 implementation can move a match across it; and the longdouble inlier
    sets are fit_similarity's at every re-fit.  (A condition on the inputs: the seeds of
    pair_geometry_reference were chosen so that it holds.)"""
    r = ref.similarity_reference(name)
    frm_to = ((r['b'], r['a']), (r['a'], r['b']))
    for d in (0, 1):
        tr, tr64 = r['trace'][d], r['trace64'][d]
        assert len(tr) == len(tr64)
        for k, (t, t64) in enumerate(zip(tr, tr64)):
            print('%s dir %d re-fit %d: %d inliers, margin %.3g px' % (name, d, k + 1, t['inliers'].sum(), t['margin']))
            assert t['margin'] >= 1e-6
            assert np.array_equal(t['inliers'], t64['inliers']) and t['fitted'] == t64['fitted']
        # the float64 trace IS fit_similarity
        M64 = ref.similarity_trace(*frm_to[d], dtype=np.float64)[0]
        if r['oracle'][d] is None:
            assert M64 is None and r['M_ref'][d] is None
        else:
            assert np.array_equal(M64, r['oracle'][d])


@pytest.mark.parametrize('name', ref.SIZE_CASES + ref.EDGE_CASES)
def test_fit_similarity_against_longdouble(name):
    """fit_similarity's own error, the yardstick of the device's: below the floor 64 . 2^-52"""
    r = ref.similarity_reference(name)
    for d in (0, 1):
        if r['M_ref'][d] is None:
            assert r['oracle'][d] is None
            continue
        print('%s dir %d: fit_similarity error %.3g' % (name, d, r['oracle_err'][d]))
        assert r['oracle_err'][d] <= ref.SIM_FLOOR


def test_edge_cases_are_what_they_are_named_for():
    R = ref.similarity_reference
    assert len(R('none')['a']) == 0 and R('none')['M_ref'] == [None, None]
    assert len(R('one')['a']) == 1 and R('one')['M_ref'] == [None, None]
    assert len(R('one_nan')['a']) == 1 and np.isnan(R('one_nan')['a']).all() and R('one_nan')['M_ref'] == [None, None]
    # two distinct matches: the similarity through two points
    two = R('two')
    a, b = two['a'], two['b']
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(b[0], b[1])
    for d, (p, q) in enumerate(((b, a), (a, b))):
        M2 = ref.two_point_similarity(p[0], p[1], q[0], q[1])
        assert ref.similarity_error(two['M_ref'][d], M2, two['scale']) < 1e-17
    # b's points identical: no fit from b, a = b = 0 and the centroid from a
    bi = R('b_identical')
    assert bi['M_ref'][0] is None and bi['oracle'][0] is None
    M = np.asarray(bi['oracle'][1])
    assert np.array_equal(M[:, :2], np.zeros((2, 2))) and np.allclose(M[:, 2], bi['b'][0], rtol=1e-15)
    assert len(np.unique(bi['a'], axis=0)) == 5


def test_dry_schedule_runs_dry_on_the_reference():
    """the hand-built set loses its second-to-last inlier at a re-fit k in 2..9 (k = 3: all five
    at 200 px, four at 50 px, none at 10 px), in both directions; the model that stands is re-fit
    k - 1's, which is neither the first fit nor the one before"""
    r = ref.similarity_reference('dry')
    for d, (p, q) in enumerate(((r['b'], r['a']), (r['a'], r['b']))):
        tr = r['trace'][d]
        k = len(tr)
        assert 2 <= k <= 9 and not tr[-1]['fitted'] and tr[-1]['inliers'].sum() < 2
        assert all(t['fitted'] for t in tr[:-1])
        assert [int(t['inliers'].sum()) for t in tr] == [5, 4, 0]
        first = ref._fit(p.astype(np.longdouble), q.astype(np.longdouble), np.ones(5, np.longdouble))
        assert ref.similarity_error(first, r['M_ref'][d], r['scale']) > 1e-4


# ---- DLT ----------------------------------------------------------------------------------------
def _family_figures(name):
    r = ref.family_reference(name)
    cond = np.array([float(a / b) for a, b in zip(r['sig3'], r['sig4'])])
    zerr = np.abs(r['svd_xyz'][:, 2] - r['xyz_ref'][:, 2])
    print('%s: sigma3/sigma4 >= %.3g, |X3|/||X|| >= %.3g, numpy SVD |z - z_ref| <= %.3g m, '
          'ratio - 1 <= %.3g' % (name, cond.min(), r['w_ref'].min(), zerr.max(), r['svd_ratio_m1'].max()))
    return r, cond, zerr


@pytest.mark.parametrize('name', ASSERTED)
def test_triangulation_family_is_well_posed(name):
    """a well-defined null direction (sigma3/sigma4 >= 1e3) and no point at infinity
    (|X_3| / ||X|| >= 1e-6) for every match of every asserted family"""
    r, cond, _ = _family_figures(name)
    assert len(cond) == ref.MP_MAX
    assert cond.min() >= 1e3
    assert r['w_ref'].min() >= 1e-6


@pytest.mark.parametrize('name', ['launch'] + ['packed%d' % t for t in ref.PACKED_TOTALS])
def test_triangulation_launch_cases_are_well_posed(name):
    """the same two conditions for the launch-geometry and the packed cases (float64 singular
    values: these go beyond the mpmath budget), and the launch shapes the GPU tests rely on"""
    if name == 'launch':
        c = ref.launch_case()
        PR = c['PROJ'].reshape(-1, 3, 4)
        mats = [(PR[a], PR[b]) for a, b in c['pair_img']]
        sizes = np.diff(c['arena'].kp_off)
        assert len(set(sizes)) == 6                                   # six images of different sizes
        used = [r_[:, 0].max() for r_, (a, b) in zip(c['rows'], c['pair_img']) if len(r_) and sizes[a] - 1 == r_[:, 0].max()]
        assert used                                                   # an image's last keypoint is referenced
        flat = [tuple(p) for p in c['pair_img']]
        assert (4, 1) in flat and (1, 4) in flat and sum(4 in p for p in flat) >= 3
        assert c['m_cnt'].tolist() == [0, 1, 256, 257, 300] and c['m_pairs'].shape[1] == 300
    else:
        c = ref.packed_case(int(name[6:]))
        mats = [(P[0].reshape(3, 4), P[1].reshape(3, 4)) for P in c['pair_proj']]
        cnt = np.diff(c['m_off'])
        assert cnt[0] == 0 and cnt[-1] == 0 and np.any((cnt[1:-2] == 0) & (cnt[2:-1] == 0))
    ar = c['arena']
    assert np.isnan(ar.xy[ar.poison_row]).all() and np.isnan(ar.xy).sum() == 2
    assert len(ar.xy) >= ar.kp_off[:-1].max() + np.diff(ar.kp_off).max()
    for (P1, P2), (a, b), rows in zip(mats, c['pair_img'], c['rows']):
        if not len(rows):
            continue
        uv1, uv2 = ar.kp[a][rows[:, 0]], ar.kp[b][rows[:, 1]]
        _xyz, _bound, cond, w = ref.svd_bounds(P1, P2, uv1, uv2)
        assert cond.min() >= 1e3 and w.min() >= 1e-6


@pytest.mark.parametrize('name', ASSERTED + PRINTED)
def test_triangulate_down_against_mpmath(name):
    """triangulate_down (numpy's SVD) against the 60-digit null vector: its |z - z_ref| stays
    inside the first-order bound 64 eps . sigma3/sigma4 . scale, and its figures are the
    yardstick the device is held to (test_pair_geometry_gpu.py)"""
    r, _cond, zerr = _family_figures(name)
    z = triangulate_down(r['P1'], r['P2'], ref.K, r['uv1'], r['uv2'])
    assert np.array_equal(z, r['svd_xyz'][:, 2])
    bound = np.array([ref.z_bound(r['sig3'][i], r['sig4'][i], r['xyz_ref'][i]) for i in range(len(z))])
    assert np.all(zerr <= bound)
    assert np.all(r['svd_ratio_m1'] > -1e-30)        # nothing beats the null direction


# ---- ground -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_feat', ref.GROUND_SIZES)
def test_ground_restatement(n_feat):
    """the ordered float64 restatement against the same means in longdouble; the sky rays are
    the pitched-up camera's, count in the divisor, and a feature seen by them alone is (0, 0, 0)"""
    c = ref.ground_case(n_feat)
    out, n_sky = ref.ground_ordered(c['M'], c['ned'], c['base'], c['obs_img'], c['obs_uv'], c['feat_ptr'])
    cnt = np.diff(c['feat_ptr'])
    assert cnt.min() >= 1 and cnt.max() <= 7 and len(set(c['obs_img'])) == 5
    assert n_sky == int(c['sky'].sum()) > 0
    ld = np.longdouble
    uv1 = np.concatenate([c['obs_uv'], np.ones((len(c['obs_uv']), 1))], 1).astype(ld)
    v = np.einsum('oij,oj->oi', c['M'].reshape(-1, 3, 3).astype(ld)[c['obs_img']], uv1)
    v /= np.sqrt((v * v).sum(1))[:, None]
    assert np.array_equal(v[:, 2] <= 0, c['sky'])
    cam = c['ned'].astype(ld)[c['obs_img']]
    d = -(cam[:, 2] + c['base'].astype(ld)[c['obs_img']])
    p = cam + np.stack([v[:, 0] * d / v[:, 2], v[:, 1] * d / v[:, 2], d], 1)
    p[c['sky']] = 0
    only_sky = mixed = 0
    for f in range(n_feat):
        b, e = c['feat_ptr'][f], c['feat_ptr'][f + 1]
        want = p[b:e].sum(0) / ld(e - b)
        assert np.all(np.abs(out[f] - want) <= 1e-9 * np.maximum(1, np.abs(want)))
        if c['sky'][b:e].all():
            only_sky += 1
            assert np.array_equal(out[f], np.zeros(3))
        elif c['sky'][b:e].any():
            mixed += 1
    assert mixed >= 1 and (only_sky >= 1 or n_feat == 1)
