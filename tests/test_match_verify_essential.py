"""Host side of the essential model of the match verification: the argument checks of
iamx_verify_pairs_essential and iamx_five_point, the float64 restatement of the five-point solver
against a 60-digit solve, the honesty of the inputs tests/test_match_verify_essential_gpu.py asserts
on, and the matcher's list surgery for 'essential' through its launch seam.  No GPU."""
import ctypes

import numpy as np
import pytest

import essential_reference as er
import verify_reference as vr


def _lib():
    from imageanalysis_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    L = _lib()
    buf = (ctypes.c_double * 32)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def ok(K=(3666.0, 0.0, 2736.0, 0.0, 3666.0, 1824.0, 0.0, 0.0, 1.0), **kw):
        Kh = None if K is None else (ctypes.c_double * 9)(*K)
        return L.iamx_verify_pairs_essential(*[kw.get(k, d) for k, d in (
            ('pts', p), ('m_off', p), ('n_pairs', 0), ('total', 0), ('K', Kh), ('tol', p),
            ('hypotheses', 16), ('seed', 0), ('mask', p), ('out_model', p), ('out_essential', p),
            ('out_best', p), ('status', p), ('stream', None))])
    assert ok() == 0                                     # no pairs: no launch, no device needed
    assert ok(out_essential=None) == 0                   # E is optional
    assert ok(K=(3666.0, 1.5, 2736.0, 0.0, -3600.0, 1824.0, 0.0, 0.0, 1.0)) == 0     # a skew is allowed
    assert ok(K=None) == -1
    good = [3666.0, 0.0, 2736.0, 0.0, 3666.0, 1824.0, 0.0, 0.0, 1.0]
    for at, value in ((3, 1e-9), (6, 1.0), (7, -1.0), (8, 2.0), (8, 0.0), (0, 0.0), (4, 0.0),
                      (0, float('inf')), (4, float('nan')), (0, float('nan'))):
        bad = list(good)
        bad[at] = value
        assert ok(K=bad) == -1, (at, value)
    assert ok(n_pairs=-1) == -1 and ok(total=-1) == -1 and ok(hypotheses=0) == -1
    for name in ('m_off', 'tol', 'out_model', 'out_best', 'status'):
        assert ok(**{name: None}) == -1, name
    assert ok(total=4, pts=None) == -1 and ok(total=4, mask=None) == -1
    assert ok(pts=ctypes.c_void_p(p.value + 4)) == -1    # not 16-byte aligned
    # the old entry keeps refusing the model by number
    assert L.iamx_verify_pairs(p, p, 0, 0, er.ESSENTIAL, p, 16, 0, p, p, p, p, None) == -1
    # the solver alone
    assert L.iamx_five_point(p, 0, p, p, None) == 0
    assert L.iamx_five_point(p, -1, p, p, None) == -1
    assert L.iamx_five_point(None, 0, p, p, None) == -1 and L.iamx_five_point(p, 0, None, p, None) == -1
    assert L.iamx_five_point(p, 0, p, None, None) == -1
    out = (ctypes.c_int32 * 8)()
    assert L.iamx_verify_sample(5, 5, 0, 0, out) == 0 and sorted(out[:5]) == [0, 1, 2, 3, 4]


def test_sample_rule_at_five():
    L = _lib()
    out = (ctypes.c_int32 * 8)()
    for n in (5, 6, 65, 2000):
        want = vr.samples(n, 5, np.arange(256), 3)
        assert (np.diff(np.sort(want, axis=1), axis=1) > 0).all()
        for h in range(256):
            assert L.iamx_verify_sample(n, 5, h, 3, out) == 0
            assert out[:5] == want[h].tolist()


# ---------------------------------------------------------------------------------------------
# the restatement against the exact solve
# ---------------------------------------------------------------------------------------------
def test_solve64_finds_the_exact_solutions():
    """over the 144 solver samples: every model solve64 emits satisfies the solver's equations, and
    at most 1 in 50 exact real solutions has no float64 candidate within MISS"""
    r, E, count = er.solver_samples()
    total = missed = 0
    dist = []
    for k in range(len(r)):
        exact = er.solver_exact(k)
        assert len(exact) % 2 == 0 and len(exact) <= 10        # real roots of a degree-10 polynomial
        for e in exact:
            epi, det, tr = er.residuals(e, r[k])
            assert max(epi, det, tr) < 1e-17    # a solution: 64 longdouble eps (it is rounded to longdouble)
            d = er.nearest(e, E[k][:count[k]])[0]
            total += 1
            missed += int(not d <= er.MISS)
            dist.append(d)
        for j in range(count[k]):
            assert abs(np.sqrt((E[k][j].astype(np.longdouble) ** 2).sum()) - 1) < 1e-14
            assert E[k][j][np.argmax(np.abs(E[k][j]))] > 0
        assert np.isnan(E[k][count[k]:]).all()
    print('exact solutions %d, missed %d, median distance %.2e, largest %.2e'
          % (total, missed, np.median(dist), np.max(dist)))
    assert total >= 500 and missed * 50 <= total
    assert abs(16 * np.median(dist) / er.FLOOR_E - 1) < 0.01    # the constant is what measure() gives, to 3 digits


def test_solve64_pixel_model_is_the_exact_one():
    """F = K^-T E K^-1 of the restatement against the 60-digit solve, with a skewed camera too"""
    c = next(c for c in er.cases() if c.name == 'E-n65')
    for K in (er.KMAT, np.array([[3600.0, 2.5, 2700.0], [0.0, 3700.0, 1800.0], [0.0, 0.0, 1.0]])):
        idx = vr.samples(65, 5, np.arange(4), 0)
        E, F, valid = er.solve64(c.points, K, idx)
        for h in range(4):
            eE, eF = er.solve_mp(c.points, K, idx[h])
            assert valid[h].sum() == len(eE) >= 2
            for j in np.nonzero(valid[h])[0]:
                dE, k = er.nearest(E[h][j], eE)
                assert dE <= 1e-9 and vr.model_distance(F[h][j], eF[k]) <= 1e-9 + 16 * dE


# ---------------------------------------------------------------------------------------------
# honesty of the GPU cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [None, er.OTHER_SEED])
def test_gpu_cases_are_unambiguous(seed):
    """On every asserted input the reference's own consensus is unambiguous: under its best candidate
    no error lies inside the guard band, the best candidate is not flagged (but for UNSTABLE), and
    where a planted set is asserted the reference returns it."""
    roots = {}
    for c in (er.cases() if seed is None else er.other_seed_cases()):
        r = er.case_consensus(c.name, seed)
        if c.status is not None:
            assert r['status'] == c.status, c.name
        if r['status'] != er.OK:
            continue
        k, _h, _root, count = r['best']
        roots[c.name] = int(np.bincount(r['hyp']).max())
        err, t2 = r['err'][k], r['tol2']
        with np.errstate(invalid='ignore'):
            inside = (err > t2 * (1 - er.BAND)) & (err <= t2 * (1 + er.BAND))
            mask = err <= t2
        assert inside.sum() == 0, c.name
        assert bool(r['flagged'][k]) == (c.name in er.UNSTABLE), c.name
        assert r['lower'][k] == r['upper'][k] == count == mask.sum(), c.name
        if c.expect == 'exact':
            assert (mask == c.planted).all(), c.name
            assert c.planted.mean() >= 0.6 and len(c.points) >= 25
        elif c.expect == 'superset':
            extra = int(mask.sum() - c.planted.sum())
            assert mask[c.planted].all() and 1 <= extra <= 28, c.name
    if seed is None:
        # the candidate list's capacity is exercised: a sample with ten real solutions
        assert roots['E-n64'] == 10 and roots['E-n256'] == 10
        assert er.case_consensus('E-identical')['status'] == er.NO_MODEL
        assert er.case_consensus('E-n4')['status'] == er.TOO_FEW


def test_standin_project_is_unambiguous():
    from imageanalysis_amd.matchpairs import MatchPairs
    _proj, truth = er.standin_project(MatchPairs)
    for _key, t in truth.items():
        r = er.consensus(t['points'], er.KMAT, er.TOL, 256, 0)
        k = r['best'][0]
        err = r['err'][k]
        assert ((err <= r['tol2']) == t['planted']).all() and not r['flagged'][k]
        assert ((err > r['tol2'] * (1 - er.BAND)) & (err <= r['tol2'] * (1 + er.BAND))).sum() == 0


# ---------------------------------------------------------------------------------------------
# the matcher
# ---------------------------------------------------------------------------------------------
def test_surgery_essential_through_the_seam():
    from imageanalysis_amd import matcher
    from imageanalysis_amd.matchpairs import MatchPairs
    proj, truth = er.standin_project(MatchPairs)
    a, b, c = proj.image_list
    seen = []

    def launch(jobs, transform, hypotheses, seed, arena):
        assert transform == 'essential' and hypotheses == 256 and seed == 9
        assert arena[0] is None and arena[1] is None and (arena[2] == er.KMAT).all()
        seen.append([(ia, ib, len(pairs)) for ia, ib, pairs, _tol in jobs])
        for ia, ib, pairs, tol in jobs:
            assert (pairs == truth[(ia, ib)]['forward']).all() and tol == er.TOL
        return ([truth[(ia, ib)]['planted'].astype(np.uint8) for ia, ib, _p, _t in jobs], [0] * len(jobs))
    counts = matcher.verify_matches(proj, er.KMAT, 'essential', seed=9, launch=launch)
    assert seen == [[(0, 1, 100), (0, 2, 110), (1, 2, 120)]]
    keep = {k: t['forward'][t['planted']].tolist() for k, t in truth.items()}
    assert isinstance(a.match_list['b'], MatchPairs) and a.match_list['b'].tolist() == keep[(0, 1)]
    assert type(a.match_list['c']) is list and a.match_list['c'] == keep[(0, 2)]
    assert b.match_list['c'].tolist() == keep[(1, 2)]
    assert b.match_list['a'] == truth[(0, 1)]['reverse_kept'].tolist()
    assert 'a' not in c.match_list
    assert c.match_list['b'].tolist() == truth[(1, 2)]['reverse_kept'].tolist()
    n_in = sum(len(t['forward']) for t in truth.values())
    n_out = sum(int(t['planted'].sum()) for t in truth.values())
    assert counts == dict(pairs=3, matches_in=n_in, matches_out=n_out, lists_emptied=0, too_few=0,
                          no_model=0, orphans_dropped=2)
    assert (a.matches_clean, b.matches_clean, c.matches_clean) == (False, False, False)


def test_hypotheses_defaults_by_model():
    from imageanalysis_amd import matcher
    from imageanalysis_amd.matchpairs import MatchPairs
    for transform, K, want in (('homography', None, 2048), ('fundamental', None, 2048),
                               ('essential', er.KMAT, 256)):
        proj, truth = er.standin_project(MatchPairs)
        got = []

        def launch(jobs, transform_, hypotheses, seed, arena):
            got.append(hypotheses)
            return [np.ones(len(j[2]), np.uint8) for j in jobs], [0] * len(jobs)
        matcher.verify_matches(proj, K, transform, launch=launch)
        assert got == [want], transform


def test_essential_without_a_camera_matrix():
    from imageanalysis_amd import matcher
    from imageanalysis_amd.matchpairs import MatchPairs
    proj, _truth = er.standin_project(MatchPairs)
    a, b, _c = proj.image_list
    before = a.match_list['b'].tolist()
    with pytest.raises(NotImplementedError, match='five-point'):
        matcher.verify_matches(proj, None, 'essential')
    with pytest.raises(NotImplementedError, match='no camera matrix'):
        matcher.filter_by_transform(None, a, b, 'essential')
    assert a.match_list['b'].tolist() == before and a.matches_clean
    # a short list is emptied before any launch, with a K as without
    a.match_list['b'] = before[:24]
    assert matcher.filter_by_transform(er.KMAT, a, b, 'essential') is True
    assert a.match_list['b'] == []
