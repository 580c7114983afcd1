"""Host side of the match verification: the sampling rule of csrc/verify_rule.h against its Python
restatement, the argument checks of the C ABI, the list surgery of matcher.verify_matches through
its launch seam, and the honesty of the inputs tests/test_match_verify_gpu.py asserts on (the
reference's own consensus on them is unambiguous).  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import verify_reference as vr


def _lib():
    from imageanalysis_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------
# the sampling rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, (1 << 63) + 5])
def test_sample_equals_restatement(seed):
    L = _lib()
    hyps = np.arange(4096)
    out = (ctypes.c_int32 * 8)()
    for n in (4, 5, 8, 9, 63, 64, 65, 2000, 1 << 24):
        for k in (4, 8):
            if k > n:
                continue
            want = vr.samples(n, k, hyps, seed)
            assert want.min() >= 0 and want.max() < n
            assert (np.diff(np.sort(want, axis=1), axis=1) > 0).all(), "indices repeat"
            got = np.zeros((len(hyps), k), np.int64)
            for h in hyps.tolist():
                assert L.iamx_verify_sample(n, k, h, seed, out) == 0
                got[h] = out[:k]
            assert (got == want).all(), (n, k)
            for h in (0, 1, 4095):
                assert vr.sample(n, k, h, seed) == want[h].tolist()


def test_sample_is_spread():
    """n = 9, k = 8: every index is the omitted one about 4096 / 9 = 455 times"""
    s = vr.samples(9, 8, np.arange(4096), 0)
    omitted = 36 - s.sum(1)
    counts = np.bincount(omitted, minlength=9)
    assert counts.sum() == 4096 and counts.min() >= 300, counts


def test_argument_checks_without_a_gpu():
    L = _lib()
    buf = (ctypes.c_double * 32)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = lambda **kw: L.iamx_verify_pairs(*[kw.get(k, d) for k, d in (
        ('pts', p), ('m_off', p), ('n_pairs', 0), ('total', 0), ('model', 0), ('tol', p),
        ('hypotheses', 16), ('seed', 0), ('mask', p), ('out_model', p), ('out_best', p),
        ('status', p), ('stream', None))])
    assert ok() == 0                                     # no pairs: no launch, no device needed
    assert ok(model=1) == 0
    assert ok(model=2) == -1 and ok(model=-1) == -1
    assert ok(n_pairs=-1) == -1 and ok(total=-1) == -1 and ok(hypotheses=0) == -1
    for name in ('m_off', 'tol', 'out_model', 'out_best', 'status'):
        assert ok(**{name: None}) == -1, name
    assert ok(total=4, pts=None) == -1 and ok(total=4, mask=None) == -1
    assert ok(pts=ctypes.c_void_p(p.value + 4)) == -1    # not 16-byte aligned
    out = (ctypes.c_int32 * 8)()
    assert L.iamx_verify_sample(9, 8, 0, 0, out) == 0
    assert L.iamx_verify_sample(9, 8, 0, 0, None) == -1
    assert L.iamx_verify_sample(7, 8, 0, 0, out) == -1 and L.iamx_verify_sample(9, 9, 0, 0, out) == -1
    assert L.iamx_verify_sample(9, 0, 0, 0, out) == -1 and L.iamx_verify_sample(9, 4, -1, 0, out) == -1
    assert L.iamx_verify_sample(1 << 31, 4, 0, 0, out) == -1


# ---------------------------------------------------------------------------------------------
# the reference agrees with itself
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['H-n65', 'F-n65', 'F-duplicates', 'H-share0.6'])
def test_reference_paths_agree(name):
    """the vectorised float64 solve, the scalar walk in Python floats, longdouble and mpmath"""
    c = next(c for c in vr.cases() if c.name == name)
    r = vr.case_consensus(name)
    for h in (0, r['best'][0]):
        idx = r['idx'][h].tolist()
        scalar = vr.solve_scalar(c.points, c.model, idx, float, math.sqrt)
        exact = vr.solve_mp(c.points, c.model, idx)
        bound = max(16 * vr.model_distance(r['models64'][h], exact), 1e-12)
        assert vr.model_distance(scalar, exact) <= bound
        assert vr.model_distance(r['modelsld'][h], exact) <= 1e-15


# ---------------------------------------------------------------------------------------------
# honesty of the GPU cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [None, vr.OTHER_SEED])
def test_gpu_cases_are_unambiguous(seed):
    """On every asserted input the reference's own consensus is unambiguous: under its best model no
    error lies inside the guard band, the best hypothesis is not flagged, float64 and longdouble
    agree on its mask (but for the cases listed as UNSTABLE), and where a planted set is asserted
    the reference returns it."""
    for c in (vr.cases() if seed is None else vr.other_seed_cases()):
        r = vr.case_consensus(c.name, seed)
        if c.status is not None:
            assert r['status'] == c.status, c.name
        if r['status'] != vr.OK:
            continue
        h, count = r['best']
        err, t2 = r['err'][h], r['tol2']
        with np.errstate(invalid='ignore'):
            inside = (err > t2 * (1 - vr.BAND)) & (err <= t2 * (1 + vr.BAND))
            mask = err <= t2
        assert inside.sum() == 0, c.name
        assert not r['flagged'][h], c.name
        assert r['lower'][h] == r['upper'][h] == count == mask.sum(), c.name
        assert r['stable'] == (c.name not in vr.UNSTABLE), c.name
        if c.expect == 'exact':
            assert (mask == c.planted).all(), c.name
            assert c.planted.mean() >= 0.6 and len(c.points) >= 25
        elif c.expect == 'superset':
            assert mask[c.planted].all(), c.name


def test_standin_project_is_unambiguous():
    from imageanalysis_amd.matchpairs import MatchPairs
    _proj, truth = vr.standin_project(MatchPairs)
    for key, t in truth.items():
        r = vr.consensus(t['points'], vr.TOL, vr.HOMOGRAPHY, 256, 0)
        h = r['best'][0]
        err = r['err'][h]
        assert ((err <= r['tol2']) == t['planted']).all() and not r['flagged'][h] and r['stable']
        assert ((err > r['tol2'] * (1 - vr.BAND)) & (err <= r['tol2'] * (1 + vr.BAND))).sum() == 0


# ---------------------------------------------------------------------------------------------
# list surgery of verify_matches, through the launch seam
# ---------------------------------------------------------------------------------------------
def _project():
    from imageanalysis_amd.matchpairs import MatchPairs
    proj, truth = vr.standin_project(MatchPairs)
    return proj, truth, MatchPairs


def _planted_launch(truth, status=None, seen=None):
    def launch(jobs, transform, hypotheses, seed, arena):
        assert arena is None
        if seen is not None:
            seen.append([(ia, ib, len(pairs)) for ia, ib, pairs, _tol in jobs])
        for ia, ib, pairs, tol in jobs:
            assert (pairs == truth[(ia, ib)]['forward']).all() and tol == vr.TOL
        return ([truth[(ia, ib)]['planted'].astype(np.uint8) for ia, ib, _p, _t in jobs],
                [0 if status is None else status.get((ia, ib), 0) for ia, ib, _p, _t in jobs])
    return launch


def test_surgery_forward_reverse_and_counts():
    from imageanalysis_amd import matcher
    proj, truth, MatchPairs = _project()
    a, b, c = proj.image_list
    seen = []
    counts = matcher.verify_matches(proj, None, 'fundamental', launch=_planted_launch(truth, seen=seen))
    assert seen == [[(0, 1, 100), (0, 2, 110), (1, 2, 120)]]         # one batch, in image order
    keep = {k: t['forward'][t['planted']].tolist() for k, t in truth.items()}
    assert isinstance(a.match_list['b'], MatchPairs) and a.match_list['b'].tolist() == keep[(0, 1)]
    assert a.match_list['b']._a is not None, "the forward list left its array form"
    assert type(a.match_list['c']) is list and a.match_list['c'] == keep[(0, 2)]
    assert b.match_list['c'].tolist() == keep[(1, 2)]
    assert type(b.match_list['a']) is list
    assert b.match_list['a'] == truth[(0, 1)]['reverse_kept'].tolist()        # its own order kept
    assert 'a' not in c.match_list                                          # not created
    assert isinstance(c.match_list['b'], MatchPairs) and c.match_list['b']._a is not None
    assert c.match_list['b'].tolist() == truth[(1, 2)]['reverse_kept'].tolist()
    n_in = sum(len(t['forward']) for t in truth.values())
    n_out = sum(int(t['planted'].sum()) for t in truth.values())
    assert counts == dict(pairs=3, matches_in=n_in, matches_out=n_out, lists_emptied=0, too_few=0,
                          no_model=0, orphans_dropped=2)
    assert (a.matches_clean, b.matches_clean, c.matches_clean) == (False, False, False)


def test_surgery_batches_by_match_count(monkeypatch):
    from imageanalysis_amd import matcher
    proj, truth, _ = _project()
    monkeypatch.setattr(matcher, 'VERIFY_BATCH_MATCHES', 215)
    seen = []
    matcher.verify_matches(proj, None, 'homography', launch=_planted_launch(truth, seen=seen))
    assert seen == [[(0, 1, 100), (0, 2, 110)], [(1, 2, 120)]]
    monkeypatch.setattr(matcher, 'VERIFY_BATCH_MATCHES', 50)      # a pair larger than the bound goes alone
    proj, truth, _ = _project()
    seen = []
    matcher.verify_matches(proj, None, 'homography', launch=_planted_launch(truth, seen=seen))
    assert [len(s) for s in seen] == [1, 1, 1]


def test_surgery_clean_when_nothing_goes():
    from imageanalysis_amd import matcher
    proj, truth, _ = _project()
    a, b, c = proj.image_list
    del b.match_list['a']                                   # (its orphans would dirty b)
    for t in truth.values():
        t['planted'][:] = True
    before = {im.name: {k: [list(p) for p in v] for k, v in im.match_list.items()} for im in proj.image_list}
    counts = matcher.verify_matches(proj, None, 'homography', launch=_planted_launch(truth))
    assert counts['matches_in'] == counts['matches_out'] and counts['lists_emptied'] == 0
    assert (a.matches_clean, b.matches_clean, c.matches_clean) == (True, True, True)
    for im in proj.image_list:
        assert {k: [list(p) for p in v] for k, v in im.match_list.items()} == before[im.name]


def test_surgery_min_pairs_and_statuses():
    from imageanalysis_amd import matcher
    proj, truth, MatchPairs = _project()
    a, b, c = proj.image_list
    # (a, b): 24 matches, one short of min_pairs -> both directions emptied, never launched
    short = truth[(0, 1)]['forward'][:24]
    a.match_list['b'] = MatchPairs(short.copy())
    b.match_list['a'] = short[:, ::-1].tolist()
    # (a, c): NO_MODEL; (b, c): TOO_FEW, with a reverse list of 24 that is emptied for its length
    c.match_list['b'] = truth[(1, 2)]['reverse'][:24].tolist()
    seen = []
    counts = matcher.verify_matches(
        proj, None, 'homography',
        launch=_planted_launch(truth, status={(0, 2): vr.NO_MODEL, (1, 2): vr.TOO_FEW}, seen=seen))
    assert seen == [[(0, 2, 110), (1, 2, 120)]]
    assert a.match_list['b'] == [] and b.match_list['a'] == []
    assert a.match_list['c'] == []
    assert b.match_list['c'].tolist() == truth[(1, 2)]['forward'].tolist()      # TOO_FEW: unchanged
    assert c.match_list['b'] == []
    assert counts == dict(pairs=3, matches_in=24 + 110 + 120, matches_out=120, lists_emptied=4,
                          too_few=1, no_model=1, orphans_dropped=0)


def test_transform_values():
    from imageanalysis_amd import matcher
    proj, truth, _ = _project()
    a, b, _c = proj.image_list
    before = a.match_list['b'].tolist()
    zero = dict(pairs=0, matches_in=0, matches_out=0, lists_emptied=0, too_few=0, no_model=0,
                orphans_dropped=0)
    assert matcher.verify_matches(proj, None, 'none') == zero
    assert matcher.filter_by_transform(None, a, b, 'none') is True
    assert a.match_list['b'].tolist() == before and a.matches_clean
    for fn in (lambda t: matcher.verify_matches(proj, None, t),
               lambda t: matcher.filter_by_transform(None, a, b, t)):
        with pytest.raises(NotImplementedError, match='five-point'):
            fn('essential')
        with pytest.raises(ValueError):
            fn('affine')
    a.match_list['b'] = before[:24]
    assert matcher.filter_by_transform(None, a, b, 'homography') is True     # short: emptied, no launch
    assert a.match_list['b'] == []
