"""iamx_verify_pairs (csrc/match_verify.hip) on the device against tests/verify_reference.py: the
edges of n, the reported model / mask / choice of every pair, planted inlier sets, degenerate
inputs, batching, and matcher.verify_matches on a stand-in project.  Every launch goes through the
C ABI with poison-filled outputs and guard bytes behind the mask."""
import ctypes

import numpy as np
import pytest

import verify_reference as vr

pytestmark = pytest.mark.gpu
GUARD = 64
POISON_U8, POISON_F, POISON_I = 0xAB, 777.0, -999


def _launch(case_list, model, hypotheses, seed):
    """one launch over case_list (None = a pair without matches); per pair (mask, model, best,
    status) as numpy, plus whether the guard bytes survived"""
    import torch
    from imageanalysis_amd import _lib
    lens = [0 if c is None else len(c.points) for c in case_list]
    m_off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=m_off[1:])
    total = int(m_off[-1])
    pts = np.concatenate([c.points for c in case_list if c is not None] + [np.zeros((0, 4), np.float32)])
    dev = torch.device('cuda', 0)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    d_off = torch.from_numpy(m_off).to(dev)
    d_tol = torch.full((len(lens),), vr.TOL, dtype=torch.float64, device=dev)
    d_mask = torch.full((total + GUARD,), POISON_U8, dtype=torch.uint8, device=dev)
    d_model = torch.full((len(lens), 9), POISON_F, dtype=torch.float64, device=dev)
    d_best = torch.full((len(lens), 2), POISON_I, dtype=torch.int32, device=dev)
    d_status = torch.full((len(lens),), POISON_I, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().iamx_verify_pairs(P(d_pts), P(d_off), len(lens), total, model, P(d_tol), hypotheses,
                                      seed, P(d_mask), P(d_model), P(d_best), P(d_status),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().iamx_last_error()
    torch.cuda.synchronize()
    mask, model_, best, status = (t.cpu().numpy() for t in (d_mask, d_model, d_best, d_status))
    assert (mask[total:] == POISON_U8).all(), "guard bytes behind the mask were written"
    return [(mask[m_off[k]:m_off[k + 1]].copy(), model_[k].copy(), best[k].copy(), int(status[k]))
            for k in range(len(lens))]


@pytest.fixture(scope='module')
def singles():
    return {c.name: _launch([c], c.model, c.hypotheses, c.seed)[0] for c in vr.cases()}


def _check_abc(c, result, ref):
    """(a) model, (b) mask and count, (c) choice of one pair with status OK"""
    mask, model, best, status = result
    assert status == vr.OK
    assert np.isfinite(model).all()
    assert 0 <= best[0] < c.hypotheses
    assert abs(np.sqrt((model.astype(np.longdouble) ** 2).sum()) - 1) < 1e-14
    assert model[np.argmax(np.abs(model))] > 0
    # (a) the reported hypothesis' sample, solved by the reference
    idx = vr.sample(len(c.points), vr.SAMPLE[c.model], int(best[0]), ref['seed'])
    assert idx == ref['idx'][best[0]].tolist()
    exact = vr.solve_mp(c.points, c.model, idx)
    f64 = ref['models64'][best[0]]
    tol_a = max(16 * vr.model_distance(f64, exact), vr.FLOOR)
    got = vr.model_distance(model, exact)
    print('%s: |device - exact| = %.2e, bound %.2e' % (c.name, got, tol_a))
    assert got <= tol_a
    # (b) the mask is the reported model's, outside the guard band.  Where the reference finds its
    # own best model's errors ill conditioned (UNSTABLE: float64 and longdouble disagree on them),
    # the yardstick is the float64 evaluation, which is then an exact one: no band.
    assert ref['stable'] == (c.name not in vr.UNSTABLE)
    dtype = np.longdouble if ref['stable'] else np.float64
    err = vr.errors(model, c.points, c.model, dtype)[0]
    t2 = dtype(c.tol) * dtype(c.tol)
    with np.errstate(invalid='ignore'):
        inside = (err > t2 * (1 - vr.BAND)) & (err <= t2 * (1 + vr.BAND)) & ref['stable']
        want = err <= t2
    assert set(np.unique(mask)) <= {0, 1}
    assert (mask.astype(bool) == want)[~inside].all()
    assert int(best[1]) == int(mask.sum())
    # (c) nothing the reference trusts beats it, nothing earlier ties it
    ok = ~ref['flagged']
    assert (ref['lower'][ok] <= best[1]).all()
    assert (ref['lower'][:best[0]][ok[:best[0]]] < best[1]).all()


def _ref(c, seed=None):
    r = dict(vr.case_consensus(c.name, seed))
    r['seed'] = c.seed if seed is None else seed
    return r


@pytest.mark.parametrize('case', vr.cases(), ids=repr)
def test_pair(case, singles):
    """statuses at the edges of n and on degenerate inputs; (a)-(c) for every pair with a model;
    the planted sets"""
    mask, model, best, status = singles[case.name]
    ref = _ref(case)
    assert status == ref['status']
    if case.status is not None:
        assert status == case.status
    if status == vr.TOO_FEW:
        assert (mask == 1).all() and np.isnan(model).all() and best.tolist() == [-1, -1]
        return
    if status == vr.NO_MODEL:
        assert (mask == 0).all() and np.isnan(model).all() and best.tolist() == [-1, 0]
        return
    _check_abc(case, singles[case.name], ref)
    if case.expect == 'exact':
        assert (mask.astype(bool) == case.planted).all()
    elif case.expect == 'superset':
        assert mask.astype(bool)[case.planted].all()


def _batchable(model):
    return [c for c in vr.cases() if c.model == model and c.hypotheses == 256 and c.seed == 0]


@pytest.mark.parametrize('model', [vr.HOMOGRAPHY, vr.FUNDAMENTAL])
def test_batch_equals_singles(model, singles):
    """all cases of a model in one launch, shuffled, with empty pairs between them: bit for bit the
    single launches; a second run repeats the first"""
    group = _batchable(model)
    order = np.random.default_rng(11 + model).permutation(len(group))
    batch = []
    for k in order:
        batch += [group[k], None]
    first = _launch(batch, model, 256, 0)
    second = _launch(batch, model, 256, 0)
    for c, a, b in zip(batch, first, second):
        if c is None:
            assert a[3] == vr.TOO_FEW and len(a[0]) == 0
            continue
        for x, y, z in zip(singles[c.name], a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes() == np.asarray(z).tobytes(), c.name


@pytest.mark.parametrize('model', [vr.HOMOGRAPHY, vr.FUNDAMENTAL])
def test_other_seed(model, singles):
    group = vr.other_seed_cases(model)
    seed = vr.OTHER_SEED
    out = _launch(group, model, 256, seed)
    moved = 0
    for c, res in zip(group, out):
        ref = _ref(c, seed)
        assert res[3] == ref['status']
        if res[3] == vr.OK:
            _check_abc(c, res, ref)
            moved += int(res[2][0] != singles[c.name][2][0])
    assert moved >= 1


def test_verify_matches_project():
    from imageanalysis_amd import matcher
    from imageanalysis_amd.matchpairs import MatchPairs
    proj, truth = vr.standin_project(MatchPairs)
    a, b, c = proj.image_list
    counts = matcher.verify_matches(proj, None, 'homography', hypotheses=256, seed=0)
    keep = {k: t['forward'][t['planted']].tolist() for k, t in truth.items()}
    assert isinstance(a.match_list['b'], MatchPairs) and a.match_list['b'].tolist() == keep[(0, 1)]
    assert isinstance(a.match_list['c'], list) and a.match_list['c'] == keep[(0, 2)]
    assert isinstance(b.match_list['c'], MatchPairs) and b.match_list['c'].tolist() == keep[(1, 2)]
    assert b.match_list['a'] == truth[(0, 1)]['reverse_kept'].tolist()
    assert 'a' not in c.match_list
    assert isinstance(c.match_list['b'], MatchPairs)
    assert c.match_list['b'].tolist() == truth[(1, 2)]['reverse_kept'].tolist()
    n_in = sum(len(t['forward']) for t in truth.values())
    n_out = sum(int(t['planted'].sum()) for t in truth.values())
    assert counts == dict(pairs=3, matches_in=n_in, matches_out=n_out, lists_emptied=0, too_few=0,
                          no_model=0, orphans_dropped=2)
    assert not a.matches_clean and not b.matches_clean and not c.matches_clean


def test_filter_by_transform_one_direction():
    from imageanalysis_amd import matcher
    from imageanalysis_amd.matchpairs import MatchPairs
    proj, truth = vr.standin_project(MatchPairs)
    a, b, _c = proj.image_list
    rev_before = list(b.match_list['a'])
    clean = matcher.filter_by_transform(None, a, b, 'homography', hypotheses=256)
    t = truth[(0, 1)]
    assert clean is False and a.match_list['b'].tolist() == t['forward'][t['planted']].tolist()
    assert b.match_list['a'] == rev_before and not a.matches_clean and b.matches_clean
