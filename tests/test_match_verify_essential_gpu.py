"""iamx_five_point and iamx_verify_pairs_essential (csrc/five_point.h, match_verify.hip) on the device
against tests/essential_reference.py: the solver alone on 144 samples, then per pair the edges of
n, the reported model / mask / choice, planted inlier sets, degenerate inputs, batching, and
matcher.verify_matches on a stand-in project over relief.  Every launch goes through the C ABI with
poison-filled outputs and guard bytes behind them."""
import ctypes

import numpy as np
import pytest

import essential_reference as er
import verify_reference as vr

pytestmark = pytest.mark.gpu
GUARD = 64
POISON_U8, POISON_F, POISON_I = 0xAB, 777.0, -999


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _launch(case_list, hypotheses, seed, K=er.KMAT):
    """one launch over case_list (None = a pair without matches); per pair (mask, model, best,
    status, essential) as numpy"""
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
    d_tol = torch.full((len(lens),), er.TOL, dtype=torch.float64, device=dev)
    d_mask = torch.full((total + GUARD,), POISON_U8, dtype=torch.uint8, device=dev)
    d_model = torch.full((len(lens) + 1, 9), POISON_F, dtype=torch.float64, device=dev)
    d_ess = torch.full((len(lens) + 1, 9), POISON_F, dtype=torch.float64, device=dev)
    d_best = torch.full((len(lens) + 1, 2), POISON_I, dtype=torch.int32, device=dev)
    d_status = torch.full((len(lens) + 1,), POISON_I, dtype=torch.int32, device=dev)
    Kh = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    rc = _lib.lib().iamx_verify_pairs_essential(
        _P(d_pts), _P(d_off), len(lens), total, Kh.ctypes.data_as(ctypes.c_void_p), _P(d_tol), hypotheses,
        seed, _P(d_mask), _P(d_model), _P(d_ess), _P(d_best), _P(d_status),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().iamx_last_error()
    torch.cuda.synchronize()
    mask, model, ess, best, status = (t.cpu().numpy() for t in (d_mask, d_model, d_ess, d_best, d_status))
    assert (mask[total:] == POISON_U8).all(), "guard bytes behind the mask were written"
    assert (model[-1] == POISON_F).all() and (ess[-1] == POISON_F).all(), "guard row behind the models"
    assert (best[-1] == POISON_I).all() and status[-1] == POISON_I, "guard row behind best / status"
    return [(mask[m_off[k]:m_off[k + 1]].copy(), model[k].copy(), best[k].copy(), int(status[k]), ess[k].copy())
            for k in range(len(lens))]


@pytest.fixture(scope='module')
def singles():
    return {c.name: _launch([c], c.hypotheses, c.seed)[0] for c in er.cases()}


# ---------------------------------------------------------------------------------------------
# the solver alone
# ---------------------------------------------------------------------------------------------
def test_five_point_solver():
    """144 samples: every emitted E satisfies its equations within 16 x what solve64 leaves on the
    same solution; every exact real solution solve64 finds is emitted within max(16 d64, FLOOR_E)"""
    import torch
    from imageanalysis_amd import _lib
    r, E64, c64 = er.solver_samples()
    n = len(r)
    dev = torch.device('cuda', 0)
    d_r = torch.from_numpy(r).to(dev)
    d_E = torch.full((n * 90 + GUARD,), POISON_F, dtype=torch.float64, device=dev)
    d_c = torch.full((n + GUARD,), POISON_I, dtype=torch.int32, device=dev)
    rc = _lib.lib().iamx_five_point(_P(d_r), n, _P(d_E), _P(d_c),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().iamx_last_error()
    torch.cuda.synchronize()
    E, cnt = d_E.cpu().numpy(), d_c.cpu().numpy()
    assert (E[n * 90:] == POISON_F).all() and (cnt[n:] == POISON_I).all(), "guard elements were written"
    E, cnt = E[:n * 90].reshape(n, 10, 9), cnt[:n]
    assert ((cnt >= 0) & (cnt <= 10)).all()
    total = missed = 0
    worst = [0.0, 0.0]
    for k in range(n):
        assert np.isnan(E[k][cnt[k]:]).all() and np.isfinite(E[k][:cnt[k]]).all()
        for j in range(cnt[k]):
            e = E[k][j]
            assert abs(np.sqrt((e.astype(np.longdouble) ** 2).sum()) - 1) < 1e-14
            assert e[np.argmax(np.abs(e))] > 0
            d, m = er.nearest(e, E64[k][:c64[k]])
            assert m >= 0, "a model solve64 does not have"
            got, ref = er.residuals(e, r[k]), er.residuals(E64[k][m], r[k])
            for g, w in zip(got, ref):
                worst[0] = max(worst[0], g / w if w > 0 else (0.0 if g == 0 else np.inf))
                assert g <= 16 * w, (k, j, got, ref)
        for ex in er.solver_exact(k):
            d64 = er.nearest(ex, E64[k][:c64[k]])[0]
            total += 1
            if not d64 <= er.MISS:
                missed += 1
                continue
            d = er.nearest(ex, E[k][:cnt[k]])[0]
            worst[1] = max(worst[1], d / max(16 * d64, er.FLOOR_E))
            assert d <= max(16 * d64, er.FLOOR_E), (k, d, d64)
    print('largest residual ratio device / solve64 %.3g (bound 16); largest distance / bound %.3g; '
          'exact solutions %d, solve64 missed %d' % (worst[0], worst[1], total, missed))
    assert missed * 50 <= total


# ---------------------------------------------------------------------------------------------
# pairs
# ---------------------------------------------------------------------------------------------
def _ref(c, seed=None):
    r = dict(er.case_consensus(c.name, seed))
    r['seed'] = c.seed if seed is None else seed
    return r


def _check_abc(c, result, ref):
    """(a) model, (b) mask and count, (c) choice of one pair with status OK"""
    mask, model, best, status, ess = result
    assert status == er.OK
    assert np.isfinite(model).all() and np.isfinite(ess).all()
    assert 0 <= best[0] < c.hypotheses
    for m in (model, ess):
        assert abs(np.sqrt((m.astype(np.longdouble) ** 2).sum()) - 1) < 1e-14
        assert m[np.argmax(np.abs(m))] > 0
    assert set(np.unique(mask)) <= {0, 1}
    assert int(best[1]) == int(mask.sum())
    if c.name in er.UNSTABLE:
        # the yardstick is the float64 expression under the reported model: an exact one, no band
        err = er.errors(model, c.points)[0]
        with np.errstate(invalid='ignore'):
            assert (mask.astype(bool) == (err <= ref['tol2'])).all()
        return
    # (a) the reported hypothesis' sample, solved exactly
    idx = vr.sample(len(c.points), er.SAMPLE, int(best[0]), ref['seed'])
    assert idx == ref['idx'][best[0]].tolist()
    exE, exF = er.solve_mp(c.points, c.K, idx)
    got, k = er.nearest(model, exF)
    assert k >= 0
    mine = np.nonzero(ref['hyp'] == best[0])[0]                 # the reference's candidates of that sample
    d64 = min(vr.model_distance(ref['F64'][m], exF[k]) for m in mine)
    tol_a = max(16 * d64, er.FLOOR_E)
    gotE = vr.model_distance(ess, exE[k])
    d64E = min(vr.model_distance(ref['E64'][m], exE[k]) for m in mine)
    print('%s: |F - exact| = %.2e, bound %.2e; |E - exact| = %.2e, bound %.2e'
          % (c.name, got, tol_a, gotE, max(16 * d64E, er.FLOOR_E)))
    assert got <= tol_a
    assert gotE <= max(16 * d64E, er.FLOOR_E)
    # (b) the mask is the reported model's, outside the guard band
    err = er.errors(model, c.points, np.longdouble)[0]
    t2 = np.longdouble(c.tol) * np.longdouble(c.tol)
    with np.errstate(invalid='ignore'):
        inside = (err > t2 * (1 - er.BAND)) & (err <= t2 * (1 + er.BAND))
        want = err <= t2
    assert (mask.astype(bool) == want)[~inside].all()
    # (c) nothing the reference trusts beats it, nothing earlier ties it
    ok = ~ref['flagged']
    assert (ref['lower'][ok] <= best[1]).all()
    me = mine[int(np.argmin([vr.model_distance(ref['F64'][m], model) for m in mine]))]
    assert (ref['lower'][:me][ok[:me]] < best[1]).all()


@pytest.mark.parametrize('case', er.cases(), ids=repr)
def test_pair(case, singles):
    """statuses at the edges of n and on degenerate inputs; (a)-(c) for every pair with a model;
    the planted sets"""
    mask, model, best, status, ess = singles[case.name]
    ref = _ref(case)
    assert status == ref['status']
    if case.status is not None:
        assert status == case.status
    if status == er.TOO_FEW:
        assert (mask == 1).all() and np.isnan(model).all() and np.isnan(ess).all()
        assert best.tolist() == [-1, -1]
        return
    if status == er.NO_MODEL:
        assert (mask == 0).all() and np.isnan(model).all() and np.isnan(ess).all()
        assert best.tolist() == [-1, 0]
        return
    _check_abc(case, singles[case.name], ref)
    if case.expect == 'exact':
        assert (mask.astype(bool) == case.planted).all()
    elif case.expect == 'superset':
        assert mask.astype(bool)[case.planted].all()
        assert 1 <= int(mask.sum() - case.planted.sum()) <= 28


def test_essential_output_is_optional(singles):
    """a NULL out_essential changes nothing else (kernels.verify_pairs without return_essential)"""
    from imageanalysis_amd import kernels
    c = next(c for c in er.cases() if c.name == 'E-n65')
    four = kernels.verify_pairs(c.points, np.array([0, 65], np.int64), 'essential', er.TOL, 256, 0, K=er.KMAT)
    five = kernels.verify_pairs(c.points, np.array([0, 65], np.int64), 'essential', er.TOL, 256, 0, K=er.KMAT,
                                return_essential=True)
    assert len(four) == 4 and len(five) == 5
    mask, model, best, status, ess = singles[c.name]
    for got in (four, five):
        assert got[0].cpu().numpy().tobytes() == mask.tobytes()
        assert got[1].cpu().numpy().tobytes() == model.tobytes() and tuple(got[1].shape) == (1, 3, 3)
        assert got[2].cpu().numpy().tobytes() == best.tobytes() and int(got[3].cpu()[0]) == status
    assert five[4].cpu().numpy().tobytes() == ess.tobytes()
    with pytest.raises(ValueError):
        kernels.verify_pairs(c.points, np.array([0, 65], np.int64), 'essential', er.TOL)
    with pytest.raises(ValueError):
        kernels.verify_pairs(c.points, np.array([0, 65], np.int64), 'fundamental', er.TOL, K=er.KMAT)


def test_five_point_binding():
    from imageanalysis_amd import kernels
    r, E64, c64 = er.solver_samples()
    E, count = kernels.five_point(r[:7])
    assert tuple(E.shape) == (7, 10, 3, 3) and count.cpu().numpy().tolist() == c64[:7].tolist()
    E0, count0 = kernels.five_point(np.zeros((0, 5, 4)))
    assert tuple(E0.shape) == (0, 10, 3, 3) and count0.numel() == 0
    with pytest.raises(ValueError):
        kernels.five_point(np.zeros((3, 4, 4)))


def test_batch_equals_singles(singles):
    """all cases in one launch, shuffled, with empty pairs between them: bit for bit the single
    launches; a second run repeats the first"""
    group = [c for c in er.cases() if c.hypotheses == 256 and c.seed == 0]
    order = np.random.default_rng(13).permutation(len(group))
    batch = []
    for k in order:
        batch += [group[k], None]
    first = _launch(batch, 256, 0)
    second = _launch(batch, 256, 0)
    for c, a, b in zip(batch, first, second):
        if c is None:
            assert a[3] == er.TOO_FEW and len(a[0]) == 0
            continue
        for x, y, z in zip(singles[c.name], a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes() == np.asarray(z).tobytes(), c.name


def test_other_seed(singles):
    group = er.other_seed_cases()
    seed = er.OTHER_SEED
    out = _launch(group, 256, seed)
    moved = 0
    for c, res in zip(group, out):
        ref = _ref(c, seed)
        assert res[3] == ref['status']
        if res[3] == er.OK:
            _check_abc(c, res, ref)
            moved += int(res[2][0] != singles[c.name][2][0])
    assert moved >= 1


def test_skewed_camera():
    """a camera with skew and unequal focal lengths: the reported model is an exact solution of the
    reported sample under that camera"""
    K = np.array([[3600.0, 2.5, 2700.0], [0.0, 3700.0, 1800.0], [0.0, 0.0, 1.0]])
    c = next(c for c in er.cases() if c.name == 'E-n65')
    mask, model, best, status, ess = _launch([c], 64, 0, K=K)[0]
    assert status == er.OK
    idx = vr.sample(65, er.SAMPLE, int(best[0]), 0)
    exE, exF = er.solve_mp(c.points, K, idx)
    E64, F64, valid = er.solve64(c.points, K, np.array([idx]))
    got, k = er.nearest(model, exF)
    d64 = min(vr.model_distance(F64[0][j], exF[k]) for j in np.nonzero(valid[0])[0])
    assert got <= max(16 * d64, er.FLOOR_E)
    assert vr.model_distance(ess, exE[k]) <= max(16 * min(vr.model_distance(E64[0][j], exE[k])
                                                          for j in np.nonzero(valid[0])[0]), er.FLOOR_E)
    assert int(best[1]) == int(mask.sum())


# ---------------------------------------------------------------------------------------------
# the matcher
# ---------------------------------------------------------------------------------------------
def test_verify_matches_project():
    from imageanalysis_amd import matcher
    from imageanalysis_amd.matchpairs import MatchPairs
    proj, truth = er.standin_project(MatchPairs)
    a, b, c = proj.image_list
    counts = matcher.verify_matches(proj, er.KMAT, 'essential', hypotheses=256, seed=0)
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
    proj, truth = er.standin_project(MatchPairs)
    a, b, _c = proj.image_list
    rev_before = list(b.match_list['a'])
    clean = matcher.filter_by_transform(er.KMAT, a, b, 'essential', hypotheses=256)
    t = truth[(0, 1)]
    assert clean is False and a.match_list['b'].tolist() == t['forward'][t['planted']].tolist()
    assert b.match_list['a'] == rev_before and not a.matches_clean and b.matches_clean
