"""Host: the high-precision BA reference of tests/ba_reference.py pinned against the goldens,
against mpmath and against SciPy, and the conditions on the synthetic edge-case problems
(tests/ba_edge_cases.py) that the solver-level comparisons of test_ba_edges_gpu.py rely on."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN

import ba_edge_cases as ec
import ba_reference as ref

BA_CASES = sorted(glob.glob(os.path.join(GOLDEN, 'ba_*.npz')))


def _golden(path):
    g = np.load(path)
    C, P = int(g['n_cameras']), int(g['n_points'])
    K = g['K']
    calib = None if bool(g['cam_calib']) else np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], *g['dist']])
    return g, C, P, calib


def test_body2cam_is_the_oracles():
    from oracle import ba_oracle
    assert np.array_equal(ref.BODY2CAM, ba_oracle.BODY2CAM) and ref._EPS == ba_oracle._EPS


@pytest.mark.parametrize('path', BA_CASES, ids=os.path.basename)
def test_residual_equals_goldens(path):
    g, C, P, calib = _golden(path)
    ci, pi, uv = g['camera_indices'], g['point_indices'], g['points_2d']
    scale = np.abs(g['f0']).max()                     # 1e-13 relative: what the reference has to reproduce
    for x, f in ((g['x0'], g['f0']), (g['x_final'], g['f_final'])):
        assert np.abs(ref.residual(x, C, P, ci, pi, uv, calib).ravel() - f).max() <= 1e-13 * scale
        # float64 and longdouble runs of the same code differ by float64 rounding only
        rl = ref.residual(x, C, P, ci, pi, uv, calib, np.longdouble).ravel()
        assert rl.dtype == np.longdouble and np.abs(rl - f).max() <= 1e-13 * scale


@pytest.mark.parametrize('path', BA_CASES, ids=os.path.basename)
def test_residual_equals_the_oracle_restatement(path):
    from oracle import ba_oracle
    g, C, P, calib = _golden(path)
    want = ba_oracle.residuals(g['x0'], C, P, g['camera_indices'], g['point_indices'], g['points_2d'],
                               g['K'], g['dist'], calib_global=calib is None)
    got = ref.residual(g['x0'], C, P, g['camera_indices'], g['point_indices'], g['points_2d'], calib)
    # (the bound the goldens' f0 is held to above: the oracle restatement reproduces f0 to 1e-13 too)
    assert np.abs(got.ravel() - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize('path', BA_CASES, ids=os.path.basename)
def test_jac_blocks_vs_golden_finite_differences(path):
    """1e-6 / 1e-5 (test_ba_gpu.py) is the accuracy of the goldens' J3, not of jac_blocks"""
    import scipy.sparse as sp
    g, C, P, calib = _golden(path)
    ci, pi = g['camera_indices'].astype(np.int64), g['point_indices'].astype(np.int64)
    Jc, Jp, Jk = ref.jac_blocks(g['x0'], C, P, ci, pi, g['points_2d'], calib)
    O, n = ci.size, g['x0'].size
    J3 = sp.csr_matrix((g['J3_data'], g['J3_indices'], g['J3_indptr']), shape=(2 * O, n)).toarray()
    rows = np.arange(2 * O).reshape(O, 2)
    ref_c = J3[rows[:, :, None], (ci[:, None] * 7 + np.arange(7))[:, None, :]]
    ref_p = J3[rows[:, :, None], (C * 7 + pi[:, None] * 3 + np.arange(3))[:, None, :]]
    assert np.abs(Jc - ref_c).max() / np.abs(ref_c).max() < 1e-6
    assert np.abs(Jp - ref_p).max() / np.abs(ref_p).max() < 1e-6
    if calib is None:
        ref_k = J3[:, C * 7 + P * 3:].reshape(O, 2, 8)
        for k in range(8):
            s = max(np.abs(ref_k[:, :, k]).max(), 1e-12)
            assert np.abs(Jk[:, :, k] - ref_k[:, :, k]).max() / s < 1e-5, k
    # ... and dense_A puts the blocks where the reference's Jacobian has them
    A = ref.dense_A(Jc, Jp, Jk, ci, pi, np.ones(n), np.full(n, 0.5), C, P).toarray()
    assert np.abs(A[:2 * O] - J3).max() <= 1e-5 * np.abs(J3).max()        # (J3's accuracy, as above)
    assert np.array_equal(A[2 * O:], 0.5 * np.identity(n))


def _sample(p):
    """a few observations of a problem: the largest |x| and |y| in the frame, the one nearest the
    principal point, the first, the last and (degenerate_q) one of the camera without a rotation"""
    off = p['uv'] - [ec.CU, ec.CV]
    pick = {int(np.abs(off[:, 0]).argmax()), int(np.abs(off[:, 1]).argmax()),
            int((off ** 2).sum(1).argmin()), 0, p['O'] - 1}
    deg = ref.degenerate_cameras(p['x0'], p['C'])[p['cam_idx']]
    if deg.any():
        pick.add(int(np.nonzero(deg)[0][0]))
    return sorted(pick)


def test_jac_reference_noise():
    """N_ref: jac_blocks() against mpmath (50 digits, central difference h = 1e-20) on observations
    drawn from every structure, per column group relative to the largest magnitude of the group in
    its problem.  The measured value stays below ba_reference.JAC_REF_NOISE, the constant the
    device tolerance (32 x) is derived from."""
    worst, n_obs = {}, 0
    for name in ec.NAMES:
        p = ec.make(name, 0, with_calib=True)
        C, P, x = p['C'], p['P'], p['x0']
        J = ref.jac_blocks(x, C, P, p['cam_idx'], p['pt_idx'], p['uv'], None)
        scales = ref.group_scales(*J)
        for o in _sample(p):
            c, q = int(p['cam_idx'][o]), int(p['pt_idx'][o])
            m = ref.jac_mp(x[c * 7:c * 7 + 7], x[C * 7 + q * 3:C * 7 + q * 3 + 3], p['uv'][o],
                           x[C * 7 + P * 3:], True)
            for k, v in ref.group_errors((J[0][o], J[1][o], J[2][o]), m, scales).items():
                worst[k] = max(worst.get(k, 0.0), v)
            n_obs += 1
    measured = max(worst.values())
    print('N_ref = %.3g over %d observations; per group: %s' % (
        measured, n_obs, ' '.join('%s=%.2g' % kv for kv in sorted(worst.items()))))
    assert n_obs >= 36
    assert 0 < measured <= ref.JAC_REF_NOISE
    assert ref.JAC_REF_NOISE <= 2 * measured          # the constant is the measurement, not a guess


def test_degenerate_quaternion_columns():
    p = ec.make('degenerate_q', 0, with_calib=False)
    deg = ref.degenerate_cameras(p['x0'], p['C'])
    assert deg.sum() == 1
    Jc, Jp, _ = ref.jac_blocks(p['x0'], p['C'], p['P'], p['cam_idx'], p['pt_idx'], p['uv'], p['calib'])
    sel = deg[p['cam_idx']]
    assert sel.sum() > 30 and np.all(Jc[sel, :, 3:] == 0) and np.all(Jc[~sel, :, 3:].any(axis=(1, 2)))
    # (d/d point = -d/d ned: two complex-step columns of the reference, each within its own noise)
    assert np.abs(Jp[sel] + Jc[sel, :, :3]).max() <= 2 * ref.JAC_REF_NOISE * np.abs(Jp).max()
    from oracle import ba_oracle
    want = ba_oracle.residuals(p['x0'], p['C'], p['P'], p['cam_idx'], p['pt_idx'], p['uv'],
                               np.array([[ec.F, 0, ec.CU], [0, ec.F, ec.CV], [0, 0, 1]]), ec.DIST)
    got = ref.residual(p['x0'], p['C'], p['P'], p['cam_idx'], p['pt_idx'], p['uv'], p['calib']).ravel()
    # (two summation orders of the same formulas: a few roundings of a coordinate of frame size)
    assert np.abs(got - want).max() <= 64 * ref.EPS * 2 * ec.CU


@pytest.mark.parametrize('with_calib', [False, True], ids=['plain', 'calib'])
def test_normal_blocks_vs_scipy_dense(with_calib):
    """A^T A blocks and S = U' - W V'^-1 W^T formed densely with SciPy on cams_n[3]"""
    import scipy.linalg as sl
    p = ec.make('cams_n-%d' % ec.CAMS_N[3], 0, with_calib)
    C, P, n = p['C'], p['P'], p['x0'].size
    A, b, d, dreg = ec.reference_system(p, ec.scaling)
    Jc, Jp, Jk = ref.jac_blocks(p['x0'], C, P, p['cam_idx'], p['pt_idx'], p['uv'], p['calib'])
    nb = ref.normal_blocks(Jc, Jp, Jk, b[:2 * p['O']], p['cam_idx'], p['pt_idx'], d, dreg, C, P)
    Ad = A.toarray()
    N = Ad.T @ Ad
    g = Ad.T @ b
    nc, npt = C * 7, P * 3
    cs = np.r_[0:nc, nc + npt:n]                       # the camera side: cameras (+ calibration)
    ps = np.r_[nc:nc + npt]
    # float64 dense products (any BLAS order) against the longdouble blocks: sum_bound with the
    # exact sum of |a_i b_i| of every entry, k = the rows of A
    m = Ad.shape[0]
    tolN = ref.sum_bound_k(np.abs(Ad).T @ np.abs(Ad), m)
    tolg = ref.sum_bound_k(np.abs(Ad).T @ np.abs(b), m)
    dc, dp = d[:nc].reshape(C, 7), d[nc:nc + npt].reshape(P, 3)
    for c in range(C):
        sl7 = slice(c * 7, c * 7 + 7)
        blk = N[sl7, sl7] - np.diag(dreg[sl7] ** 2)
        assert np.all(np.abs(dc[c][:, None] * nb['U'][c] * dc[c][None, :] - blk) <= tolN[sl7, sl7])
    for q in range(P):
        sl3 = slice(nc + q * 3, nc + q * 3 + 3)
        assert np.all(np.abs(nb['Vp'][q] - N[sl3, sl3]) <= tolN[sl3, sl3])
    assert np.all(np.abs((dc * nb['gc']).ravel() - g[:nc]) <= tolg[:nc])
    assert np.all(np.abs((dp * nb['gp']).ravel() - g[nc:nc + npt]) <= tolg[nc:nc + npt])
    # the dense Schur complement goes through SciPy's float64 inverse of the whole point block:
    # the kappa rule (64 eps kappa scale) with kappa of that block and the un-cancelled sums as scale
    W = N[np.ix_(cs, ps)]
    Vi = sl.inv(N[np.ix_(ps, ps)])
    S = N[np.ix_(cs, cs)] - W @ Vi @ W.T
    rhs = g[cs] - W @ Vi @ g[ps]
    kap = np.linalg.cond(N[np.ix_(ps, ps)])
    rule = 64 * ref.EPS * kap
    absS = np.abs(N[np.ix_(cs, cs)]) + np.abs(W) @ np.abs(Vi) @ np.abs(W.T)
    for c in range(C):
        sl7 = slice(c * 7, c * 7 + 7)
        assert np.all(np.abs(nb['Scc'][c] - S[sl7, sl7]) <= rule * absS[sl7, sl7])
    want_rhs = np.concatenate([nb['rhs'].ravel(), nb['rhs_k']]) if with_calib else nb['rhs'].ravel()
    assert np.all(np.abs(want_rhs - rhs) <= rule * (np.abs(g[cs]) + np.abs(W) @ np.abs(Vi) @ np.abs(g[ps])))
    y = np.random.default_rng(3).normal(size=cs.size)
    q, s_q = nb['apply'](y)
    assert np.all(np.abs(q - S @ y) <= rule * (absS @ np.abs(y)))
    assert np.all(s_q > 0)
    # the 3x3 / 7x7 longdouble inverses: the same n eps kappa rule with longdouble's round-off 2^-64
    rule_l = 64 * 2.0 ** -64
    assert np.all(np.abs(np.einsum('pij,pjk->pik', nb['Vinv'], nb['Vp']) - np.identity(3)).max((1, 2)) <= rule_l * nb['kV'])
    Si = ref.spd_inv(nb['Scc'])
    assert np.all(np.abs(np.einsum('cij,cjk->cik', Si, nb['Scc']) - np.identity(7)).max((1, 2)) <= rule_l * nb['kS'])


def test_sum_bound():
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(50, 300)), rng.normal(size=(50, 300))
    exact = (a.astype(np.longdouble) * b).sum(1)
    bound = ref.sum_bound(a.astype(np.longdouble) * b)
    assert np.all(np.abs((a * b).sum(1) - exact) <= bound)
    assert np.all(np.abs(np.cumsum(a * b, 1)[:, -1] - exact) <= bound)       # another order
    assert np.all(bound <= 8 * 316 * 2.0 ** -53 * np.abs(a * b).sum(1) * (1 + 4 * ref.EPS))       # (the same formula in float64)
    assert np.array_equal(ref.sum_bound_k(np.abs(a.astype(np.longdouble) * b).sum(1), 300), bound)


# ---- conditions the solver-level GPU comparisons rely on ----------------------------------------
@pytest.mark.parametrize('name', ec.LSMR_NAMES)
def test_lsmr_reference_is_reproducible(name):
    """SciPy's lsmr on two storage forms of the same A (CSR; dense -- for the 15400 x 9300 landmark
    case, 1.1 GB dense, the CSC form with rows and columns traversed in another order) agrees to
    1e-11 at k = 1, 2, 5: the 1e-10 / 1e-9 of the device comparison are then the device's own."""
    from scipy.sparse.linalg import lsmr
    p = ec.make(name, 0, with_calib=False)
    A, b, _, _ = ec.reference_system(p, ec.scaling_lsmr, seed=2)
    B = A.tocsc() if name == 'landmark' else A.toarray()
    for k in (1, 2, 5):
        xa = lsmr(A, b, atol=0, btol=0, conlim=0, maxiter=k)
        xb = lsmr(B, b, atol=0, btol=0, conlim=0, maxiter=k)
        assert xa[1] == xb[1] == 7 and xa[2] == xb[2] == k
        assert np.abs(xa[0] - xb[0]).max() <= 1e-11 * np.abs(xa[0]).max(), k


@pytest.fixture(scope='module')
def cond_mid():
    """cond of A for ba_mid.npz under the d / dreg recipe of the converged-Schur comparison"""
    g, C, P, calib = _golden(os.path.join(GOLDEN, 'ba_mid.npz'))
    p = dict(C=C, P=P, O=g['camera_indices'].size, cam_idx=g['camera_indices'], pt_idx=g['point_indices'],
             uv=g['points_2d'], x0=g['x0'], calib=calib)
    A, _, _, _ = ec.reference_system(p, ec.scaling_goldens)
    return np.linalg.cond(A.toarray())


@pytest.mark.parametrize('with_calib', [False, True], ids=['plain', 'calib'])
@pytest.mark.parametrize('name', ec.SCHUR_NAMES)
def test_schur_problems_no_worse_conditioned_than_ba_mid(name, with_calib, cond_mid):
    """the 2e-7 of test_ba_schur_gpu.py was set on the goldens (d = 1 / colnorm U(0.5, 2), dreg =
    U(1e-3, 3e-2)); it carries over to problems whose subproblem matrix is no worse conditioned than
    ba_mid's under that recipe.  The edge-case problems keep the recipe but draw dreg from
    ba_edge_cases.DREG_RANGE (see there).  landmark (A is 15425 x 9275: a dense SVD takes minutes):
    cond(A) = sqrt of the ratio of the extreme eigenvalues of the sparse A^T A by Lanczos (the
    smallest in shift-invert mode); it equals numpy's eigvalsh of the dense A^T A to 1e-10
    (853.4975 with calibration columns, 890.2827 without)."""
    p = ec.make(name, 0, with_calib)
    A, _, _, _ = ec.reference_system(p, ec.scaling)
    if name == 'landmark':
        from scipy.sparse.linalg import eigsh
        N = (A.T @ A).tocsc()
        hi = eigsh(N, k=1, which='LA', return_eigenvectors=False, tol=1e-10)[0]
        lo = eigsh(N, k=1, sigma=0, which='LM', return_eigenvectors=False, tol=1e-10)[0]
        c = np.sqrt(hi / lo)
    else:
        c = np.linalg.cond(A.toarray())
    print('cond(A) %s = %.3g, ba_mid = %.3g' % (name, c, cond_mid))
    assert c <= cond_mid


def test_structures_are_what_they_say():
    for P in ec.POINTS_N:
        p = ec.make('points_n-%d' % P)
        order = ec.internal_point_order(p['C'], P, p['cam_idx'], p['pt_idx'])
        counts = np.bincount(p['pt_idx'], minlength=P)[order]
        assert np.array_equal(counts, ec.points_n_counts(P)) and (order != np.arange(P)).any()
        assert {0, 1, 2, 3} <= set(counts.tolist())
        if P >= 256:
            assert counts[:256].sum() == 1024
        if P == 513:
            assert counts[256:512].sum() == 1025 and counts[511] > 1       # a point across two rounds
    for at in ('first', 'middle', 'last'):
        p = ec.make('lanes-' + at)
        assert sorted(np.bincount(p['cam_idx'], minlength=9).tolist()) == ec.LANES
    p = ec.make('landmark')
    assert p['C'] == 1025 and np.bincount(p['pt_idx']).max() == 1025
    for O in ec.RAGGED:
        assert ec.make('ragged-%d' % O)['O'] == O
    for name in ec.NAMES:
        a, b = ec.make(name), ec.make(name, shuffle=True)
        assert np.all(np.diff(a['cam_idx']) >= 0) and np.array_equal(a['cam_idx'], b['cam_idx'])
        if a['O'] > 3:
            assert not np.array_equal(a['pt_idx'], b['pt_idx'])
        pairs = set(zip(a['cam_idx'].tolist(), a['pt_idx'].tolist()))
        assert len(pairs) == a['O'] and pairs == set(zip(b['cam_idx'].tolist(), b['pt_idx'].tolist()))
