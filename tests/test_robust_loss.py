"""CPU: the numpy restatement of the robust loss factors (tests/robust_loss_restatement.py, what
csrc/ba_robust.hip is held to) against mpmath at 50 digits and against SciPy's own
construct_loss_function / scale_for_robust_loss_function.

The yardstick is SciPy's float64 error against mpmath on the same inputs: the restatement may be
no worse than max(16 x that, 64 . 2^-52) (the rule of test_pair_geometry.py), per input group.
SciPy's J_scale of Huber beyond z = 1 is rounding noise in [EPS, ~4 EPS] (z^-1/2 - z^-1/2 clipped):
it is left out of the yardstick, the restatement gives exactly sqrt(EPS) there, and the
well-conditioned product sqrt(J_scale) . f_scaled = rho' f is held to the rule instead."""
import numpy as np
import pytest

import robust_loss_restatement as rl

PARAMS = [(loss, C) for loss in rl.LOSSES for C in rl.F_SCALES]


@pytest.mark.parametrize('loss,C', PARAMS)
def test_restatement_against_mpmath_and_scipy(loss, C):
    for name, f in rl.cases(loss, C).items():
        ex = rl.exact(loss, f, C)
        rho, ff, fj = rl.restate(loss, f, C)
        s_rho, s_fs, s_sj = rl.scipy_values(loss, f, C)
        z = (f / C) ** 2
        clipped_huber = (z > 1.0) if loss == 'huber' else np.zeros(f.size, bool)
        keep = ~clipped_huber
        got = {'rho_c2': C * C * rho, 'fs': f * ff, 'sj': fj, 'prod': fj * (f * ff)}
        ref = {'rho_c2': s_rho, 'fs': s_fs, 'sj': s_sj, 'prod': s_sj * s_fs}
        for key in ('rho_c2', 'fs', 'sj', 'prod'):
            e_got, e_ref = rl.rel_err(got[key], ex[key]), rl.rel_err(ref[key], ex[key])
            sel = np.ones(f.size, bool) if key in ('rho_c2', 'prod') else keep
            bound = rl.rule(e_ref[sel])
            print('%s C=%g %s %s: restatement %.3g, SciPy %.3g, bound %.3g'
                  % (loss, C, name, key, e_got[sel].max(initial=0.0), e_ref[sel].max(initial=0.0), bound))
            assert np.all(e_got[sel] <= bound), (loss, C, name, key)
        # Huber beyond z = 1: exactly the clip, and SciPy's noise stays within a few EPS of it
        assert np.all(fj[clipped_huber] == rl.EPS ** 0.5)
        assert np.all((s_sj[clipped_huber] ** 2 >= rl.EPS) & (s_sj[clipped_huber] ** 2 <= 8 * rl.EPS))
        # the f factor of a clipped row is a power of two times rho': the product is rho' f again
        assert np.all(np.isfinite(ff) & np.isfinite(fj) & (fj >= rl.EPS ** 0.5) & (fj <= 1.0))


@pytest.mark.parametrize('loss', sorted(rl.BRANCH_Z))
@pytest.mark.parametrize('C', rl.F_SCALES)
def test_branch_inputs_straddle_the_branch_point(loss, C):
    """the 'branch' group has z on both sides of the branch point, within 4 ulp of it"""
    f = rl.branch_inputs(loss, C)
    z = (f / C) ** 2
    b = rl.BRANCH_Z[loss]
    assert (z <= b).any() and (z > b).any()
    assert np.abs(z[z <= b] - b).min() <= 4 * np.spacing(b)
    assert np.abs(z[z > b] - b).min() <= 4 * np.spacing(b)
    if loss != 'arctan':
        # both branches really are taken: J factor 1 / the clip (huber), unclipped / the clip (cauchy)
        fj = rl.restate(loss, f, C)[2]
        assert (fj == rl.EPS ** 0.5).any() and (fj > rl.EPS ** 0.5).any()


def test_identity_where_nothing_is_clipped():
    """Huber with every |f| <= C leaves f and J alone (factors exactly 1), and every loss tends to
    the linear one as z -> 0"""
    f = np.linspace(-1.0, 1.0, 41) * 400.0
    rho, ff, fj = rl.restate('huber', f, 400.0)
    assert np.all(ff == 1.0) and np.all(fj == 1.0) and np.array_equal(rho, (f / 400.0) ** 2)
    for loss in rl.LOSSES:
        rho, ff, fj = rl.restate(loss, np.array([1e-9, -1e-9]), 400.0)
        assert np.all(np.abs(ff - 1) <= 4 * rl.EPS) and np.all(np.abs(fj - 1) <= 4 * rl.EPS)


def test_cost_is_scipys_cost():
    from scipy.optimize._lsq.least_squares import construct_loss_function
    rng = np.random.default_rng(3)
    f = rng.normal(size=500) * 5.0
    for loss in rl.LOSSES:
        for C in rl.F_SCALES:
            ref = construct_loss_function(f.size, loss, C)(f, cost_only=True)
            got = 0.5 * C * C * rl.restate(loss, f, C)[0].sum()
            assert abs(got - ref) <= 1e-13 * ref, (loss, C)


def test_argument_checks_do_not_need_a_gpu():
    """null pointers, an unknown loss and a non-positive or non-finite f_scale: -1 before any launch"""
    import ctypes
    from imageanalysis_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()                       # (host memory: never dereferenced)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.iamx_ba_robust_cost(None, 4, 2, 1.0, p, p, None) == -1
    assert b'null pointer' in L.iamx_last_error()
    assert L.iamx_ba_robust_cost(p, 4, 2, 1.0, None, p, None) == -1
    assert L.iamx_ba_robust_cost(p, 4, 2, 1.0, p, None, None) == -1
    assert L.iamx_ba_robust_scale(None, p, p, None, 2, 2, 1.0, None) == -1
    assert L.iamx_ba_robust_scale(p, None, p, None, 2, 2, 1.0, None) == -1
    assert L.iamx_ba_robust_scale(p, p, None, None, 2, 2, 1.0, None) == -1
    for loss in (0, 5, -1):                               # (0 = linear: needs neither call)
        assert L.iamx_ba_robust_cost(p, 4, loss, 1.0, p, p, None) == -1
        assert b'unknown loss' in L.iamx_last_error()
        assert L.iamx_ba_robust_scale(p, p, p, None, 2, loss, 1.0, None) == -1
    for C in (0.0, -1.0, float('inf'), float('nan')):
        assert L.iamx_ba_robust_cost(p, 4, 2, C, p, p, None) == -1
        assert b'f_scale' in L.iamx_last_error()
        assert L.iamx_ba_robust_scale(p, p, p, None, 2, 2, C, None) == -1
    assert L.iamx_ba_robust_scale(p, p, p, None, -1, 2, 1.0, None) == -1
    assert L.iamx_ba_robust_scale(p, p, p, None, 0, 2, 1.0, None) == 0       # nothing to do: no launch


def test_loss_ids_match_the_header():
    import os
    import re
    from conftest import REPO
    from imageanalysis_amd import ba_solver
    text = open(os.path.join(REPO, 'include', 'iamx.h')).read()
    ids = {k.lower(): int(v) for k, v in re.findall(r'IAMX_LOSS_([A-Z0-9_]+) = (\d+)', text)}
    assert ids == ba_solver.LOSSES == rl.LOSS_ID


def test_unknown_loss_is_refused_before_any_device_work():
    from imageanalysis_amd import ba_solver, optimizer
    opt = optimizer.Optimizer('/nonexistent')
    assert (opt.loss, opt.f_scale) == ('linear', 1.0)
    opt.loss = 'nope'
    with pytest.raises(ValueError):
        opt.run()                                         # (nothing is set up: the check comes first)
    opt.loss, opt.f_scale = 'soft_l1', 0.0
    with pytest.raises(ValueError):
        opt.run()
    with pytest.raises(ValueError):
        ba_solver.check_loss('soft_l1', float('nan'))
    assert ba_solver.check_loss('cauchy', 3) == ('cauchy', 3.0)
