"""TEST HELPER (host only): the robust loss functions of csrc/ba_robust.hip in numpy, operation by
operation, and their yardsticks.

scipy.optimize.least_squares(loss=, f_scale=) per scalar residual f, C = f_scale, z = (f / C)^2:

    cost = 0.5 C^2 sum rho(z);  J_scale = max(rho' + 2 rho'' z, EPS);
    f <- f rho' / sqrt(J_scale);  row of J <- row of J . sqrt(J_scale)

* restate()      (rho(z), factor of f, factor of the row of J) with the closed forms of J_scale the
                 kernels use -- float64, the same operations in the same order.
* scipy_values() the same three through SciPy's own construct_loss_function and
                 scale_for_robust_loss_function (what the kernels have to reproduce).
* exact()        the three, and the product rho' f, in mpmath at 50 digits.  rho, rho', rho'' are
                 functions of z, and both SciPy and the kernels form z = fl(fl(f / C)^2) first, so the
                 float64 z is the exact argument here: the branch a value takes (Huber z <= 1, the
                 clip) is then the same for everybody and the discontinuities stay out of the errors.
* rel_err()      |x - exact| / |exact| in mpmath (0 where both are 0).
* rule()         the bound of tests/test_pair_geometry.py: max(16 x SciPy's own error on the same
                 inputs, 64 . 2^-52).
* cases()        the inputs: signed values, 0 and +-1e-300, z next to every branch point, z up to 1e12.

Nothing here imports the device side of imageanalysis_amd.
"""
import numpy as np

EPS = 2.0 ** -52
FLOOR = 64 * EPS
LOSSES = ('huber', 'soft_l1', 'cauchy', 'arctan')
LOSS_ID = {'linear': 0, 'huber': 1, 'soft_l1': 2, 'cauchy': 3, 'arctan': 4}      # include/iamx.h
F_SCALES = (0.5, 2.0, 400.0)
# z at which a loss changes its formula or its J_scale reaches the clip
BRANCH_Z = {'huber': 1.0, 'cauchy': 1.0, 'arctan': 3.0 ** -0.5}


def restate(loss, f, f_scale):
    """(rho(z), f factor, J factor) as ba_robust.hip computes them"""
    f = np.asarray(f, np.float64)
    s = f / np.float64(f_scale)
    z = s * s
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if loss == 'huber':
            small = z <= 1.0
            rz = np.sqrt(z)
            rho = np.where(small, z, 2.0 * rz - 1.0)
            d1 = np.where(small, 1.0, 1.0 / rz)
            js = np.where(small, 1.0, 0.0)
        elif loss == 'soft_l1':
            t = 1.0 + z
            q = np.sqrt(t)
            rho = 2.0 * (z / (q + 1.0))
            d1 = 1.0 / q
            js = 1.0 / (t * q)
        elif loss == 'cauchy':
            t = 1.0 + z
            rho = np.log1p(z)
            d1 = 1.0 / t
            js = (1.0 - z) / (t * t)
        elif loss == 'arctan':
            z2 = z * z
            t = 1.0 + z2
            rho = np.arctan(z)
            d1 = 1.0 / t
            js = (1.0 - 3.0 * z2) / (t * t)
        else:
            raise ValueError(loss)
    js = np.where(js < EPS, EPS, js)
    fj = np.sqrt(js)
    return rho, d1 / fj, fj


def scipy_values(loss, f, f_scale):
    """(C^2 rho(z), scaled f, sqrt(J_scale)) from SciPy's own functions"""
    from scipy.optimize._lsq.common import scale_for_robust_loss_function
    from scipy.optimize._lsq.least_squares import construct_loss_function
    f = np.array(f, np.float64)
    rho = construct_loss_function(f.size, loss, f_scale)(f)
    J, fs = scale_for_robust_loss_function(np.ones((f.size, 1)), f.copy(), rho)
    return rho[0].copy(), fs, np.asarray(J)[:, 0].copy()


def exact(loss, f, f_scale, digits=50):
    """dict of lists of mpf: rho_c2 = C^2 rho(z), fs = f rho' / sqrt(J_scale), sj = sqrt(J_scale),
    prod = rho' f -- of the float64 z = fl(fl(f / C)^2)"""
    import mpmath as mp
    f = np.asarray(f, np.float64)
    zs = (f / np.float64(f_scale)) ** 2
    out = dict(rho_c2=[], fs=[], sj=[], prod=[])
    with mp.workdps(digits):
        C, eps = mp.mpf(float(f_scale)), mp.mpf(EPS)
        for fi, zi in zip(f.tolist(), zs.tolist()):
            F, z = mp.mpf(fi), mp.mpf(zi)
            if loss == 'huber':
                if z <= 1:
                    rho, d1, d2 = z, mp.mpf(1), mp.mpf(0)
                else:
                    rho, d1, d2 = 2 * mp.sqrt(z) - 1, 1 / mp.sqrt(z), -1 / (2 * z * mp.sqrt(z))
            elif loss == 'soft_l1':
                t = 1 + z
                rho, d1, d2 = 2 * (mp.sqrt(t) - 1), 1 / mp.sqrt(t), -1 / (2 * t * mp.sqrt(t))
            elif loss == 'cauchy':
                t = 1 + z
                rho, d1, d2 = mp.log(t), 1 / t, -1 / (t * t)
            elif loss == 'arctan':
                t = 1 + z * z
                rho, d1, d2 = mp.atan(z), 1 / t, -2 * z / (t * t)
            else:
                raise ValueError(loss)
            js = d1 + 2 * d2 * z
            if js < eps:
                js = eps
            sj = mp.sqrt(js)
            out['rho_c2'].append(C * C * rho)
            out['fs'].append(F * d1 / sj)
            out['sj'].append(sj)
            out['prod'].append(d1 * F)
    return out


def rel_err(values, ref, digits=50):
    """float64 array of |x - ref| / |ref| (0 where both are 0, inf where only ref is)"""
    import mpmath as mp
    out = np.empty(len(ref))
    with mp.workdps(digits):
        for i, (x, r) in enumerate(zip(np.asarray(values, np.float64).tolist(), ref)):
            if r == 0:
                out[i] = 0.0 if x == 0 else np.inf
            else:
                out[i] = float(abs(mp.mpf(x) - r) / abs(r))
    return out


def rule(scipy_err):
    """no worse than max(16 x SciPy's own error on the case, 64 . 2^-52)"""
    e = float(np.max(scipy_err)) if np.size(scipy_err) else 0.0
    return max(16.0 * e, FLOOR)


def _ulp_steps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def branch_inputs(loss, f_scale):
    """f (both signs) whose z lies next to the branch point of `loss` on either side: the doubles
    within 4 ulp of C sqrt(z_b) -- fl(s^2) cannot reach every double next to z_b, these are the
    nearest it does reach"""
    if loss not in BRANCH_Z:
        return np.zeros(0)
    f0 = np.float64(f_scale) * np.sqrt(np.float64(BRANCH_Z[loss]))
    f = np.array([_ulp_steps(f0, k) for k in range(-4, 5)])
    return np.concatenate([f, -f])


def cases(loss, f_scale, rng=None):
    """name -> f: the input groups, each with a yardstick of its own"""
    rng = np.random.default_rng(11) if rng is None else rng
    C = float(f_scale)
    mag = C * 10.0 ** rng.uniform(-3, 1.5, 64)                    # z from 1e-6 to 1e3
    out = {'signed': mag * rng.choice([-1.0, 1.0], mag.size),
           'tiny': np.array([0.0, -0.0, 1e-300, -1e-300]),
           'large': C * np.array([1e2, -1e3, 1e4, -1e5, 9.99e5, 1e6, -1e6])}        # z up to 1e12
    b = branch_inputs(loss, f_scale)
    if b.size:
        out['branch'] = b
    return out
