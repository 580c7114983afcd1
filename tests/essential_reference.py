"""Shared by tests/test_match_verify_essential.py (host) and tests/test_match_verify_essential_gpu.py:
the reference of iamx_verify_pairs_essential / iamx_five_point (csrc/five_point.h, match_verify.hip)
and the seeded inputs of their tests.  Scenes, the sampling rule and the error measure come from
verify_reference.py.

* rays(): pixels -> calibrated rays, the rule of include/iamx.h.
* solve(): every sample of a pair at once over a dtype, following the kernel's construction step by
  step (full-pivot null space, the 10x20 constraint matrix in the header's monomial order, the
  degree-10 polynomial, the derivative-chain bisection, the models).  solve64 = solve(.., float64);
  numpy.longdouble is the evaluation the flags are measured against.
* solve_mp(): ONE sample at 60 digits: the same construction up to the polynomial, then
  mpmath.polyroots; all real solutions, as (E [m, 9], F [m, 9]) in longdouble.
* consensus(): all candidates (hypothesis, root) of a pair, lower / upper inlier counts about the
  guard band, a flag where the float64 candidate is further than FLAG from every longdouble one.

Needs numpy and mpmath only; every input comes from a seed.
"""
import functools

import numpy as np

import verify_reference as vr

ESSENTIAL = 2
SAMPLE = 5
MAX_ROOTS = 10
KMAT = vr.KMAT
TOL = vr.TOL
OK, TOO_FEW, NO_MODEL = vr.OK, vr.TOO_FEW, vr.NO_MODEL
BISECT_INNER, BISECT_LAST, NEWTON = 32, 48, 2

# the monomials of the constraint matrix in the order of include/iamx.h, degree <= 3 in x, y, z
MON3 = ('xxx', 'xxy', 'xyy', 'yyy', 'xxz', 'xx', 'xyz', 'xy', 'yyz', 'yy',
        'xzz', 'xz', 'x', 'yzz', 'yz', 'y', 'zzz', 'zz', 'z', '')
MON2 = ('xx', 'xy', 'yy', 'xz', 'yz', 'zz', 'x', 'y', 'z', '')
MON1 = ('x', 'y', 'z', '')
T11 = [[MON2.index(''.join(sorted(a + b))) for b in MON1] for a in MON1]
T21 = [[MON3.index(''.join(sorted(a + b))) for b in MON1] for a in MON2]

# Measured by measure() below (python tests/essential_reference.py) on the asserted cases, both
# seeds, UNSTABLE left out.
# FLOOR_E: 16 x solve64's median distance to the exact solution over the 144 solver samples (608
#   exact real solutions, none missed; median 6.32e-15, largest 1.17e-08).
# FLAG: 16 x the largest distance of a chosen float64 candidate from the nearest longdouble candidate
#   of its sample (7.5e-14, E-n6).
# BAND: 16 x the largest relative disagreement between the float64 and the longdouble evaluation of
#   the error measure under a chosen model, over the matches within [tol^2 / 4, 4 tol^2] (1.2e-12).
FLOOR_E = 16 * 6.32e-15
FLAG = 16 * 7.5e-14
BAND = 16 * 1.2e-12
MISS = 1e-6          # a solution further than this from every candidate counts as missed: distinct
#                      solutions of a sample lie O(0.1) apart, and a double root costs half the digits
#                      (sqrt(eps) = 1.5e-8), so 1e-6 separates "found, ill conditioned" from "not found"

# With every image 1 point on one line the 5x9 null space holds a three-dimensional family of rank-1
# matrices that satisfy all ten constraints: the polynomial system is degenerate, whether a sample is
# passed over is decided by rounding, and float64 and longdouble disagree on which candidates exist.
# The GPU test checks the status, the model's form and the mask against the float64 expression there.
UNSTABLE = ('E-collinear',)


def rays(points, K, dtype=np.float64):
    """[n, 4] pixels -> [n, 4] rays: y = (v - cv) / fy, x = ((u - cu) - skew y) / fx"""
    p = np.asarray(points, np.float32).astype(dtype)
    K = np.asarray(K, np.float64).astype(dtype)
    out = np.zeros_like(p)
    for a in (0, 2):
        y = (p[:, a + 1] - K[1, 2]) / K[1, 1]
        out[:, a + 1] = y
        out[:, a] = ((p[:, a] - K[0, 2]) - K[0, 1] * y) / K[0, 0]
    return out


# ---------------------------------------------------------------------------------------------
# the construction over a dtype, every sample at once
# ---------------------------------------------------------------------------------------------
def null_basis(r):
    """r [H, 5, 4] rays of the samples -> (basis [H, 4, 9] = X Y Z W, ok [H])"""
    H, dtype = len(r), r.dtype
    x, y, u, v = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], axis=2)   # [H, 5, 9]
    ar = np.arange(H)
    thr = np.abs(A).reshape(H, -1).max(1) * dtype.type(2.0 ** -40)
    used_r = np.zeros((H, 5), bool)
    used_c = np.zeros((H, 9), bool)
    pivcol = np.zeros((H, 5), np.int64)
    ok = np.ones(H, bool)
    with np.errstate(all='ignore'):
        for _step in range(5):
            v_ = np.where(used_r[:, :, None] | used_c[:, None, :], -1, np.abs(A))
            v_ = np.where(np.isnan(v_), -1, v_)
            flat = np.argmax(v_.reshape(H, -1), axis=1)       # first of the largest: lowest row, then column
            pr, pc = flat // 9, flat % 9
            piv = v_[ar, pr, pc]
            ok &= piv > thr
            prow = A[ar, pr, :]
            f = A[ar, :, pc] / prow[ar, pc][:, None]          # [H, 5]
            new = A - f[:, :, None] * prow[:, None, :]
            new[ar, :, pc] = 0
            is_p = np.arange(5)[None, :] == pr[:, None]
            A = np.where(is_p[:, :, None], A, new)
            used_r[ar, pr] = True
            used_c[ar, pc] = True
            pivcol[ar, pr] = pc
        free = np.argsort(used_c, axis=1, kind='stable')[:, :4]          # the free columns, ascending
        basis = np.zeros((H, 4, 9), dtype)
        for k in range(4):
            fk = free[:, k]
            basis[ar, k, fk] = 1
            for row in range(5):
                pc = pivcol[:, row]
                basis[ar, k, pc] = -A[ar, row, fk] / A[ar, row, pc]
    return basis, ok


def _mul11(p, q):
    out = np.zeros(p.shape[:-1] + (10,), p.dtype)
    for a in range(4):
        for b in range(4):
            out[..., T11[a][b]] = out[..., T11[a][b]] + p[..., a] * q[..., b]
    return out


def _mul21(p, q):
    out = np.zeros(p.shape[:-1] + (20,), p.dtype)
    for a in range(10):
        for b in range(4):
            out[..., T21[a][b]] = out[..., T21[a][b]] + p[..., a] * q[..., b]
    return out


def constraints(basis):
    """basis [H, 4, 9] -> the 10 x 20 matrices [H, 10, 20]: row 0 det E, rows 1 + 3 i + j the
    entries of (E E^T - tr(E E^T) / 2) E"""
    H = len(basis)
    E = [[np.ascontiguousarray(basis[:, :, 3 * i + j]) for j in range(3)] for i in range(3)]   # [H, 4] each
    A = np.zeros((H, 10, 20), basis.dtype)
    m0 = _mul11(E[1][1], E[2][2]) - _mul11(E[1][2], E[2][1])
    m1 = _mul11(E[1][0], E[2][2]) - _mul11(E[1][2], E[2][0])
    m2 = _mul11(E[1][0], E[2][1]) - _mul11(E[1][1], E[2][0])
    A[:, 0] = (_mul21(m0, E[0][0]) - _mul21(m1, E[0][1])) + _mul21(m2, E[0][2])
    M = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            M[i][j] = (_mul11(E[i][0], E[j][0]) + _mul11(E[i][1], E[j][1])) + _mul11(E[i][2], E[j][2])
            M[j][i] = M[i][j]
    t = basis.dtype.type(0.5) * ((M[0][0] + M[1][1]) + M[2][2])
    L = [[M[i][j] - t if i == j else M[i][j] for j in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(3):
            A[:, 1 + 3 * i + j] = (_mul21(L[i][0], E[0][j]) + _mul21(L[i][1], E[1][j])) + _mul21(L[i][2], E[2][j])
    return A


def eliminate(A):
    """Gauss-Jordan of the leading 10 x 10 block, row pivoting with the rows swapped into place:
    (A reduced [H, 10, 20], ok [H])"""
    A = A.copy()
    H, dtype = len(A), A.dtype
    ar = np.arange(H)
    with np.errstate(all='ignore'):
        thr = np.abs(A).reshape(H, -1).max(1) * dtype.type(2.0 ** -40)
        ok = np.ones(H, bool)
        for c in range(10):
            v = np.abs(A[:, c:, c])
            v = np.where(np.isnan(v), -1, v)
            who = c + np.argmax(v, axis=1)
            ok &= v[ar, who - c] > thr
            tmp = A[ar, who].copy()
            A[ar, who] = A[:, c]
            A[:, c] = tmp
            A[:, c] = A[:, c] / A[:, c, c][:, None]
            f = A[:, :, c].copy()
            new = A - f[:, :, None] * A[:, c][:, None, :]
            new[:, :, c] = 0
            new[:, c] = A[:, c]
            A = new
    return A, ok


def _conv(a, b):
    la, lb = a.shape[-1], b.shape[-1]
    out = np.zeros(a.shape[:-1] + (la + lb - 1,), a.dtype)
    for k in range(la + lb - 1):
        for i in range(la):
            if 0 <= k - i < lb:
                out[..., k] = out[..., k] + a[..., i] * b[..., k - i]
    return out


def b_matrix(A):
    """B [3][3] of coefficient arrays (ascending powers of z): lengths 4, 4, 5"""
    B = []
    for hi, lo in ((4, 5), (6, 7), (8, 9)):
        row = []
        for last, deg in ((12, 2), (15, 2), (19, 3)):
            h = [A[:, hi, last - p] for p in range(deg + 1)]
            l = [A[:, lo, last - p] for p in range(deg + 1)]
            co = [h[0]] + [h[p] - l[p - 1] for p in range(1, deg + 1)] + [-l[deg]]
            row.append(np.stack(co, axis=1))
        B.append(row)
    return B


def polynomial(B):
    """det B(z): [H, 11], ascending powers"""
    p1 = _conv(B[1][1], B[2][2]) - _conv(B[1][2], B[2][1])
    p2 = _conv(B[1][0], B[2][2]) - _conv(B[1][2], B[2][0])
    p3 = _conv(B[1][0], B[2][1]) - _conv(B[1][1], B[2][0])
    return (_conv(B[0][0], p1) - _conv(B[0][1], p2)) + _conv(B[0][2], p3)


def _horner(q, z):
    """q [H, k + 1] ascending, z [H]"""
    v = q[:, -1].copy()
    for i in range(q.shape[1] - 2, -1, -1):
        v = v * z + q[:, i]
    return v


def real_roots(c):
    """The root rule of include/iamx.h on c [H, 11]: (roots [H, 10] ascending, NaN past count;
    count [H]; ok [H])"""
    H, dtype = len(c), c.dtype
    one, half = dtype.type(1), dtype.type(0.5)
    with np.errstate(all='ignore'):
        lead = np.abs(c[:, 10])
        R = one + np.abs(c[:, :10]).max(1) / lead
        ok = np.isfinite(c).all(1) & (lead > 0) & np.isfinite(R)
        R = np.where(ok, R, one)
        c = np.where(ok[:, None], c, 0 * c + one)
        D = [c]
        for j in range(1, 10):
            D.append(D[-1][:, 1:] * np.arange(1, D[-1].shape[1], dtype=np.float64).astype(dtype)[None, :])
        roots = np.zeros((H, 0), dtype)
        count = np.zeros(H, np.int64)
        ar = np.arange(H)
        for k in range(1, 11):
            q = D[10 - k]
            last = k == 10
            pts = np.concatenate([-R[:, None], roots, R[:, None]], axis=1)       # [H, k + 1], unused = R
            new = np.tile(R[:, None], (1, k))
            ncount = np.zeros(H, np.int64)
            fa = _horner(q, pts[:, 0])
            for i in range(k):
                a, b = pts[:, i], pts[:, i + 1]
                fb = _horner(q, b)
                sa = fa < 0
                has = (sa != (fb < 0)) & (i <= count)
                lo, hi = a.copy(), b.copy()
                for _it in range(BISECT_LAST if last else BISECT_INNER):
                    mid = half * (lo + hi)
                    same = (_horner(q, mid) < 0) == sa
                    lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
                z = half * (lo + hi)
                if last:
                    for _it in range(NEWTON):
                        zn = z - _horner(q, z) / _horner(D[1], z)
                        z = np.where((zn >= a) & (zn <= b), zn, z)
                rows = ar[has]
                new[rows, ncount[rows]] = z[rows]
                ncount[rows] += 1
                fa = fb
            roots, count = new, ncount
        roots = np.where(np.arange(10)[None, :] < count[:, None], roots, np.nan)
        count = np.where(ok, count, 0)
    return roots, count, ok


def _unit(M):
    """[.., 9] -> unit Frobenius norm, largest-magnitude entry positive"""
    with np.errstate(all='ignore'):
        ss = np.zeros(M.shape[:-1], M.dtype)
        for j in range(9):
            ss = ss + M[..., j] * M[..., j]
        M = M / np.sqrt(ss)[..., None]
        big = np.argmax(np.where(np.isnan(M), -1, np.abs(M)), axis=-1)
        val = np.take_along_axis(M, big[..., None], axis=-1)
        return M * np.where(val < 0, -1, 1).astype(M.dtype)


def pixel_model(E, K):
    """E [.., 9] on rays -> F = K^-T E K^-1 [.., 9], in the closed form of the header, unit norm"""
    dtype = E.dtype.type
    K = np.asarray(K, np.float64).astype(E.dtype)
    with np.errstate(all='ignore'):
        a, d = dtype(1) / K[0, 0], dtype(1) / K[1, 1]
        b = -((K[0, 1] * d) * a)
        c = -(a * K[0, 2] + b * K[1, 2])
        e = -(d * K[1, 2])
        G = np.zeros(E.shape, E.dtype)
        for i in range(3):
            G[..., 3 * i] = E[..., 3 * i] * a
            G[..., 3 * i + 1] = E[..., 3 * i] * b + E[..., 3 * i + 1] * d
            G[..., 3 * i + 2] = (E[..., 3 * i] * c + E[..., 3 * i + 1] * e) + E[..., 3 * i + 2]
        F = np.zeros(E.shape, E.dtype)
        for j in range(3):
            F[..., j] = a * G[..., j]
            F[..., 3 + j] = b * G[..., j] + d * G[..., 3 + j]
            F[..., 6 + j] = (c * G[..., j] + e * G[..., 3 + j]) + G[..., 6 + j]
        return _unit(F)


def models(basis, B, roots):
    """per root the model on rays: E [H, 10, 9] unit norm (NaN past the count)"""
    H, dtype = len(basis), basis.dtype
    E = np.full((H, 10, 9), np.nan, dtype)
    with np.errstate(all='ignore'):
        for r in range(10):
            z = roots[:, r]
            rows = np.stack([np.stack([_horner(B[k][j], z) for j in range(3)], axis=1) for k in range(3)], axis=1)
            best, bn = None, None
            for p, q in ((0, 1), (0, 2), (1, 2)):
                u, v = rows[:, p], rows[:, q]
                cr = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                               u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
                nn = (cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2]
                if best is None:
                    best, bn = cr, nn
                else:
                    take = nn > bn
                    best, bn = np.where(take[:, None], cr, best), np.where(take, nn, bn)
            x, y = best[:, 0] / best[:, 2], best[:, 1] / best[:, 2]
            Er = ((x[:, None] * basis[:, 0] + y[:, None] * basis[:, 1]) + z[:, None] * basis[:, 2]) + basis[:, 3]
            E[:, r] = _unit(Er)
    return E


def solve_rays(r):
    """r [H, 5, 4] -> (E [H, 10, 9], count [H]): the solver alone (iamx_five_point).  Candidates
    that are not finite are NOT removed here."""
    with np.errstate(all='ignore'):
        basis, ok1 = null_basis(r)
        A, ok2 = eliminate(constraints(basis))
        B = b_matrix(A)
        roots, count, ok3 = real_roots(polynomial(B))
        E = models(basis, B, roots)
    ok = ok1 & ok2 & ok3
    E[~ok] = np.nan
    return E, np.where(ok, count, 0)


def solve(points, K, idx, dtype=np.float64):
    """the candidates of the samples idx [H, 5]: (E [H, 10, 9], F [H, 10, 9], valid [H, 10]); valid:
    a root exists there and its E and F are finite"""
    r = rays(points, K, dtype)[np.asarray(idx)]
    E, count = solve_rays(r)
    F = pixel_model(E, K)
    valid = (np.arange(10)[None, :] < count[:, None]) & np.isfinite(E).all(2) & np.isfinite(F).all(2)
    return E, F, valid


def solve64(points, K, idx):
    return solve(points, K, idx, np.float64)


# ---------------------------------------------------------------------------------------------
# one sample at 60 digits
# ---------------------------------------------------------------------------------------------
def solve_mp(points, K, idx, rays_in=None):
    """all real solutions of ONE sample: (E [m, 9], F [m, 9]) longdouble, unit norm, ascending z.
    rays_in [5, 4]: solve these rays and not points[idx]."""
    import mpmath as mp
    with mp.workdps(vr.MP_DIGITS):
        f = lambda v: mp.mpf(float(v))
        Km = [[f(v) for v in row] for row in np.asarray(K, np.float64)]
        if rays_in is None:
            rs = []
            for i in idx:
                p = [f(v) for v in np.asarray(points, np.float32)[i]]
                y1, y2 = (p[1] - Km[1][2]) / Km[1][1], (p[3] - Km[1][2]) / Km[1][1]
                rs.append([((p[0] - Km[0][2]) - Km[0][1] * y1) / Km[0][0], y1,
                           ((p[2] - Km[0][2]) - Km[0][1] * y2) / Km[0][0], y2])
        else:
            rs = [[f(v) for v in row] for row in np.asarray(rays_in, np.float64)]
        A = mp.matrix([[u * x, u * y, u, v * x, v * y, v, x, y, mp.mpf(1)] for x, y, u, v in rs])
        # null space by Gauss-Jordan with full pivoting (any route gives the same solution set)
        A = [list(A[i, :]) for i in range(5)]
        rows, cols, piv = [], [], {}
        for _ in range(5):
            best = max(((abs(A[i][j]), -i, -j) for i in range(5) if i not in rows
                        for j in range(9) if j not in cols))
            i, j = -best[1], -best[2]
            if best[0] == 0:
                return np.zeros((0, 9), np.longdouble), np.zeros((0, 9), np.longdouble)
            rows.append(i), cols.append(j)
            piv[i] = j
            for r in range(5):
                if r != i:
                    g = A[r][j] / A[i][j]
                    A[r] = [A[r][k] - g * A[i][k] for k in range(9)]
        free = [j for j in range(9) if j not in cols]
        basis = []
        for fk in free:
            b = [mp.mpf(0)] * 9
            b[fk] = mp.mpf(1)
            for i in range(5):
                b[piv[i]] = -A[i][fk] / A[i][piv[i]]
            basis.append(b)
        # polynomials as dicts: sorted monomial string -> coefficient
        def pmul(p, q):
            out = {}
            for ka, va in p.items():
                for kb, vb in q.items():
                    k = ''.join(sorted(ka + kb))
                    out[k] = out.get(k, 0) + va * vb
            return out

        def padd(p, q, s=1):
            out = dict(p)
            for k, v in q.items():
                out[k] = out.get(k, 0) + s * v
            return out
        Ep = [[{m: basis[k][3 * i + j] for k, m in enumerate(MON1)} for j in range(3)] for i in range(3)]
        det = padd(padd(pmul(padd(pmul(Ep[1][1], Ep[2][2]), pmul(Ep[1][2], Ep[2][1]), -1), Ep[0][0]),
                        pmul(padd(pmul(Ep[1][0], Ep[2][2]), pmul(Ep[1][2], Ep[2][0]), -1), Ep[0][1]), -1),
                   pmul(padd(pmul(Ep[1][0], Ep[2][1]), pmul(Ep[1][1], Ep[2][0]), -1), Ep[0][2]))
        M = [[padd(padd(pmul(Ep[i][0], Ep[j][0]), pmul(Ep[i][1], Ep[j][1])), pmul(Ep[i][2], Ep[j][2]))
              for j in range(3)] for i in range(3)]
        t = {k: v / 2 for k, v in padd(padd(M[0][0], M[1][1]), M[2][2]).items()}
        cons = [det]
        for i in range(3):
            for j in range(3):
                acc = {}
                for k in range(3):
                    L = padd(M[i][k], t, -1) if i == k else M[i][k]
                    acc = padd(acc, pmul(L, Ep[k][j]))
                cons.append(acc)
        C = [[c.get(m, mp.mpf(0)) for m in MON3] for c in cons]
        for c in range(10):
            who = max(range(c, 10), key=lambda r: abs(C[r][c]))
            C[c], C[who] = C[who], C[c]
            if C[c][c] == 0:
                return np.zeros((0, 9), np.longdouble), np.zeros((0, 9), np.longdouble)
            C[c] = [v / C[c][c] for v in C[c]]
            for r in range(10):
                if r != c:
                    g = C[r][c]
                    C[r] = [C[r][k] - g * C[c][k] for k in range(20)]
        def conv(a, b):
            out = [mp.mpf(0)] * (len(a) + len(b) - 1)
            for i, va in enumerate(a):
                for j, vb in enumerate(b):
                    out[i + j] += va * vb
            return out
        sub = lambda a, b: [x - y for x, y in zip(a, b)]
        add = lambda a, b: [x + y for x, y in zip(a, b)]
        B = []
        for hi, lo in ((4, 5), (6, 7), (8, 9)):
            row = []
            for last, deg in ((12, 2), (15, 2), (19, 3)):
                h = [C[hi][last - p] for p in range(deg + 1)] + [mp.mpf(0)]
                l = [mp.mpf(0)] + [C[lo][last - p] for p in range(deg + 1)]
                row.append(sub(h, l))
            B.append(row)
        p1 = sub(conv(B[1][1], B[2][2]), conv(B[1][2], B[2][1]))
        p2 = sub(conv(B[1][0], B[2][2]), conv(B[1][2], B[2][0]))
        p3 = sub(conv(B[1][0], B[2][1]), conv(B[1][1], B[2][0]))
        poly = add(sub(conv(B[0][0], p1), conv(B[0][1], p2)), conv(B[0][2], p3))
        zs = mp.polyroots(poly[::-1], maxsteps=500, extraprec=400)
        scale = max(abs(z) for z in zs) + 1
        real = sorted(z.real for z in zs if abs(z.imag) <= scale * mp.mpf(10) ** -30)
        Es, Fs = [], []
        Ki = mp.matrix(Km) ** -1
        for z in real:
            ev = lambda q: sum((cf * z ** k for k, cf in enumerate(q)), mp.mpf(0))
            rws = [[ev(B[k][j]) for j in range(3)] for k in range(3)]
            cands = []
            for p, q in ((0, 1), (0, 2), (1, 2)):
                u, v = rws[p], rws[q]
                cr = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
                cands.append((sum(w * w for w in cr), cr))
            cr = max(cands, key=lambda cc: cc[0])[1]
            x, y = cr[0] / cr[2], cr[1] / cr[2]
            E = [x * basis[0][k] + y * basis[1][k] + z * basis[2][k] + basis[3][k] for k in range(9)]
            Fm = Ki.T * mp.matrix([E[0:3], E[3:6], E[6:9]]) * Ki
            Fv = [Fm[i, j] for i in range(3) for j in range(3)]
            for vec, dst in ((E, Es), (Fv, Fs)):
                nrm = mp.sqrt(sum(w * w for w in vec))
                big = max(range(9), key=lambda k: (abs(vec[k]), -k))
                sg = -1 if vec[big] < 0 else 1
                dst.append([np.longdouble(mp.nstr(sg * w / nrm, 30)) for w in vec])
        return (np.array(Es, np.longdouble).reshape(-1, 9), np.array(Fs, np.longdouble).reshape(-1, 9))


def nearest(model, exact):
    """(distance, index) of the exact solution [m, 9] nearest to model [9]; (inf, -1) when there is none"""
    if len(exact) == 0 or not np.isfinite(np.asarray(model, np.float64)).all():
        return np.inf, -1
    d = [vr.model_distance(model, e) for e in exact]
    k = int(np.argmin(d))
    return d[k], k


# ---------------------------------------------------------------------------------------------
# consensus of a pair over its candidates
# ---------------------------------------------------------------------------------------------
def errors(F, points, dtype=np.float64):
    return vr.errors(F, points, vr.FUNDAMENTAL, dtype)


def consensus(points, K, tol, hypotheses, seed):
    """dict over the candidates in (hypothesis, root) order: hyp, root [C]; E64, F64 [C, 9]; lower,
    upper, exact [C] inlier counts about tol^2 (1 -+ BAND); flagged [C]; best = (candidate index,
    hypothesis, root, count) by the kernel's rule or None; status"""
    points = np.asarray(points, np.float32)
    n = len(points)
    if n < SAMPLE:
        return dict(status=TOO_FEW)
    idx = vr.samples(n, SAMPLE, np.arange(hypotheses), seed)
    E64, F64, valid = solve(points, K, idx, np.float64)
    _Eld, Fld, vld = solve(points, K, idx, np.longdouble)
    hyp, root = np.nonzero(valid)
    if len(hyp) == 0:
        return dict(status=NO_MODEL, idx=idx, best=None)
    F, E = F64[hyp, root], E64[hyp, root]
    err = errors(F, points)
    t2 = np.float64(tol) * np.float64(tol)
    with np.errstate(invalid='ignore'):
        lower = (err <= t2 * (1 - BAND)).sum(1)
        upper = (err <= t2 * (1 + BAND)).sum(1)
        exact = (err <= t2).sum(1)
    dist = np.array([nearest(F[k], Fld[hyp[k]][vld[hyp[k]]])[0] for k in range(len(hyp))])
    flagged = ~(dist <= FLAG)
    best = None
    if exact.max() >= 1:
        k = int(np.argmax(exact))
        best = (k, int(hyp[k]), int(root[k]), int(exact[k]))
    return dict(status=OK if best else NO_MODEL, idx=idx, hyp=hyp, root=root, E64=E, F64=F, lower=lower,
                upper=upper, exact=exact, flagged=flagged, dist=dist, best=best, err=err, tol2=t2)


# ---------------------------------------------------------------------------------------------
# the cases both test files walk
# ---------------------------------------------------------------------------------------------
EDGE_N = (5, 6, 9, 25, 63, 64, 65, 255, 256, 257, 2000, 2049, 4097)


class Case(object):
    def __init__(self, name, points, planted=None, expect=None, hypotheses=256, seed=0, status=OK):
        self.name, self.points = name, np.ascontiguousarray(points, np.float32)
        self.planted, self.expect, self.hypotheses, self.seed, self.status = \
            planted, expect, hypotheses, seed, status
        self.tol, self.K = TOL, KMAT

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for n in EDGE_N:
        pts, planted = vr.scene(n, 0.75 if n >= 25 else 1.0, 25.0, 1000 + n)
        out.append(Case('E-n%d' % n, pts, planted, 'exact' if n >= 25 else None))
    for hyp in (1, 8, 33, 255, 257):                 # 255, 257: either side of the kernel's round of 256
        pts, planted = vr.scene(65, 0.75, 25.0, 77)
        out.append(Case('E-hyp%d' % hyp, pts, planted, None, hypotheses=hyp, status=None))
    for share in (0.6, 0.9):
        pts, planted = vr.scene(120, share, 25.0, 300 + int(share * 10))
        out.append(Case('E-share%.1f' % share, pts, planted, 'exact'))
    out.append(Case('E-duplicates', vr.duplicates(60, 5), status=None))
    out.append(Case('E-collinear', vr.collinear(60, 6), status=None))
    out.append(Case('E-outliers', vr.pure_outliers(60, 7), status=None))
    out.append(Case('E-identical', vr.identical(40), status=NO_MODEL))
    pts, planted = vr.scene(200, 0.75, 0.0, 55)
    out.append(Case('E-flat', pts, planted, 'superset'))
    out.append(Case('E-n4', vr.scene(4, 1.0, 25.0, 4)[0], status=TOO_FEW))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_consensus(name, seed=None):
    c = next(c for c in cases() if c.name == name)
    return consensus(c.points, c.K, c.tol, c.hypotheses, c.seed if seed is None else seed)


OTHER_SEED = vr.OTHER_SEED


def other_seed_cases():
    return [c for c in cases() if c.hypotheses == 256 and 25 <= len(c.points) <= 300]


SOLVER_SCENES = ('E-n64', 'E-n65', 'E-n256')
SOLVER_SAMPLES = 48


@functools.lru_cache(maxsize=None)
def solver_samples():
    """(rays float64 [144, 5, 4], E64 [144, 10, 9], count64 [144]): the first 48 samples of three scenes"""
    out = []
    for name in SOLVER_SCENES:
        c = next(c for c in cases() if c.name == name)
        idx = vr.samples(len(c.points), SAMPLE, np.arange(SOLVER_SAMPLES), c.seed)
        out.append(rays(c.points, c.K)[idx])
    r = np.ascontiguousarray(np.concatenate(out))
    E, count = solve_rays(r)
    return r, E, count


@functools.lru_cache(maxsize=None)
def solver_exact(k):
    """the exact real solutions of solver sample k: E [m, 9] longdouble"""
    return solve_mp(None, np.eye(3), None, rays_in=solver_samples()[0][k])[0]


def residuals(E, r):
    """(epipolar, det, trace) residuals of E [9] (any dtype) on the rays r [5, 4], in longdouble"""
    E = np.asarray(E, np.longdouble).reshape(3, 3)
    r = np.asarray(r, np.longdouble)
    x1 = np.stack([r[:, 0], r[:, 1], np.ones(5, np.longdouble)], axis=1)
    x2 = np.stack([r[:, 2], r[:, 3], np.ones(5, np.longdouble)], axis=1)
    epi = np.abs(((x2 @ E) * x1).sum(1)).max()
    det = abs(E[0, 0] * (E[1, 1] * E[2, 2] - E[1, 2] * E[2, 1]) - E[0, 1] * (E[1, 0] * E[2, 2] - E[1, 2] * E[2, 0])
              + E[0, 2] * (E[1, 0] * E[2, 1] - E[1, 1] * E[2, 0]))
    EEt = E @ E.T
    tr = np.abs(2 * EEt @ E - np.trace(EEt) * E).max()
    return float(epi), float(det), float(tr)


# ---------------------------------------------------------------------------------------------
# a three-image stand-in project over 25 m relief
# ---------------------------------------------------------------------------------------------
def standin_project(pairs_type):
    """vr.standin_project over relief: the same lists and orphans, scenes with 25 m relief"""
    real = vr.scene
    try:
        vr.scene = lambda n, share, relief, seed, row=None: real(n, share, 25.0, seed, row)
        return vr.standin_project(pairs_type)
    finally:
        vr.scene = real


# ---------------------------------------------------------------------------------------------
# where FLOOR_E, FLAG and BAND come from:  python tests/essential_reference.py
# ---------------------------------------------------------------------------------------------
def measure():
    r, E, count = solver_samples()
    d = []
    for k in range(len(r)):
        for e in solver_exact(k):
            d.append(nearest(e, E[k][:count[k]])[0])
    d = np.array(d)
    print('solver samples: %d exact solutions, solve64 median distance %.2e, largest %.2e, beyond 1e-6: %d'
          % (len(d), np.median(d), d.max(), (d > 1e-6).sum()))
    flag = band = 0.0
    for seed in (None, OTHER_SEED):
        for c in (cases() if seed is None else other_seed_cases()):
            ref = case_consensus(c.name, seed)
            if ref['status'] != OK or c.name in UNSTABLE:
                continue
            k = ref['best'][0]
            flag = max(flag, ref['dist'][k])
            e64 = ref['err'][k]
            eld = errors(ref['F64'][k], c.points, np.longdouble)[0]
            t2 = np.longdouble(ref['tol2'])
            near = (eld >= t2 / 4) & (eld <= t2 * 4)
            if near.any():
                band = max(band, float((np.abs(e64 - eld) / eld)[near].max()))
    print('chosen candidates: largest distance float64 - longdouble %.2e; largest relative disagreement '
          'of the error within [tol^2 / 4, 4 tol^2] %.2e' % (flag, band))


if __name__ == '__main__':
    measure()
