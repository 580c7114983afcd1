"""Shared by tests/test_match_verify.py (host) and tests/test_match_verify_gpu.py: the reference of
iamx_verify_pairs (csrc/match_verify.hip) and the seeded inputs of its tests.

* sample() / samples(): the sampling rule of csrc/verify_rule.h restated in Python integers and in
  numpy uint64 (wrapping) arithmetic.
* scene(): two FC6310S frames 100 m up, 30 m apart, 0.3 px noise, over +-25 m of relief or a flat
  field; planted outliers displaced in a random direction by at least 5 tol from the true epipolar
  line.  duplicates(), collinear(), identical(), pure_outliers(): the degenerate inputs.
* solve(): every hypothesis of a pair at once over a dtype (numpy.float64 restates the kernel
  operation by operation; numpy.longdouble is the reference).  solve_scalar(): one hypothesis in
  plain Python over any number type -- mpmath at 60 digits for up to MP_MAX samples per family.
* errors(): the two error measures over a dtype.
* consensus(): all hypotheses in float64, per hypothesis a lower and an upper inlier count
  (err <= tol^2 (1 -+ 1e-9)) and a flag where the float64 model is further than FLOOR from the
  longdouble one.

Needs numpy and mpmath only; every input comes from a seed.
"""
import functools

import numpy as np

W_PX, H_PX = 5472, 3648
FX = 3666.6665
KMAT = np.array([[FX, 0.0, 2736.0], [0.0, FX, 1824.0], [0.0, 0.0, 1.0]])
TOL = max(1.0, W_PX ** 0.25)            # 8.6 px: matcher.filter_by_transform's tolerance
EPS = 2.0 ** -52
FLOOR = 64 * EPS                        # floor of the model tolerance, and the flag's threshold
BAND = 1e-9                             # relative guard band about tol^2
MP_DIGITS = 60
MP_MAX = 64
HOMOGRAPHY, FUNDAMENTAL = 0, 1
SAMPLE = {HOMOGRAPHY: 4, FUNDAMENTAL: 8}
OK, TOO_FEW, NO_MODEL = 0, 1, 2
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
D = 0xD1B54A32D192ED03


# ---------------------------------------------------------------------------------------------
# the sampling rule
# ---------------------------------------------------------------------------------------------
def _mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def sample(n, k, hyp, seed):
    """the k indices hypothesis hyp draws out of n, in draw order (Python integers)"""
    key = _mix((_mix(_mix((seed + G) & M64) ^ n) + hyp * G) & M64)
    taken, out = [], []
    for d in range(k):
        r = _mix((key + (d + 1) * D) & M64)
        j = ((r >> 32) * (n - d)) >> 32
        for t in taken:                  # ascending
            if j >= t:
                j += 1
        out.append(j)
        taken.append(j)
        taken.sort()
    return out


def _mix_np(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return z


def samples(n, k, hyps, seed):
    """sample() for an array of hypothesis indices: int64 [len(hyps), k]"""
    with np.errstate(over='ignore'):
        hyps = np.asarray(hyps, np.uint64)
        k0 = _mix_np(np.array([(seed + G) & M64], np.uint64)) ^ np.uint64(n)
        key = _mix_np(_mix_np(k0) + hyps * np.uint64(G))
        out = np.zeros((len(hyps), k), np.int64)
        taken = np.zeros((len(hyps), 0), np.int64)
        for d in range(k):
            r = _mix_np(key + np.uint64(((d + 1) * D) & M64))
            j = (((r >> np.uint64(32)) * np.uint64(n - d)) >> np.uint64(32)).astype(np.int64)
            for i in range(d):
                j = j + (j >= taken[:, i])
            out[:, d] = j
            taken = np.sort(np.concatenate([taken, j[:, None]], axis=1), axis=1)
    return out


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------
def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


# camera 1 at the origin looking along +z (down), camera 2 30 m along x, slightly turned
R2 = _rot(np.radians(3.0), np.radians(1.0), np.radians(-0.7))
C2 = np.array([30.0, 2.0, 1.0])
_T = R2 @ (-C2)
_TX = np.array([[0, -_T[2], _T[1]], [_T[2], 0, -_T[0]], [-_T[1], _T[0], 0]])
F_TRUE = np.linalg.inv(KMAT).T @ _TX @ R2 @ np.linalg.inv(KMAT)


def _line_distance(x1, x2):
    """distance of x2 [n,2] from the true epipolar line of x1 [n,2], pixels"""
    h1 = np.concatenate([x1, np.ones((len(x1), 1))], axis=1)
    l2 = h1 @ F_TRUE.T
    return np.abs((l2[:, :2] * x2).sum(1) + l2[:, 2]) / np.hypot(l2[:, 0], l2[:, 1])


def scene(n, share, relief, seed, row=None):
    """(points float32 [n, 4], planted bool [n]): round(share n) true matches with 0.3 px noise,
    the rest outliers.  relief: half height of the terrain in metres (0 = a flat field) under the
    100 m flight.  row: every image 1 point exactly on the line y = row + x / 2 (no noise in image 1)."""
    rng = np.random.default_rng(seed)
    x1 = np.zeros((0, 2))
    x2 = np.zeros((0, 2))
    while len(x1) < n:
        m = 2 * n + 16
        p = np.stack([rng.uniform(40, W_PX - 40, m), rng.uniform(40, H_PX - 40, m)], axis=1)
        if row is not None:                      # exactly collinear in float32: even x, y = row + x / 2
            p[:, 0] = 2.0 * np.round(p[:, 0] / 2.0)
            p[:, 1] = row + p[:, 0] / 2.0
        depth = 100.0 + rng.uniform(-relief, relief, m)
        ray = np.concatenate([p, np.ones((m, 1))], axis=1) @ np.linalg.inv(KMAT).T
        X = ray * depth[:, None]
        q = (X - C2) @ R2.T @ KMAT.T
        q = q[:, :2] / q[:, 2:]
        ok = (q[:, 0] > 40) & (q[:, 0] < W_PX - 40) & (q[:, 1] > 40) & (q[:, 1] < H_PX - 40)
        x1, x2 = np.concatenate([x1, p[ok]]), np.concatenate([x2, q[ok]])
    x1, x2 = x1[:n], x2[:n]
    n_in = int(round(share * n))
    planted = np.zeros(n, bool)
    planted[rng.permutation(n)[:n_in]] = True
    noisy1 = x1 + (rng.normal(0, 0.3, (n, 2)) if row is None else 0.0)
    noisy2 = x2 + rng.normal(0, 0.3, (n, 2))
    for i in np.nonzero(~planted)[0]:
        while True:
            ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(5 * TOL, 400.0)
            cand = x2[i] + mag * np.array([np.cos(ang), np.sin(ang)])
            if _line_distance(x1[i:i + 1], cand[None])[0] >= 5 * TOL + 2.0 and \
                    40 < cand[0] < W_PX - 40 and 40 < cand[1] < H_PX - 40:
                noisy2[i] = cand
                break
    return np.concatenate([noisy1, noisy2], axis=1).astype(np.float32), planted


def duplicates(n, seed):
    """half the matches exact copies of the other half (relief, all true matches)"""
    pts, _ = scene((n + 1) // 2, 1.0, 25.0, seed)
    out = np.concatenate([pts, pts])[:n]
    return np.ascontiguousarray(out[np.random.default_rng(seed + 1).permutation(n)])


def collinear(n, seed):
    """all points of image 1 on one line (relief, a quarter outliers)"""
    return scene(n, 0.75, 25.0, seed, row=300.0)[0]


def identical(n):
    return np.tile(np.array([[1000.5, 2000.25, 1100.0, 1900.75]], np.float32), (n, 1))


def pure_outliers(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, W_PX, n), rng.uniform(0, H_PX, n),
                     rng.uniform(0, W_PX, n), rng.uniform(0, H_PX, n)], axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# the solve over a dtype, every hypothesis at once
# ---------------------------------------------------------------------------------------------
def _tree256(v):
    """the kernel's reduction: lane t sums elements t, t+256, ... in order; a xor butterfly over the
    64 lanes of each wave (32, 16, .., 1); then ((w0 + w1) + w2) + w3"""
    n = len(v)
    pad = np.zeros((-n) % 256 + n, v.dtype)
    pad[:n] = v
    rows = pad.reshape(-1, 256)
    acc = np.zeros(256, v.dtype)
    full = n // 256
    for r in range(full):
        acc = acc + rows[r]
    if n % 256:                                   # lanes past the end add nothing (not even a zero)
        acc[:n % 256] = acc[:n % 256] + rows[full][:n % 256]
    acc = acc.reshape(4, 64)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ m]
    return ((acc[0, 0] + acc[1, 0]) + acc[2, 0]) + acc[3, 0]


def normalisation(points, dtype=np.float64):
    """(cx1, cy1, s1, cx2, cy2, s2) or None where an image's points coincide"""
    p = np.asarray(points, np.float32).astype(dtype)
    n = dtype(len(p))
    c = [_tree256(p[:, k]) / n for k in range(4)]
    d1 = np.sqrt((p[:, 0] - c[0]) * (p[:, 0] - c[0]) + (p[:, 1] - c[1]) * (p[:, 1] - c[1]))
    d2 = np.sqrt((p[:, 2] - c[2]) * (p[:, 2] - c[2]) + (p[:, 3] - c[3]) * (p[:, 3] - c[3]))
    md1, md2 = _tree256(d1) / n, _tree256(d2) / n
    if not (md1 > 0 and md2 > 0 and np.isfinite(md1) and np.isfinite(md2)):
        return None
    root2 = dtype(1.4142135623730951) if dtype is np.float64 else np.sqrt(dtype(2))
    return c[0], c[1], root2 / md1, c[2], c[3], root2 / md2


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _mat3(A, B):
    """A [.., 3, 3] times B [.., 3, 3], every entry (a0 b0 + a1 b1) + a2 b2"""
    C = np.zeros(np.broadcast(A, B).shape, np.result_type(A, B))
    for i in range(3):
        for j in range(3):
            C[..., i, j] = _dot3(A[..., i, 0], B[..., 0, j], A[..., i, 1], B[..., 1, j],
                                 A[..., i, 2], B[..., 2, j])
    return C


def _rank2(F):
    A = F.copy()
    V = np.zeros_like(F)
    for i in range(3):
        V[:, i, i] = 1
    one = F.dtype.type(1)
    with np.errstate(all='ignore'):
        for _sweep in range(8):
            for p in range(2):
                for q in range(p + 1, 3):
                    alpha = _dot3(A[:, 0, p], A[:, 0, p], A[:, 1, p], A[:, 1, p], A[:, 2, p], A[:, 2, p])
                    beta = _dot3(A[:, 0, q], A[:, 0, q], A[:, 1, q], A[:, 1, q], A[:, 2, q], A[:, 2, q])
                    gamma = _dot3(A[:, 0, p], A[:, 0, q], A[:, 1, p], A[:, 1, q], A[:, 2, p], A[:, 2, q])
                    zeta = (beta - alpha) / (2 * gamma)
                    t = np.where(zeta >= 0, one, -one) / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
                    c = one / np.sqrt(one + t * t)
                    s = c * t
                    rot = gamma != 0
                    c, s = np.where(rot, c, one), np.where(rot, s, 0 * one)
                    for M in (A, V):
                        mp_, mq = M[:, :, p].copy(), M[:, :, q].copy()
                        M[:, :, p] = c[:, None] * mp_ - s[:, None] * mq
                        M[:, :, q] = s[:, None] * mp_ + c[:, None] * mq
    nrm = np.stack([_dot3(A[:, 0, j], A[:, 0, j], A[:, 1, j], A[:, 1, j], A[:, 2, j], A[:, 2, j])
                    for j in range(3)], axis=1)
    k = np.zeros(len(F), np.int64)
    k[nrm[:, 1] < nrm[:, 0]] = 1
    k[nrm[:, 2] < nrm[np.arange(len(F)), k]] = 2
    A[np.arange(len(F)), :, k] = 0
    out = np.zeros_like(F)
    for i in range(3):
        for j in range(3):
            out[:, i, j] = _dot3(A[:, i, 0], V[:, j, 0], A[:, i, 1], V[:, j, 1], A[:, i, 2], V[:, j, 2])
    return out


def system(points, norm, model, idx, dtype=np.float64):
    """the 8x9 systems of the samples idx [H, k] in normalised coordinates: [H, 8, 9]"""
    p = np.asarray(points, np.float32).astype(dtype)
    cx1, cy1, s1, cx2, cy2, s2 = norm
    H = len(idx)
    A = np.zeros((H, 8, 9), dtype)
    rows = np.repeat(idx, 2, axis=1) if model == HOMOGRAPHY else idx
    s = p[rows]                                               # [H, 8, 4]
    x, y = (s[..., 0] - cx1) * s1, (s[..., 1] - cy1) * s1
    u, v = (s[..., 2] - cx2) * s2, (s[..., 3] - cy2) * s2
    if model == HOMOGRAPHY:
        ev, od = slice(0, 8, 2), slice(1, 8, 2)
        A[:, ev, 0], A[:, ev, 1], A[:, ev, 2] = -x[:, ev], -y[:, ev], -1
        A[:, od, 3], A[:, od, 4], A[:, od, 5] = -x[:, od], -y[:, od], -1
        t = np.where(np.arange(8) % 2 == 1, v, u)
        A[:, :, 6], A[:, :, 7], A[:, :, 8] = t * x, t * y, t
    else:
        A[:, :, 0], A[:, :, 1], A[:, :, 2] = u * x, u * y, u
        A[:, :, 3], A[:, :, 4], A[:, :, 5] = v * x, v * y, v
        A[:, :, 6], A[:, :, 7], A[:, :, 8] = x, y, 1
    return A


def null_vectors(A):
    """Gauss-Jordan over the nine columns in order, the rule of include/iamx.h: [H, 9]"""
    A = A.copy()
    H, dtype = len(A), A.dtype
    ar = np.arange(H)
    thr = np.abs(A).reshape(H, -1).max(1) * dtype.type(2.0 ** -40)
    used = np.zeros((H, 8), bool)
    pivcol = np.full((H, 8), -1)
    pval = np.ones((H, 8), dtype)
    free = np.zeros((H, 9), bool)
    with np.errstate(all='ignore'):
        for c in range(9):
            v = np.where(used, -1, np.abs(A[:, :, c]))
            who = np.argmax(v, axis=1)
            piv = v[ar, who] > thr
            free[:, c] = ~piv
            prow = A[ar, who, :]
            f = A[:, :, c] / prow[:, c][:, None]
            new = A - f[:, :, None] * prow[:, None, :]
            new[:, :, c] = 0
            is_p = np.arange(8)[None, :] == who[:, None]
            A = np.where((piv[:, None] & ~is_p)[:, :, None], new, A)
            mine = piv[:, None] & is_p
            pval = np.where(mine, prow[:, c][:, None], pval)
            pivcol = np.where(mine, c, pivcol)
            used |= mine
        L = 8 - np.argmax(free[:, ::-1], axis=1)
        x = np.zeros((H, 9), dtype)
        x[ar, L] = 1
        for r in range(8):
            val = -A[ar, r, L] / pval[:, r]
            u = used[:, r]
            x[ar[u], pivcol[u, r]] = val[u]
    return x


def finish(x, norm, model):
    """null vectors [H, 9] -> pixel models [H, 9]: rank 2 (fundamental), denormalised, unit
    Frobenius norm, largest-magnitude entry positive"""
    dtype = x.dtype.type
    cx1, cy1, s1, cx2, cy2, s2 = norm
    Mh = x.reshape(-1, 3, 3)
    T1 = np.array([[s1, 0, -(s1 * cx1)], [0, s1, -(s1 * cy1)], [0, 0, 1]], x.dtype)
    with np.errstate(all='ignore'):
        if model == HOMOGRAPHY:
            L = np.array([[dtype(1) / s2, 0, cx2], [0, dtype(1) / s2, cy2], [0, 0, 1]], x.dtype)
        else:
            Mh = _rank2(Mh)
            L = np.array([[s2, 0, 0], [0, s2, 0], [-(s2 * cx2), -(s2 * cy2), 1]], x.dtype)
        M = _mat3(_mat3(L[None], Mh), T1[None]).reshape(-1, 9)
        ss = np.zeros(len(M), x.dtype)
        for j in range(9):
            ss = ss + M[:, j] * M[:, j]
        M = M / np.sqrt(ss)[:, None]
        big = np.argmax(np.abs(M), axis=1)
        sign = np.where(M[np.arange(len(M)), big] < 0, dtype(-1), dtype(1))
        return M * sign[:, None]


def solve(points, model, idx, dtype=np.float64):
    """models [H, 9] of the samples idx [H, k]; None where the normalisation fails"""
    norm = normalisation(points, dtype)
    if norm is None:
        return None
    return finish(null_vectors(system(points, norm, model, idx, dtype)), norm, model)


def errors(M, points, model, dtype=np.float64):
    """the error of every match under every model: [H, n]; a homography's zero or non-finite w
    gives NaN"""
    M = np.asarray(M).astype(dtype).reshape(-1, 9)[:, :, None]
    p = np.asarray(points, np.float32).astype(dtype)
    x1, y1, x2, y2 = (p[None, :, k] for k in range(4))
    with np.errstate(all='ignore'):
        if model == HOMOGRAPHY:
            w = (M[:, 6] * x1 + M[:, 7] * y1) + M[:, 8]
            u = ((M[:, 0] * x1 + M[:, 1] * y1) + M[:, 2]) / w
            v = ((M[:, 3] * x1 + M[:, 4] * y1) + M[:, 5]) / w
            dx, dy = u - x2, v - y2
            err = dx * dx + dy * dy
            return np.where((w != 0) & np.isfinite(w), err, np.nan)
        l2x = (M[:, 0] * x1 + M[:, 1] * y1) + M[:, 2]
        l2y = (M[:, 3] * x1 + M[:, 4] * y1) + M[:, 5]
        l2z = (M[:, 6] * x1 + M[:, 7] * y1) + M[:, 8]
        l1x = (M[:, 0] * x2 + M[:, 3] * y2) + M[:, 6]
        l1y = (M[:, 1] * x2 + M[:, 4] * y2) + M[:, 7]
        e = (x2 * l2x + y2 * l2y) + l2z
        e2 = e * e
        ea, eb = e2 / (l1x * l1x + l1y * l1y), e2 / (l2x * l2x + l2y * l2y)
        return np.where(np.isnan(ea) | np.isnan(eb), np.nan, np.maximum(ea, eb))


def model_distance(a, b):
    """distance of two unit-norm models up to sign (longdouble)"""
    a, b = np.asarray(a, np.longdouble).ravel(), np.asarray(b, np.longdouble).ravel()
    return float(min(np.sqrt(((a - b) ** 2).sum()), np.sqrt(((a + b) ** 2).sum())))


# ---------------------------------------------------------------------------------------------
# one hypothesis over any number type (mpmath)
# ---------------------------------------------------------------------------------------------
def solve_scalar(points, model, idx, num, sqrt):
    """the model of ONE sample idx [k] with every number a num(..) and the rule of the kernel: a
    list of 9, or None.  num = mpmath.mpf and sqrt = mpmath.sqrt (inside a workdps block) is the
    60-digit reference; num = float and sqrt = math.sqrt walks the float64 path."""
    p = [[num(float(v)) for v in row] for row in np.asarray(points, np.float32)]
    n = num(len(p))
    c = [sum((row[k] for row in p), num(0)) / n for k in range(4)]
    md1 = sum((sqrt((r[0] - c[0]) ** 2 + (r[1] - c[1]) ** 2) for r in p), num(0)) / n
    md2 = sum((sqrt((r[2] - c[2]) ** 2 + (r[3] - c[3]) ** 2) for r in p), num(0)) / n
    if not (md1 > 0 and md2 > 0):
        return None
    s1, s2 = sqrt(num(2)) / md1, sqrt(num(2)) / md2
    A = []
    for r in range(8):
        q = p[idx[r // 2 if model == HOMOGRAPHY else r]]
        x, y, u, v = (q[0] - c[0]) * s1, (q[1] - c[1]) * s1, (q[2] - c[2]) * s2, (q[3] - c[3]) * s2
        z, o = num(0), num(1)
        if model == HOMOGRAPHY:
            A.append([-x, -y, -o, z, z, z, u * x, u * y, u] if r % 2 == 0 else
                     [z, z, z, -x, -y, -o, v * x, v * y, v])
        else:
            A.append([u * x, u * y, u, v * x, v * y, v, x, y, o])
    thr = max(abs(a) for row in A for a in row) * num(2.0 ** -40)
    used, pivcol, free = [False] * 8, [-1] * 8, []
    for cidx in range(9):
        best, who = num(-1), -1
        for r in range(8):
            if not used[r] and abs(A[r][cidx]) > best:
                best, who = abs(A[r][cidx]), r
        if who < 0 or not best > thr:
            free.append(cidx)
            continue
        used[who], pivcol[who] = True, cidx
        for r in range(8):
            if r != who:
                f = A[r][cidx] / A[who][cidx]
                A[r] = [num(0) if j == cidx else A[r][j] - f * A[who][j] for j in range(9)]
    L = free[-1]
    xv = [num(0)] * 9
    xv[L] = num(1)
    for r in range(8):
        if used[r]:
            xv[pivcol[r]] = -A[r][L] / A[r][pivcol[r]]
    Mh = [xv[0:3], xv[3:6], xv[6:9]]
    mul = lambda P, Q: [[sum((P[i][k] * Q[k][j] for k in range(3)), num(0)) for j in range(3)] for i in range(3)]
    T1 = [[s1, num(0), -s1 * c[0]], [num(0), s1, -s1 * c[1]], [num(0), num(0), num(1)]]
    if model == HOMOGRAPHY:
        Lm = [[1 / s2, num(0), c[2]], [num(0), 1 / s2, c[3]], [num(0), num(0), num(1)]]
    else:
        V = [[num(int(i == j)) for j in range(3)] for i in range(3)]
        for _sweep in range(8):
            for pp in range(2):
                for qq in range(pp + 1, 3):
                    al = sum((Mh[i][pp] ** 2 for i in range(3)), num(0))
                    be = sum((Mh[i][qq] ** 2 for i in range(3)), num(0))
                    ga = sum((Mh[i][pp] * Mh[i][qq] for i in range(3)), num(0))
                    if ga == 0:
                        continue
                    zeta = (be - al) / (2 * ga)
                    t = (1 if zeta >= 0 else -1) / (abs(zeta) + sqrt(1 + zeta * zeta))
                    cs = 1 / sqrt(1 + t * t)
                    sn = cs * t
                    for Mx in (Mh, V):
                        for i in range(3):
                            a_, b_ = Mx[i][pp], Mx[i][qq]
                            Mx[i][pp], Mx[i][qq] = cs * a_ - sn * b_, sn * a_ + cs * b_
        nrm = [sum((Mh[i][j] ** 2 for i in range(3)), num(0)) for j in range(3)]
        k = 0
        if nrm[1] < nrm[k]:
            k = 1
        if nrm[2] < nrm[k]:
            k = 2
        for i in range(3):
            Mh[i][k] = num(0)
        Mh = [[sum((Mh[i][m] * V[j][m] for m in range(3)), num(0)) for j in range(3)] for i in range(3)]
        Lm = [[s2, num(0), num(0)], [num(0), s2, num(0)], [-s2 * c[2], -s2 * c[3], num(1)]]
    M = [v for row in mul(mul(Lm, Mh), T1) for v in row]
    fro = sqrt(sum((v * v for v in M), num(0)))
    if not fro > 0:
        return None
    M = [v / fro for v in M]
    big = max(range(9), key=lambda j: (abs(M[j]), -j))
    return [-v for v in M] if M[big] < 0 else M


def solve_mp(points, model, idx):
    """solve_scalar at MP_DIGITS digits, rounded to longdouble [9]"""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        M = solve_scalar(points, model, list(idx), mp.mpf, mp.sqrt)
        if M is None:
            return None
        return np.array([np.longdouble(mp.nstr(v, 30)) for v in M], np.longdouble)


# ---------------------------------------------------------------------------------------------
# consensus of a pair
# ---------------------------------------------------------------------------------------------
def consensus(points, tol, model, hypotheses, seed):
    """dict: status; idx [H, k]; models64, modelsld [H, 9]; lower, upper [H] inlier counts with
    err <= tol^2 (1 -+ BAND) under the float64 model in float64; flagged [H]: the float64 model is
    not finite, or further than FLOOR from the longdouble one; best = (hypothesis, lower count) of
    the hypothesis the rule picks from the float64 counts (None: no model); stable: float64 and
    longdouble agree on the best model's mask outside the guard band."""
    points = np.asarray(points, np.float32)
    n, k = len(points), SAMPLE[model]
    if n < k:
        return dict(status=TOO_FEW)
    idx = samples(n, k, np.arange(hypotheses), seed)
    m64 = solve(points, model, idx, np.float64)
    if m64 is None:
        return dict(status=NO_MODEL)
    mld = solve(points, model, idx, np.longdouble)
    finite = np.isfinite(m64).all(1)
    err = errors(m64, points, model)
    t2 = np.float64(tol) * np.float64(tol)
    with np.errstate(invalid='ignore'):
        lower = np.where(finite, (err <= t2 * (1 - BAND)).sum(1), 0)
        upper = np.where(finite, (err <= t2 * (1 + BAND)).sum(1), 0)
        exact = np.where(finite, (err <= t2).sum(1), 0)
    dist = np.array([model_distance(a, b) if f and np.isfinite(b).all() else np.inf
                     for a, b, f in zip(m64, mld, finite)])
    flagged = ~(dist <= FLOOR)
    best = None
    if exact.max() >= 1:
        h = int(np.argmax(exact))                    # first of the largest: ties to the lowest h
        best = (h, int(exact[h]))
    stable = True
    if best:
        # is the error measure itself well conditioned under the chosen model?  (a model whose
        # epipolar lines are rounding noise gives errors that float64 and longdouble disagree on)
        eld = errors(m64[best[0]], points, model, np.longdouble)[0]
        tld = np.longdouble(tol) * np.longdouble(tol)
        with np.errstate(invalid='ignore'):
            inside = (eld > tld * (1 - BAND)) & (eld <= tld * (1 + BAND))
            stable = bool(((eld <= tld) == (err[best[0]] <= t2))[~inside].all())
    return dict(status=OK if best else NO_MODEL, stable=stable, idx=idx, models64=m64, modelsld=mld, lower=lower,
                upper=upper, exact=exact, flagged=flagged, dist=dist, best=best, err=err, tol2=t2)


# ---------------------------------------------------------------------------------------------
# the cases both test files walk
# ---------------------------------------------------------------------------------------------
# Cases whose chosen model makes the error measure itself ill conditioned: with every image 1 point on
# one line the fundamental samples are rank deficient, and the null vector the rule picks has epipolar
# lines in image 2 whose direction is rounding noise (|l2x|, |l2y| ~ 1e-17 of |l2z|).  float64 and
# longdouble then disagree on e^2 / (l2x^2 + l2y^2) for most matches; the mask is checked against the
# float64 expression there (tests/test_match_verify.py pins the list).
UNSTABLE = ('F-collinear',)
EDGE_N = (4, 5, 8, 9, 25, 63, 64, 65, 255, 256, 257, 2000, 2049, 4097)


class Case(object):
    def __init__(self, name, model, points, planted=None, expect=None, hypotheses=256, seed=0,
                 status=OK):
        self.name, self.model, self.points = name, model, np.ascontiguousarray(points, np.float32)
        self.planted, self.expect, self.hypotheses, self.seed, self.status = \
            planted, expect, hypotheses, seed, status
        self.tol = TOL

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for model, tag, relief in ((HOMOGRAPHY, 'H', 0.0), (FUNDAMENTAL, 'F', 25.0)):
        for n in EDGE_N:
            if n < SAMPLE[model]:
                continue
            share = 0.75 if n >= 25 else 1.0
            pts, planted = scene(n, share, relief, 1000 + n)
            out.append(Case('%s-n%d' % (tag, n), model, pts, planted, 'exact' if n >= 25 else None))
        for hyp in (1, 8, 33):
            pts, planted = scene(65, 0.75, relief, 77)
            out.append(Case('%s-hyp%d' % (tag, hyp), model, pts, planted, None, hypotheses=hyp))
        for share in (0.6, 0.9):
            pts, planted = scene(120, share, relief, 300 + int(share * 10))
            out.append(Case('%s-share%.1f' % (tag, share), model, pts, planted, 'exact'))
        out.append(Case('%s-duplicates' % tag, model, duplicates(60, 5), status=None))
        out.append(Case('%s-collinear' % tag, model, collinear(60, 6), status=None))
        out.append(Case('%s-outliers' % tag, model, pure_outliers(60, 7), status=None))
        out.append(Case('%s-identical' % tag, model, identical(40), status=NO_MODEL))
    pts, planted = scene(200, 0.75, 0.0, 55)
    out.append(Case('F-flat', FUNDAMENTAL, pts, planted, 'superset'))
    out.append(Case('H-n3', HOMOGRAPHY, scene(3, 1.0, 0.0, 3)[0], status=TOO_FEW))
    out.append(Case('F-n7', FUNDAMENTAL, scene(7, 1.0, 25.0, 7)[0], status=TOO_FEW))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_consensus(name, seed=None):
    c = next(c for c in cases() if c.name == name)
    return consensus(c.points, c.tol, c.model, c.hypotheses, c.seed if seed is None else seed)


# ---------------------------------------------------------------------------------------------
# a three-image stand-in project with planted wrong matches
# ---------------------------------------------------------------------------------------------
class StandInImage(object):
    def __init__(self, name, uv):
        self.name, self.width, self.height = name, W_PX, H_PX
        self.uv_list = np.ascontiguousarray(uv, np.float32)
        self.kp_list = list(range(len(uv)))
        self.match_list = {}
        self.matches_clean = True


class StandInProject(object):
    def __init__(self, images):
        self.image_list = images


def standin_project(pairs_type):
    """(project, truth): images a, b, c; flat-field scenes for (a, b), (a, c), (b, c) with a quarter
    planted outliers; keypoints of every image in a seeded random order.  Forward lists: (a, b) and
    (b, c) of pairs_type (the package's MatchPairs), (a, c) a plain list.  Reverse lists: (b, a) a
    plain list in another order with two orphans added, (c, a) missing, (c, b) of pairs_type in
    another order.  truth[(x, y)] = dict(points, forward, planted, reverse, orphans)."""
    rng = np.random.default_rng(2024)
    names = ['a', 'b', 'c']
    scenes = {(0, 1): scene(100, 0.75, 0.0, 801), (0, 2): scene(110, 0.75, 0.0, 802),
              (1, 2): scene(120, 0.75, 0.0, 803)}
    kp = {k: [] for k in range(3)}
    where = {}
    for (x, y), (pts, _planted) in scenes.items():
        where[(x, y)] = (len(kp[x]), len(kp[y]))
        kp[x].extend(pts[:, :2].tolist())
        kp[y].extend(pts[:, 2:].tolist())
    perm = {k: rng.permutation(len(kp[k])) for k in range(3)}         # new position of old index
    images = []
    for k in range(3):
        uv = np.zeros((len(kp[k]), 2), np.float32)
        uv[perm[k]] = np.asarray(kp[k], np.float32)
        images.append(StandInImage(names[k], uv))
    truth = {}
    for (x, y), (pts, planted) in scenes.items():
        ox, oy = where[(x, y)]
        n = len(pts)
        fwd = np.stack([perm[x][ox + np.arange(n)], perm[y][oy + np.arange(n)]], axis=1).astype(np.int32)
        order = rng.permutation(n)
        fwd, planted, pts = fwd[order], planted[order], pts[order]
        rev_order = rng.permutation(n)
        rev = fwd[rev_order][:, ::-1]
        rev_planted = planted[rev_order]
        truth[(x, y)] = dict(points=pts, forward=fwd, planted=planted, reverse=rev,
                             reverse_kept=rev[rev_planted], orphans=0)
    a, b, c = images
    a.match_list['b'] = pairs_type(truth[(0, 1)]['forward'].copy())
    a.match_list['c'] = truth[(0, 2)]['forward'].tolist()
    b.match_list['c'] = pairs_type(truth[(1, 2)]['forward'].copy())
    orphan = [[int(truth[(0, 1)]['forward'][0, 1]), int(truth[(0, 1)]['forward'][1, 0])],
              [int(truth[(0, 1)]['forward'][2, 1]), int(truth[(0, 1)]['forward'][3, 0])]]
    rv = truth[(0, 1)]['reverse'].tolist()
    b.match_list['a'] = rv[:5] + [orphan[0]] + rv[5:] + [orphan[1]]
    truth[(0, 1)]['orphans'] = 2
    c.match_list['b'] = pairs_type(np.ascontiguousarray(truth[(1, 2)]['reverse']))
    return StandInProject(images), truth


OTHER_SEED = (1 << 63) + 5


def other_seed_cases(model=None):
    """the cases that are run again under OTHER_SEED: 256 hypotheses, 25 <= n <= 300"""
    return [c for c in cases() if c.hypotheses == 256 and 25 <= len(c.points) <= 300
            and (model is None or c.model == model)]
