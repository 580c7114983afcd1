"""Shared by tests/test_pair_geometry.py (host) and tests/test_pair_geometry_gpu.py: high-precision
references for the four kernels of csrc/triangulate.hip, and the seeded generators of their inputs.

* mp_null_vector(): the 4x4 DLT system solved with mpmath at 60 digits -- the yardstick for
  iamx_triangulate_pairs / _pairs_xyz / _packed (one-sided Jacobi, f64) and for numpy's SVD in
  oracle/smart_oracle.triangulate_down.
* similarity_trace(): oracle/smart_oracle.fit_similarity restated over a dtype (numpy.longdouble
  = the reference; numpy.float64 = the oracle itself, with its inlier sets exposed): the same
  threshold schedule, the same break rules, and per iteration the inlier set and the smallest
  |residual - threshold|.
* ground_ordered(): iamx_triangulate_ground in numpy float64 scalars, operation by operation in
  the kernel's order (products and sums rounded separately, sky rays in the divisor).

Needs numpy, mpmath and the repository's oracle/ package only; every input comes from a seed.
"""
import numpy as np

from oracle.smart_oracle import SIMILARITY_THRESHOLDS

# the camera of tests/golden/find_matches_strip.pkl (oracle/gen_golden.py K_FC6310S)
W_PX, H_PX = 5472, 3648
FX = 3666.6665
K = np.array([[FX, 0.0, 2736.0], [0.0, FX, 1824.0], [0.0, 0.0, 1.0]])
IK = np.linalg.inv(K)
EPS = 2.0 ** -52
MP_DIGITS = 60
MP_MAX = 64                      # matches per family that go through mpmath
SIM_NOISE = 0.3                  # px, similarity cases
# px, triangulation cases.  At 0.3 px the nominal flight (30 m baseline at 100 m) has sigma3/sigma4
# = 179 and at 0.03 px 1.5e3, less at a higher altitude: the rays miss each other by so much that the null direction is not the well-defined
# one the comparison needs (>= 1e3).  The short baseline (1.8 px of parallax) gets no noise at
# all: rounding the keypoints to float32 (2e-4 px) already leaves sigma4 != 0.
PIXEL_NOISE = 0.01
POISON_FILL = 777.0              # what the outputs are pre-filled with


# ---------------------------------------------------------------------------------------------
# two-view DLT
# ---------------------------------------------------------------------------------------------
def dlt_matrix(P1, P2, uv1, uv2):
    """[x1 P1_3 - P1_1; y1 P1_3 - P1_2; x2 P2_3 - P2_1; y2 P2_3 - P2_2] of one match in float64,
    formed as the kernel and oracle/smart_oracle.triangulate_down form it (keypoints widened from
    float32, IK . [u, v, 1] left to right)."""
    A = np.zeros((4, 4))
    for j, (P, uv) in enumerate(((P1, uv1), (P2, uv2))):
        P = np.asarray(P, np.float64).reshape(3, 4)
        u, v = np.float64(uv[0]), np.float64(uv[1])
        x = IK[0, 0] * u + IK[0, 1] * v + IK[0, 2]
        y = IK[1, 0] * u + IK[1, 1] * v + IK[1, 2]
        A[2 * j] = x * P[2] - P[0]
        A[2 * j + 1] = y * P[2] - P[1]
    return A


def mp_null_vector(A):
    """(X, sigma3, sigma4) of the float64 matrix A at MP_DIGITS digits: X the right singular vector
    of the smallest singular value (an mpmath column, unit length), sigma3 >= sigma4 the two
    smallest singular values."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        M = mp.matrix([[mp.mpf(float(a)) for a in row] for row in A])
        _U, S, V = mp.svd_r(M)
        order = sorted(range(4), key=lambda i: S[i])
        X = V[order[0], :].T
        X = X / mp.norm(X)
        return X, S[order[1]], S[order[0]]


def mp_residual_ratio(A, xhat, sigma4):
    """criterion (a): ||A xhat|| / ||xhat|| / sigma4 for a float64 solution xhat = (x, y, z, 1),
    evaluated at MP_DIGITS digits (1 for the exact null direction, never below it)."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        M = mp.matrix([[mp.mpf(float(a)) for a in row] for row in A])
        x = mp.matrix([mp.mpf(float(a)) for a in xhat])
        return mp.norm(M * x) / mp.norm(x) / sigma4


def dlt_svd_xyz(P1, P2, uv1, uv2):
    """oracle/smart_oracle.triangulate_down with all three coordinates: float64 [n, 3]
    (numpy's SVD; column 2 is triangulate_down's result bit for bit)"""
    out = np.zeros((len(uv1), 3))
    for i in range(len(uv1)):
        X = np.linalg.svd(dlt_matrix(P1, P2, uv1[i], uv2[i]))[2][3]
        out[i] = X[:3] / X[3]
    return out


def coord_bound(sig3, sig4, xyz_ref):
    """criterion (b)'s floor 64 eps . sigma3/sigma4 . scale for each of x, y, z.  A unit null
    vector X turned by a small angle theta moves x_k = X_k / X_3 by at most theta (1 + |x_k|) / |X_3|
    to first order, and 1 / |X_3| = ||(x, y, z, 1)||: that product is the scale."""
    x = np.asarray(xyz_ref, np.float64)
    scale = np.sqrt(1.0 + (x * x).sum()) * (1.0 + np.abs(x))
    return 64 * EPS * float(sig3 / sig4) * scale


def z_bound(sig3, sig4, xyz_ref):
    return coord_bound(sig3, sig4, xyz_ref)[2]


def svd_bounds(P1, P2, uv1, uv2):
    """for matches beyond the mpmath budget: (xyz [n, 3], bound [n, 3], sigma3/sigma4 [n],
    |X_3| [n]) from numpy's SVD -- coord_bound() with float64 singular values"""
    n = len(uv1)
    xyz, bound, cond, w = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    for i in range(n):
        _u, s, vt = np.linalg.svd(dlt_matrix(P1, P2, uv1[i], uv2[i]))
        xyz[i] = vt[3][:3] / vt[3][3]
        cond[i], w[i] = s[2] / s[3], abs(vt[3][3])
        bound[i] = coord_bound(s[2], s[3], xyz[i])
    return xyz, bound, cond, w


# ---------------------------------------------------------------------------------------------
# similarity
# ---------------------------------------------------------------------------------------------
def _fit(P, Q, w):
    n = w.sum()
    if n < 2:
        return None
    cp = (P * w[:, None]).sum(0) / n
    cq = (Q * w[:, None]).sum(0) / n
    Pc, Qc = P - cp, Q - cq
    den = (w * (Pc * Pc).sum(1)).sum()
    if den == 0:
        return None
    a = (w * (Pc * Qc).sum(1)).sum() / den
    b = (w * (Pc[:, 0] * Qc[:, 1] - Pc[:, 1] * Qc[:, 0])).sum() / den
    A = np.array([[a, -b], [b, a]], dtype=P.dtype)
    return np.hstack([A, (cq - A.dot(cp)).reshape(2, 1)])


def similarity_trace(from_pts, to_pts, dtype=np.longdouble):
    """fit_similarity in `dtype`.  Returns (M or None, trace); trace[k - 1] describes re-fit k
    (1..9) as a dict: inliers (bool [n]), margin (smallest |residual - threshold|), fitted (False
    where the re-fit found fewer than two inliers or a zero denominator and the loop stopped)."""
    P = np.asarray(from_pts, np.float32).astype(dtype).reshape(-1, 2)
    Q = np.asarray(to_pts, np.float32).astype(dtype).reshape(-1, 2)
    trace = []
    M = _fit(P, Q, np.ones(len(P), dtype)) if len(P) else None
    if M is None:
        return None, trace
    for thr in SIMILARITY_THRESHOLDS:
        res = np.sqrt((((P.dot(M[:, :2].T) + M[:, 2]) - Q) ** 2).sum(1))
        inl = res <= thr
        new = _fit(P, Q, inl.astype(dtype))
        trace.append(dict(inliers=inl, margin=float(np.abs(res - dtype(thr)).min()),
                          fitted=new is not None))
        if new is None:
            break
        M = new
    return M, trace


def similarity_error(M, M_ref, coord_scale):
    """largest entry of |M - M_ref|, the four rotation/scale entries as they are and the two
    translations divided by the largest coordinate of the case"""
    d = np.abs(np.asarray(M, np.longdouble).reshape(2, 3) - np.asarray(M_ref, np.longdouble).reshape(2, 3))
    d[:, 2] /= coord_scale
    return float(d.max())


SIM_FLOOR = 64 * EPS             # five compounded tree sums of <= 4096 terms, ~12 ulp each


def two_point_similarity(p0, p1, q0, q1):
    """the similarity that maps p0 -> q0 and p1 -> q1 (complex division), 2x3 longdouble"""
    p0, p1, q0, q1 = (np.asarray(v, np.float32).astype(np.longdouble) for v in (p0, p1, q0, q1))
    dp, dq = p1 - p0, q1 - q0
    den = dp[0] * dp[0] + dp[1] * dp[1]
    a = (dp[0] * dq[0] + dp[1] * dq[1]) / den
    b = (dp[0] * dq[1] - dp[1] * dq[0]) / den
    return np.array([[a, -b, q0[0] - (a * p0[0] - b * p0[1])],
                     [b, a, q0[1] - (b * p0[0] + a * p0[1])]], dtype=np.longdouble)


SIM_SIZES = (2, 3, 64, 255, 256, 257, 1000, 4096)
SIM_OUTLIERS = (6.0, 30.0, 120.0, 900.0)


def similarity_case(n, seed=1):
    """(a_pts, b_pts) float32 [n, 2]: image b's points uniform over the frame, image a's the same
    under a similarity (a few degrees, a few percent, some hundred px) plus SIM_NOISE, 30 % of
    them pushed away by 6 / 30 / 120 / 900 px in turn (graded outliers, one grade per threshold)"""
    rng = np.random.default_rng([seed, n])
    b = rng.uniform([0, 0], [W_PX, H_PX], (n, 2))
    ang, s = np.deg2rad(rng.uniform(-8, 8)), rng.uniform(0.95, 1.05)
    R = s * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    a = b.dot(R.T) + rng.uniform(-400, 400, 2) + rng.normal(0, SIM_NOISE, (n, 2))
    out = np.nonzero(rng.random(n) < 0.3)[0]
    for j, i in enumerate(out):
        th = rng.uniform(0, 2 * np.pi)
        a[i] += SIM_OUTLIERS[j % 4] * np.array([np.cos(th), np.sin(th)])
    return a.astype(np.float32), b.astype(np.float32)


def dry_case():
    """five hand-built matches whose re-fits run out of inliers: a, b float32 [5, 2].  Four points
    of b on a 1000 px square map onto a with errors of 17 px in a pattern no similarity absorbs
    (zero mean, zero moment against the corners and against the corners turned by 90 degrees), the
    fifth, at the centre, lies 117 px off.  The schedule keeps all five at 200 px, loses the
    fifth at 50 px, and at 10 px every remaining one: re-fit 3 has no inliers."""
    b = np.array([[1000, 1000], [2000, 1000], [2000, 2000], [1000, 2000], [1500, 1500]], np.float64)
    a = b + 100.0
    a[0] += [24, 0]
    a[1] += [0, 24]
    a[2] += [24, 0]
    a[3] += [0, 24]
    a[4] += [100, -60]
    return a.astype(np.float32), b.astype(np.float32)


# ---------------------------------------------------------------------------------------------
# ground intersection
# ---------------------------------------------------------------------------------------------
def ground_ordered(M, ned, base, obs_img, obs_uv, feat_ptr):
    """(out [n_feat, 3] float64, n_sky): every operation one correctly rounded float64 operation
    in the order csrc/triangulate.hip spells out"""
    f8 = np.float64
    n = len(feat_ptr) - 1
    out = np.zeros((n, 3))
    n_sky = 0
    for f in range(n):
        s0 = s1 = s2 = f8(0.0)
        b, e = int(feat_ptr[f]), int(feat_ptr[f + 1])
        for o in range(b, e):
            im = int(obs_img[o])
            m = [f8(x) for x in M[im]]
            c = [f8(x) for x in ned[im]]
            u, v = f8(obs_uv[o][0]), f8(obs_uv[o][1])
            p0 = (m[0] * u + m[1] * v) + m[2]
            p1 = (m[3] * u + m[4] * v) + m[5]
            p2 = (m[6] * u + m[7] * v) + m[8]
            nrm = np.sqrt((p0 * p0 + p1 * p1) + p2 * p2)
            v0, v1, v2 = p0 / nrm, p1 / nrm, p2 / nrm
            if v2 > 0.0:
                d = -(c[2] + f8(base[im]))
                factor = d / v2
                s0 = s0 + (c[0] + v0 * factor)
                s1 = s1 + (c[1] + v1 * factor)
                s2 = s2 + (c[2] + d)
            else:
                n_sky += 1
        cnt = f8(e - b)
        out[f] = [s0 / cnt, s1 / cnt, s2 / cnt]
    return out, n_sky


# ---------------------------------------------------------------------------------------------
# cameras and scenes
# ---------------------------------------------------------------------------------------------
def _rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


# camera axes (x right, y down the image, z forward) of a camera that looks straight down with
# the top of the image to the north, as rows in NED
_NADIR = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def ned2cam(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0):
    """rotation NED -> camera: nadir, turned by yaw about down, its forward axis lifted by pitch
    towards the top of the image (90 = level), rolled about forward"""
    return (_rot(2, np.deg2rad(roll_deg)).dot(_rot(0, -np.deg2rad(pitch_deg))).dot(_NADIR)
            .dot(_rot(2, np.deg2rad(yaw_deg)).T))


def projection(R, ned):
    """[R | t] with t = -R . ned, 3x4"""
    R = np.asarray(R, np.float64)
    return np.hstack([R, -R.dot(np.asarray(ned, np.float64).reshape(3, 1))])


def project_points(R, ned, X):
    """pixels of the NED points X [n, 3], float64 (no noise, no rounding)"""
    c = (X - np.asarray(ned, np.float64)).dot(np.asarray(R).T)
    x = c[:, :2] / c[:, 2:3]
    return x * FX + K[:2, 2]


def ground_points(rng, n, R1, ned1, R2, ned2, relief=5.0):
    """n NED points near the ground plane z = 0 (+- relief) that both cameras see inside the frame"""
    pts = np.zeros((0, 3))
    centre = (np.asarray(ned1, float) + np.asarray(ned2, float)) / 2
    # where the mean optical axis meets the ground
    axis = (np.asarray(R1)[2] + np.asarray(R2)[2]) / 2
    centre = centre + axis * (-centre[2] / axis[2])
    while len(pts) < n:
        X = centre + np.concatenate([rng.uniform(-90, 90, (4 * n + 16, 2)),
                                     rng.uniform(-relief, relief, (4 * n + 16, 1))], 1)
        ok = np.ones(len(X), bool)
        for R, ned in ((R1, ned1), (R2, ned2)):
            uv = project_points(R, ned, X)
            ok &= ((X - ned).dot(np.asarray(R)[2]) > 1) & (uv[:, 0] > 20) & (uv[:, 0] < W_PX - 20) \
                & (uv[:, 1] > 20) & (uv[:, 1] < H_PX - 20)
        pts = np.concatenate([pts, X[ok]])
    return pts[:n]


def observe(rng, R, ned, X, noise=PIXEL_NOISE):
    """float32 keypoints of X in the camera, with pixel noise"""
    return (project_points(R, ned, X) + rng.normal(0, noise, (len(X), 2))).astype(np.float32)


# geometry families of the accuracy test: name -> (baseline m, pitch deg, |NED| offset m, asserted)
FAMILIES = {
    'nominal': (30.0, 0.0, 0.0, True),
    'far_1e3': (30.0, 0.0, 1e3, True),
    'far_1e4': (30.0, 0.0, 1e4, True),
    'short_baseline': (0.05, 0.0, 0.0, True),
    'oblique': (30.0, 30.0, 0.0, True),
    'far_1e5': (30.0, 0.0, 1e5, False),
    'far_1e6': (30.0, 0.0, 1e6, False),
}
_OFFSET_DIR = np.array([0.8, -0.6, 0.02])


def family_case(name, n=MP_MAX, seed=7):
    """dict(P1, P2 [3, 4], uv1, uv2 float32 [n, 2]) of one family: two cameras 100 m above the
    ground, `baseline` apart along the track; the far-origin families are the nominal scene and
    its very keypoints with every NED position moved by offset . (0.8, -0.6, 0.02)"""
    baseline, pitch, offset, _ = FAMILIES[name]
    rng = np.random.default_rng([seed, int(baseline * 100), int(pitch)])
    R1 = ned2cam(12.0, pitch + 1.5, -2.0)
    R2 = ned2cam(15.0, pitch - 1.0, 1.0)
    ned1 = np.array([3.0, -2.0, -100.0])
    ned2 = ned1 + baseline * np.array([0.97, 0.2, 0.03])
    X = ground_points(rng, n, R1, ned1, R2, ned2)
    noise = PIXEL_NOISE if baseline > 1 else 0.0
    uv1, uv2 = observe(rng, R1, ned1, X, noise), observe(rng, R2, ned2, X, noise)
    move = offset * _OFFSET_DIR
    return dict(P1=projection(R1, ned1 + move), P2=projection(R2, ned2 + move), uv1=uv1, uv2=uv2)


_family_refs = {}


def family_reference(name):
    """the family's case with its mpmath reference, computed once and shared (callers do not
    modify it): A [n, 4, 4], xyz_ref [n, 3] float64 (rounded from mpmath), sig3, sig4 (mpmath),
    and numpy's SVD on the same matrices: svd_xyz [n, 3], svd_ratio_m1 [n] (criterion (a) - 1)"""
    import mpmath as mp
    if name not in _family_refs:
        c = family_case(name)
        n = len(c['uv1'])
        A = np.stack([dlt_matrix(c['P1'], c['P2'], c['uv1'][i], c['uv2'][i]) for i in range(n)])
        xyz, s3, s4, w = np.zeros((n, 3)), [], [], np.zeros(n)
        for i in range(n):
            X, a, b = mp_null_vector(A[i])
            with mp.workdps(MP_DIGITS):
                xyz[i] = [float(X[k] / X[3]) for k in range(3)]
                w[i] = float(abs(X[3]))
            s3.append(a)
            s4.append(b)
        svd = dlt_svd_xyz(c['P1'], c['P2'], c['uv1'], c['uv2'])
        ratio = np.array([float(mp_residual_ratio(A[i], list(svd[i]) + [1.0], s4[i]) - 1) for i in range(n)])
        _family_refs[name] = dict(c, A=A, xyz_ref=xyz, w_ref=w, sig3=s3, sig4=s4, svd_xyz=svd,
                                  svd_ratio_m1=ratio)
    return _family_refs[name]


# ---------------------------------------------------------------------------------------------
# the launches of the GPU tests, as host arrays
# ---------------------------------------------------------------------------------------------
class Arena(object):
    """keypoints of several images in one float32 array with an int64 prefix table, and ONE
    poison keypoint (NaN, NaN) behind the last image -- inside the array, so an index that reaches
    it reads memory the launch owns.  Unused rows of a match table point at it."""

    def __init__(self, n_images):
        self.kp = [np.zeros((0, 2), np.float32) for _ in range(n_images)]

    def add(self, image, uv):
        """append keypoints to an image; returns their indices"""
        first = len(self.kp[image])
        self.kp[image] = np.concatenate([self.kp[image], np.asarray(uv, np.float32)])
        return np.arange(first, first + len(uv), dtype=np.int32)

    def shuffle(self, rng):
        """permute every image's keypoints; returns per image the map old index -> new index"""
        maps = []
        for i, kp in enumerate(self.kp):
            perm = rng.permutation(len(kp))
            self.kp[i] = kp[perm]
            inv = np.empty(len(kp), np.int32)
            inv[perm] = np.arange(len(kp), dtype=np.int32)
            maps.append(inv)
        return maps

    def finish(self):
        sizes = np.array([len(k) for k in self.kp], np.int64)
        self.kp_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        # behind the poison a margin of finite keypoints as long as the largest image: a kernel
        # that looks a row up under the wrong image still reads memory the launch owns
        margin = np.full((int(sizes.max()) if len(sizes) else 0, 2), 12345.0, np.float32)
        self.xy = np.concatenate(self.kp + [np.full((1, 2), np.nan, np.float32), margin])
        self.poison_row = int(self.kp_off[-1])
        return self

    def poison(self, image):
        """the poison keypoint's index as image `image` addresses it"""
        return np.int32(self.kp_off[-1] - self.kp_off[image])


def match_table(arena, pair_img, rows, clip):
    """int32 [n_pairs, clip, 2]: rows[p] first, the poison keypoint in every row past them"""
    t = np.zeros((len(pair_img), clip, 2), np.int32)
    for p, (a, b) in enumerate(pair_img):
        t[p, :, 0], t[p, :, 1] = arena.poison(a), arena.poison(b)
        t[p, :len(rows[p])] = rows[p]
    return t


LAUNCH_PAIRS = ((4, 1), (1, 4), (0, 4), (5, 2), (4, 3))   # slot 4 in four pairs, (4, 1) and (1, 4)
LAUNCH_COUNTS = (0, 1, 256, 257, 300)
LAUNCH_CLIP = 300


def launch_case(seed=11):
    """the launch-geometry case: six cameras along a track, different keypoint counts, the match
    rows of LAUNCH_PAIRS with LAUNCH_COUNTS matches.  dict(arena, PROJ [6, 12], pair_img [5, 2],
    m_cnt [5], m_pairs [5, clip, 2], rows)"""
    rng = np.random.default_rng(seed)
    R = [ned2cam(10.0 + 3 * i, rng.uniform(-3, 3), rng.uniform(-3, 3)) for i in range(6)]
    ned = [np.array([20.0 * i, 2.0 * (-1) ** i, -100.0 - 4 * i]) for i in range(6)]
    arena = Arena(6)
    arena.add(3, rng.uniform(0, 3000, (17, 2)))          # keypoints no match uses
    arena.add(5, rng.uniform(0, 3000, (9, 2)))
    rows = []
    for (a, b), n in zip(LAUNCH_PAIRS, LAUNCH_COUNTS):
        X = ground_points(rng, n, R[a], ned[a], R[b], ned[b]) if n else np.zeros((0, 3))
        rows.append(np.stack([arena.add(a, observe(rng, R[a], ned[a], X)),
                              arena.add(b, observe(rng, R[b], ned[b], X))], 1))
    maps = arena.shuffle(rng)
    rows = [np.stack([maps[a][r[:, 0]], maps[b][r[:, 1]]], 1).astype(np.int32)
            for (a, b), r in zip(LAUNCH_PAIRS, rows)]
    arena.finish()
    PROJ = np.stack([projection(R[i], ned[i]).ravel() for i in range(6)])
    pair_img = np.array(LAUNCH_PAIRS, np.int32)
    return dict(arena=arena, PROJ=PROJ, pair_img=pair_img, m_cnt=np.array(LAUNCH_COUNTS, np.int32),
                m_pairs=match_table(arena, pair_img, rows, LAUNCH_CLIP), rows=rows)


PACKED_TOTALS = (1, 256, 257, 600)
# per total: matches of pairs 0..7 -- an empty first pair, two empty pairs in the middle, an
# empty last pair
PACKED_COUNTS = {1: (0, 1, 0, 0, 0, 0, 0, 0), 256: (0, 100, 0, 0, 155, 1, 0, 0),
                 257: (0, 256, 0, 0, 1, 0, 0, 0), 600: (0, 256, 0, 0, 257, 86, 1, 0)}
PACKED_IMAGES = ((0, 1), (1, 2), (2, 0), (0, 1), (2, 1), (0, 2), (1, 0), (2, 1))


def packed_case(total, seed=13):
    """dict(arena, pair_img [8, 2], pair_proj [8, 2, 12], m_off [9], m_pairs [total, 2], rows):
    three images; every pair has cameras of its own (altitude 60 + 25 p m, yaw 40 p degrees), so a
    match triangulated with another pair's matrices lands metres away"""
    rng = np.random.default_rng([seed, total])
    counts = PACKED_COUNTS[total]
    assert sum(counts) == total
    arena = Arena(3)
    rows, proj = [], []
    for p, ((a, b), n) in enumerate(zip(PACKED_IMAGES, counts)):
        Ra, Rb = ned2cam(40.0 * p, 2.0, -1.0), ned2cam(40.0 * p + 4, -1.0, 2.0)
        na = np.array([5.0 * p, -3.0 * p, -60.0 - 25 * p])
        nb = na + [30.0, 15.0, 1.0]
        X = ground_points(rng, n, Ra, na, Rb, nb) if n else np.zeros((0, 3))
        rows.append(np.stack([arena.add(a, observe(rng, Ra, na, X)),
                              arena.add(b, observe(rng, Rb, nb, X))], 1))
        proj.append(np.stack([projection(Ra, na).ravel(), projection(Rb, nb).ravel()]))
    maps = arena.shuffle(rng)
    rows = [np.stack([maps[a][r[:, 0]], maps[b][r[:, 1]]], 1).astype(np.int32)
            for (a, b), r in zip(PACKED_IMAGES, rows)]
    arena.finish()
    m_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dict(arena=arena, pair_img=np.array(PACKED_IMAGES, np.int32), pair_proj=np.stack(proj),
                m_off=m_off, m_pairs=np.concatenate(rows).astype(np.int32), rows=rows)


def similarity_launch(cases, clip):
    """several (a_pts, b_pts) cases as ONE launch: image 2p is pair p's a, image 2p + 1 its b, the
    matches (i, i) in a shuffled order, poisoned rows past every count.
    dict(arena, pair_img, m_cnt, m_pairs [n, clip, 2], rows)"""
    rng = np.random.default_rng(17)
    arena = Arena(2 * len(cases))
    rows = []
    for p, (a, b) in enumerate(cases):
        ia, ib = arena.add(2 * p, a), arena.add(2 * p + 1, b)
        arena.add(2 * p + 1, rng.uniform(0, 3000, (p + 1, 2)))   # keypoints no match uses
        rows.append(np.stack([ia, ib], 1).astype(np.int32).reshape(-1, 2))
    arena.finish()
    pair_img = np.arange(2 * len(cases), dtype=np.int32).reshape(-1, 2)
    assert clip > max(len(r) for r in rows)
    return dict(arena=arena, pair_img=pair_img, m_cnt=np.array([len(r) for r in rows], np.int32),
                m_pairs=match_table(arena, pair_img, rows, clip), rows=rows)


def similarity_cases():
    """name -> (a_pts, b_pts) float32 of every similarity case the GPU tests launch"""
    rng = np.random.default_rng(19)
    pts = lambda n: rng.uniform([0, 0], [W_PX, H_PX], (n, 2)).astype(np.float32)
    cases = {'n%d' % n: similarity_case(n) for n in SIM_SIZES}
    cases['none'] = (pts(0), pts(0))
    cases['one'] = (pts(1), pts(1))
    cases['two'] = (pts(2), pts(2))
    cases['b_identical'] = (pts(5), np.repeat(pts(1), 5, 0))
    cases['plain'] = similarity_case(40, seed=3)
    cases['dry'] = dry_case()
    # one match whose keypoint in a is NaN: still fewer than two matches, whatever they hold
    cases['one_nan'] = (np.full((1, 2), np.nan, np.float32), pts(1))
    return cases


SIZE_CASES = tuple('n%d' % n for n in SIM_SIZES)
EDGE_CASES = ('none', 'one', 'two', 'b_identical', 'plain', 'dry', 'one_nan')
_sim_refs = {}


def similarity_reference(name):
    """one similarity case with its references, computed once and shared (callers do not modify
    it).  Index 0 is the kernel's direction 0 (image b's pixels onto image a's), index 1 the
    other way: M_ref (longdouble 2x3 or None), trace (longdouble), oracle (fit_similarity's
    float64 2x3 or None), trace64, oracle_err (similarity_error of the oracle), scale (the
    largest coordinate)"""
    from oracle.smart_oracle import fit_similarity
    if name not in _sim_refs:
        a, b = similarity_cases()[name]
        r = dict(a=a, b=b, scale=float(max(np.abs(a).max(), np.abs(b).max())) if len(a) else 1.0,
                 M_ref=[], trace=[], oracle=[], trace64=[], oracle_err=[])
        for frm, to in ((b, a), (a, b)):
            M, tr = similarity_trace(frm, to, np.longdouble)
            _M64, tr64 = similarity_trace(frm, to, np.float64)
            O = fit_similarity(frm, to) if len(frm) else None
            r['M_ref'].append(M)
            r['trace'].append(tr)
            r['trace64'].append(tr64)
            r['oracle'].append(O)
            r['oracle_err'].append(None if M is None or O is None else similarity_error(O, M, r['scale']))
        _sim_refs[name] = r
    return _sim_refs[name]


def similarity_tolerance(oracle_err):
    """max(16 x the float64 oracle's error on the case, 64 . 2^-52)"""
    return max(16 * oracle_err, SIM_FLOOR)


GROUND_SIZES = (1, 255, 256, 257)


def ground_case(n_feat, seed=23):
    """dict(M [5, 9], ned [5, 3], base [5], obs_img, obs_uv, feat_ptr, sky [n_obs] bool as the
    generator intends them): 1..7 observations per feature over five images; image 4 looks 50
    degrees ABOVE the horizon (the frame's corner lies 42 degrees off its axis), so every ray of it
    is a sky ray; feature 3 (and every 50th after it) is seen by it
    alone"""
    rng = np.random.default_rng([seed, n_feat])
    cam2body = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=float)
    M, ned, base = np.zeros((5, 9)), np.zeros((5, 3)), np.zeros(5)
    for i in range(5):
        pitch = 140.0 if i == 4 else rng.uniform(-8, 8)
        cam2ned = ned2cam(rng.uniform(0, 360), pitch, rng.uniform(-4, 4)).T
        body2ned = cam2ned.dot(np.linalg.inv(cam2body))
        M[i] = body2ned.dot(cam2body).dot(IK).ravel()
        ned[i] = [rng.uniform(-200, 200), rng.uniform(-200, 200), -rng.uniform(80, 140)]
        base[i] = rng.uniform(-10, 30)
    cnt = rng.integers(1, 8, n_feat)
    cnt[:min(7, n_feat)] = np.arange(7, 0, -1)[:min(7, n_feat)]
    feat_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    obs_img = rng.integers(0, 5, feat_ptr[-1]).astype(np.int32)
    obs_img[:7] = [0, 4, 1, 4, 2, 3, 4]                   # feature 0: seven rays, three of them sky
    for f in range(3, n_feat, 50):
        obs_img[feat_ptr[f]:feat_ptr[f + 1]] = 4
    obs_uv = rng.uniform([0, 0], [W_PX, H_PX], (len(obs_img), 2))
    return dict(M=M, ned=ned, base=base, obs_img=obs_img, obs_uv=obs_uv, feat_ptr=feat_ptr,
                sky=obs_img == 4)
