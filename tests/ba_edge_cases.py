"""TEST HELPER (host only): small synthetic bundle-adjustment problems whose STRUCTURE -- how many
observations every camera and every point has -- is prescribed, each the smallest that crosses one
loop boundary or branch of csrc/ba_kernels.hip / ba_linalg.hip / ba_schur.hip:

  tiny-{1,2,3}            one camera, O = P = 1, 2, 3 observations
  lanes-{first,middle,last}   9 cameras with 0, 1, 63, 64, 65, 255, 256, 257, 513 observations (the
                          empty camera first / in the middle / last): the 64-lane trips of
                          jt_cam_kernel, the 256-thread trips of acc_cam / lsmr_fwd / schur_adj, an
                          empty camera, the XCD remap of lsmr_fwd with q = 1, r = 1
  cams_n-{3,4,5,7,8,16,17}    ~40 observations per camera: 4 cameras per jt_cam workgroup, the q / r
                          cases of the XCD remap, 7 C below the fixed n-vector grids
  points_n-{255,256,257,513}  per-point counts 0, 1, 2, 3, 10, 11; in the solver's internal point
                          order the first 256 points hold exactly 1024 point-sorted slots and (513)
                          the next 256 exactly 1025: the 256-point workgroups and ADJ_CH rounds of
                          lsmr_adj_kernel, unobserved and single-observation points
  landmark                1025 cameras with 2 ordinary observations each + one point seen by all of
                          them (P = 700): a point spanning ADJ_CH, schur_factor's 1024 stride, sums
                          of per-camera partials over > 1024 cameras
  ragged-{255,256,257,511}    5 cameras: the LDS write-back tail of ba_residual_jac_kernel<false>
  degenerate_q            cams_n-16 with |q|^2 < 4 eps for one camera (residual / Jacobian only)
  two_obs                 cams_n-3 + a fourth camera with two observations of well-observed points:
                          the rank-deficient 7x7 block behind the diagonal fallback of schur_factor

Cameras are nadir on a compact grid 100 m above the points (1 m apart for the landmark case, 4 m
otherwise), so that every point projects inside the 5472 x 3648 frame of every camera and the
distortion polynomial stays in its sane range; quaternions are unnormalised (scale 0.5 - 2, as in
test_ba_gpu.py); uv = the reference projection at the true parameters + 0.5 px noise; x0 = the true
parameters slightly perturbed.  Observations are camera-major like the reference's.
"""
import numpy as np

import ba_reference as ref

F, CU, CV = 3666.6665, 2736.0, 1824.0
DIST = (-0.12, 0.083, -0.0016, -0.00096, -0.012)
CALIB = np.array([F, F, CU, CV, *DIST])
LANES = [0, 1, 63, 64, 65, 255, 256, 257, 513]
CAMS_N = [3, 4, 5, 7, 8, 16, 17]
POINTS_N = [255, 256, 257, 513]
RAGGED = [255, 256, 257, 511]

NAMES = (['tiny-%d' % k for k in (1, 2, 3)] + ['lanes-first', 'lanes-middle', 'lanes-last'] +
         ['cams_n-%d' % c for c in CAMS_N] + ['points_n-%d' % p for p in POINTS_N] + ['landmark'] +
         ['ragged-%d' % o for o in RAGGED] + ['degenerate_q', 'two_obs'])
# the structures the solver-level comparisons run on
LSMR_NAMES = [n for n in NAMES if n.split('-')[0] in ('lanes', 'cams_n', 'points_n', 'landmark')]
SCHUR_NAMES = LSMR_NAMES                              # converged Schur step (landmark: sparse reference)


def _from_cam_counts(counts, P, rng):
    """camera c takes counts[c] distinct points, dealt round robin over a random order of the points"""
    counts = np.asarray(counts, np.int64)
    assert counts.max() <= P
    order = rng.permutation(P)
    cam = np.repeat(np.arange(len(counts)), counts)
    return cam, order[np.arange(cam.size) % P]


def points_n_counts(P):
    """per-point observation counts of points_n-P in the solver's internal point order"""
    nz = 3 if P <= 256 else 1                         # unobserved points (they sort last)
    counts = np.tile([1, 2, 3, 10], 129)[:P - nz]

    def fix(lo, hi, target):
        diff = target - counts[lo:hi].sum()
        tens = lo + np.nonzero(counts[lo:hi] == 10)[0]
        assert 0 <= diff <= tens.size
        counts[tens[:diff]] += 1

    if P >= 256:
        fix(0, 256, 1024)
    if P == 513:
        fix(256, 512, 1025)
    return np.concatenate([counts, np.zeros(nz, np.int64)])


def _points_n(P, rng, C=24):
    counts = points_n_counts(P)
    n_seen = int((counts > 0).sum())
    first = np.where(counts > 0, np.arange(P) * (C - counts.max()) // n_seen, C)
    cam = np.concatenate([first[j] + np.arange(counts[j]) for j in range(P)])
    pt = np.repeat(np.arange(P), counts)
    # reference ids: the groups of points that share a first camera change places as wholes, so the
    # ids are a non-trivial permutation while (first camera, id) still sorts to the order above
    gkey = rng.permutation(C + 1)[first]
    new_id = np.empty(P, np.int64)
    new_id[np.lexsort((np.arange(P), gkey))] = np.arange(P)
    return C, cam, new_id[pt]


def pairs(name, rng):
    """(C, P, cam, pt) of the structure, observations in generation order"""
    kind, _, arg = name.partition('-')
    if kind == 'tiny':
        k = int(arg)
        return 1, k, np.zeros(k, np.int64), np.arange(k)
    if kind == 'lanes':
        counts = LANES[1:]
        at = {'first': 0, 'middle': 4, 'last': 8}[arg]
        counts = counts[:at] + [0] + counts[at:]
        return (9, 520) + _from_cam_counts(counts, 520, rng)
    if kind in ('cams_n', 'degenerate_q'):
        C = int(arg) if kind == 'cams_n' else CAMS_N[5]
        return (C, 60) + _from_cam_counts(rng.integers(36, 45, C), 60, rng)
    if kind == 'two_obs':
        return (4, 60) + _from_cam_counts([40, 41, 39, 2], 60, rng)
    if kind == 'points_n':
        C, cam, pt = _points_n(int(arg), rng)
        return C, int(arg), cam, pt
    if kind == 'landmark':
        C, P = 1025, 700
        cam = np.repeat(np.arange(C), 3)
        pt = np.stack([(2 * np.arange(C)) % (P - 1), (2 * np.arange(C) + 1) % (P - 1),
                       np.full(C, P - 1)], 1).ravel()
        return C, P, cam, pt
    if kind == 'ragged':
        O = int(arg)
        counts = np.full(5, O // 5)
        counts[:O % 5] += 1
        return (5, 120) + _from_cam_counts(counts, 120, rng)
    raise KeyError(name)


def internal_point_order(C, P, cam_idx, pt_idx):
    """old id of every point in DeviceBA's internal order: by first observing camera, then by id"""
    first = np.full(P, C, np.int64)
    np.minimum.at(first, np.asarray(pt_idx, np.int64), np.asarray(cam_idx, np.int64))
    return np.lexsort((np.arange(P), first))


def make(name, seed=0, with_calib=False, shuffle=False):
    """dict(name, C, P, O, cam_idx, pt_idx, uv, x0, calib, with_calib): x0 carries the 8 calibration
    parameters behind the points with_calib, else `calib` (9) is the fixed calibration.
    shuffle: the observations of every camera in random order (still camera-major)."""
    rng = np.random.default_rng([seed, NAMES.index(name)])
    C, P, cam, pt = pairs(name, rng)
    key = rng.random(cam.size) if shuffle else np.arange(cam.size)
    o = np.lexsort((key, cam))
    cam, pt = cam[o].astype(np.int32), pt[o].astype(np.int32)
    O = cam.size
    spacing = 1.0 if C > 100 else 4.0
    ncol = int(np.ceil(np.sqrt(C)))
    grid = np.stack([np.arange(C) // ncol, np.arange(C) % ncol], 1).astype(np.float64)
    grid -= grid.mean(0)
    cams = np.zeros((C, 7))
    cams[:, :2] = grid * spacing + rng.normal(0, 0.1, (C, 2))
    cams[:, 2] = -100.0 + rng.normal(0, 1.0, C)
    # nadir (ypr = heading, -90, 0 <=> q ~ (c, 0, -c, 0)), unnormalised
    cams[:, 3:] = np.array([0.7071, 0, -0.7071, 0]) * rng.uniform(0.5, 2.0, (C, 1)) \
        + rng.normal(0, 0.02, (C, 4))
    pts = np.stack([rng.uniform(-20, 20, P), rng.uniform(-30, 30, P), rng.normal(0, 1.5, P)], 1)
    if name == 'degenerate_q':
        # |q|^2 < 4 eps: the rotation is the identity, the camera looks along +north from the side
        cams[5] = [-100.0, 0.3, -0.5, 1e-9, 0.3e-9, -0.2e-9, 0.1e-9]
    truth = np.hstack([cams.ravel(), pts.ravel()])
    proj = -ref.residual(truth, C, P, cam, pt, np.zeros((O, 2)), CALIB)
    assert proj[:, 0].min() > 0 and proj[:, 0].max() < 2 * CU, name
    assert proj[:, 1].min() > 0 and proj[:, 1].max() < 2 * CV, name
    uv = proj + rng.normal(0, 0.5, (O, 2))
    cams0, pts0 = cams.copy(), pts + rng.normal(0, 0.05, (P, 3))
    cams0[:, :3] += rng.normal(0, 0.03, (C, 3))
    keep = ref.degenerate_cameras(truth, C)
    cams0[:, 3:] += np.where(keep[:, None], 0.0, rng.normal(0, 1e-3, (C, 4)))
    x0 = np.hstack([cams0.ravel(), pts0.ravel()])
    if with_calib:
        x0 = np.hstack([x0, [F * 1.002, CU + 2.0, CV - 1.5, *(np.asarray(DIST) * 0.95)]])
    return dict(name=name, C=C, P=P, O=O, cam_idx=cam, pt_idx=pt, uv=uv, x0=x0,
                calib=None if with_calib else CALIB.copy(), with_calib=with_calib)


# The lower end of dreg: test_ba_schur_gpu.py draws U(1e-3, 3e-2) on the goldens.  The edge-case
# problems have gauge directions J does not see at all (unobserved points, empty cameras), so the
# smallest singular value of A IS the smallest dreg, and with 1e-3 cond(A) comes out at 1000 - 2700,
# above ba_mid's 977.  With 4e-3 every structure stays below it
# (test_ba_reference.py::test_schur_problems_no_worse_conditioned_than_ba_mid).
DREG_RANGE = (4e-3, 3e-2)


def scaling(prob_n, colnorm, seed, dreg_range=DREG_RANGE):
    """the d / dreg recipe of test_ba_schur_gpu.py::test_schur_step_equals_direct_solve:
    d = 1 / colnorm * U(0.5, 2), dreg = U(dreg_range); a column nothing observes gets d = 1"""
    rng = np.random.default_rng(seed)
    cn = np.where(colnorm > 0, colnorm, 1.0)
    d = np.where(colnorm > 0, (1.0 / cn) * rng.uniform(0.5, 2.0, prob_n), 1.0)
    return d, rng.uniform(dreg_range[0], dreg_range[1], prob_n)


def scaling_goldens(prob_n, colnorm, seed):
    """... with the range the existing test uses on the goldens"""
    return scaling(prob_n, colnorm, seed, (1e-3, 3e-2))


def scaling_lsmr(prob_n, colnorm, seed):
    """the recipe of test_ba_solver_gpu.py's LSMR comparisons: d = 1 / colnorm, dreg = U(0.01, 0.1)"""
    rng = np.random.default_rng(seed)
    return np.where(colnorm > 0, 1.0 / np.where(colnorm > 0, colnorm, 1.0), 1.0), rng.uniform(0.01, 0.1, prob_n)


def colnorm_of(Jc, Jp, Jk, cam, pt, C, P):
    """sqrt of the column sums of J.^2, reference column order"""
    cs = np.zeros((C, 7)), np.zeros((P, 3))
    np.add.at(cs[0], np.asarray(cam, np.int64), (Jc * Jc).sum(1))
    np.add.at(cs[1], np.asarray(pt, np.int64), (Jp * Jp).sum(1))
    tail = [] if Jk is None else [(Jk * Jk).sum((0, 1))]
    return np.sqrt(np.concatenate([cs[0].ravel(), cs[1].ravel(), *tail]))


def reference_system(p, recipe, seed=1):
    """(A csr, b, d, dreg) of the subproblem min ||A x - b||, A = [J D; Dreg], b = [r; 0], from the
    REFERENCE Jacobian of problem p at x0 -- what the host-side condition tests look at"""
    C, P = p['C'], p['P']
    Jc, Jp, Jk = ref.jac_blocks(p['x0'], C, P, p['cam_idx'], p['pt_idx'], p['uv'], p['calib'])
    r = ref.residual(p['x0'], C, P, p['cam_idx'], p['pt_idx'], p['uv'], p['calib']).ravel()
    d, dreg = recipe(p['x0'].size, colnorm_of(Jc, Jp, Jk, p['cam_idx'], p['pt_idx'], C, P), seed)
    A = ref.dense_A(Jc, Jp, Jk, p['cam_idx'], p['pt_idx'], d, dreg, C, P)
    return A, np.concatenate([r, np.zeros(p['x0'].size)]), d, dreg
