"""Shared by tests/test_chain_tools.py (host) and tests/test_chain_tools_gpu.py: the goldens of
tools/gen_chain_tools_golden.py, the project they describe, and numpy restatements of the two loops
(scripts/3c-match-triangulation.py --method triangulate with lib/line_solver.py, and
scripts/4b-colocated-feats.py with math supplied) that the kernels of csrc/chain_geom.hip are held to.
Nothing here imports the reference."""
import glob
import gzip
import math
import os
import pickle

import numpy as np

import undistort_restatement

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
TRI_CASES = sorted(glob.glob(os.path.join(GOLD, 'chain_triangulate_*.pkl.gz')))
COLO_CASES = sorted(glob.glob(os.path.join(GOLD, 'chain_colocated_*.pkl.gz')))
EPS = float(np.finfo(np.float64).eps)
CAM2BODY = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=float)

_cache = {}


def load(path):
    """a golden record, read once and shared (callers do not modify it)"""
    if path not in _cache:
        with gzip.open(path, 'rb') as f:
            _cache[path] = pickle.load(f)
    return _cache[path]


def project(g):
    """the golden's project on this package's stand-ins: both kinds of poses with the reference's
    stored quaternions bit for bit, both kinds of K / distortion"""
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd.hostlib import camera
    from imageanalysis_amd.hostlib.image_pose import PoseProject
    proj = PoseProject(g['names'])
    for im, p0, p1 in zip(proj.image_list, g['poses'], g['poses_opt']):
        for opt, (ned, ypr, quat) in ((False, p0), (True, p1)):
            im.set_camera_pose(ned, ypr[0], ypr[1], ypr[2], opt=opt)
            node = im.node.getChild('camera_pose_opt' if opt else 'camera_pose', True)
            for i in range(4):
                node.setFloatEnum('quat', i, quat[i])
    node = getNode('/config/camera', True)
    node.__dict__.pop('K_opt', None)
    node.__dict__.pop('dist_coeffs_opt', None)
    cam = g['camera']
    for key, vals in (('K', cam['K']), ('K_opt', cam['K_opt'])):
        node.setLen(key, 9)
        for i, v in enumerate(vals):
            node.setFloatEnum(key, i, v)
    camera.set_dist_coeffs(list(cam['dist']))
    camera.set_dist_coeffs(list(cam['dist_opt']), optimized=True)
    camera.set_image_params(g['width'], g['height'])
    return proj


class Scene(object):
    """the per-image arrays both restatements and the ABI calls need"""

    def __init__(self, g, group_index, attitude='initial'):
        proj = project(g)
        self.proj = proj
        self.K = np.array(g['camera']['K_opt'], np.float64).reshape(3, 3)
        self.dist = np.array(g['camera']['dist_opt'], np.float64)
        self.k4 = np.array([self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2]])
        IK = np.linalg.inv(self.K)
        n = len(proj.image_list)
        self.R = np.zeros((n, 3, 3))
        self.M = np.zeros((n, 9))
        self.pos = np.zeros((n, 3))
        for i, im in enumerate(proj.image_list):
            body2ned = im.get_body2ned(opt=(attitude == 'optimized'))
            self.R[i] = body2ned.dot(CAM2BODY)
            self.M[i] = body2ned.dot(CAM2BODY).dot(IK).ravel()
            self.pos[i] = im.get_camera_pose(opt=True)[0]
        names = set(g['groups'][group_index])
        self.in_group = np.array([nm in names for nm in g['names']], np.uint8)
        self.group_index = group_index


def group_of(g):
    a = g['argv']
    return int(a[a.index('--group') + 1]) if '--group' in a else 0


def flatten(matches):
    """list chains -> ptr i64, img i32, uv f64 [total, 2], group i32, ned f64 [n, 3] (NaN-free zeros
    where None), has_ned"""
    n = len(matches)
    ptr = np.zeros(n + 1, np.int64)
    if n:
        np.cumsum([len(m) - 2 for m in matches], out=ptr[1:])
    flat = [p for m in matches for p in m[2:]]
    img = np.array([p[0] for p in flat], np.int32)
    uv = np.array([p[1] for p in flat], np.float64).reshape(-1, 2)
    group = np.array([m[1] for m in matches], np.int32)
    has = np.array([m[0] is not None for m in matches], bool)
    ned = np.array([m[0] if m[0] is not None else [0.0, 0.0, 0.0] for m in matches], np.float64).reshape(-1, 3)
    return ptr, img, uv, group, ned, has


# ---------------------------------------------------------------------------------------------
# 3c --method triangulate
# ---------------------------------------------------------------------------------------------
def triangulate_restatement(sc, matches):
    """-> {chain: (x [3], cond_2(r), s, rho)} for every chain the reference's loop writes: group tag
    equal, >= 2 members in the group.  s = max(1, max |p_i|) (the caller adds |x_ref|), rho = the
    longest ray from a member camera to x.  An image index outside the project raises IndexError."""
    out = {}
    n_img = len(sc.pos)
    for c, match in enumerate(matches):
        if match[1] != sc.group_index:
            continue
        points, vectors = [], []
        for m in match[2:]:
            if not 0 <= m[0] < n_img:
                raise IndexError(c)
            if not sc.in_group[m[0]]:
                continue
            uv = undistort_restatement.undistort_points(np.array([m[1]], np.float32), sc.K, sc.dist)[0]
            proj = sc.M[m[0]].reshape(3, 3).dot(np.array([uv[0], uv[1], 1.0]))
            points.append(sc.pos[m[0]])
            vectors.append(proj / math.sqrt(np.dot(proj, proj)))
        if len(points) < 2:
            continue
        r = np.zeros((3, 3))
        q = np.zeros(3)
        for p, v in zip(points, vectors):
            v = v / np.linalg.norm(v)
            ri = np.identity(3) - np.outer(v, v)
            r = r + ri
            q = q + ri.dot(p)
        x = np.linalg.solve(r, q)
        P = np.array(points)
        out[c] = (x, float(np.linalg.cond(r, 2)), max(1.0, float(np.max(np.linalg.norm(P, axis=1)))),
                  float(np.max(np.linalg.norm(P - x, axis=1))))
    return out


def triangulate_bound(cond, s, x_ref):
    """|x_dev - x_ref| <= 256 eps cond_2(r) max(1, |x_ref|, max |p_i|): both solves are backward
    stable on an r, q that differ by a few ulp"""
    return 256 * EPS * cond * max(s, float(np.linalg.norm(x_ref)))


# ---------------------------------------------------------------------------------------------
# 4b-colocated-feats
# ---------------------------------------------------------------------------------------------
def pair_angles_restatement(sc, matches, min_angle):
    """-> (mark_list in the reference's order, smallest |angle - min_angle| / min_angle, pairs).
    compute_angle() as the reference means it (math.acos reachable); tmp < -1 is its except path
    (angle 0), a NaN angle never marks."""
    marks, margin, pairs = [], np.inf, 0
    n_img = len(sc.pos)
    for k, match in enumerate(matches):
        if match[1] != sc.group_index:
            continue
        members = match[2:]
        for m in members:
            if not 0 <= m[0] < n_img:
                raise IndexError(k)
        f = np.array(match[0], np.float64)
        for i, m1 in enumerate(members):
            for j, m2 in enumerate(members):
                if i < j and sc.in_group[m1[0]] and sc.in_group[m2[0]]:
                    v1, v2 = f - sc.pos[m1[0]], f - sc.pos[m2[0]]
                    with np.errstate(all='ignore'):
                        tmp = np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2))
                    if tmp > 1.0:
                        tmp = 1.0
                    angle = 0.0 if tmp < -1.0 else math.acos(tmp) * 180.0 / math.pi
                    pairs += 1
                    if not math.isnan(angle):
                        margin = min(margin, abs(angle - min_angle) / min_angle)
                    if angle < min_angle:
                        marks.append([k, i])
    return marks, margin, pairs


def counts_from_marks(ptr, marks):
    count = np.zeros(int(ptr[-1]), np.int32)
    for k, i in marks:
        count[ptr[k] + i] += 1
    return count
