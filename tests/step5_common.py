"""Shared by tests/test_step5_map.py and tests/test_step5_map_gpu.py: the goldens of
tools/gen_step5_golden.py (tests/golden/step5_<scene>_<case>.pkl.gz) as a stand-in project, and
the point sets and queries surface_interp is held to scipy on."""
import glob
import gzip
import os
import pickle

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
CASES = sorted(glob.glob(os.path.join(GOLD, 'step5_*.pkl.gz')))
SWITCHES = ('grid_steps', 'texture_resolution', 'use_direct_pose', 'force_ground_elevation_m',
            'use_srtm_surface', 'no_extrapolate')
_cache = {}


def load(path):
    if path not in _cache:
        with gzip.open(path, 'rb') as f:
            _cache[path] = pickle.load(f)
    return _cache[path]


def project(g, analysis_dir=None):
    """the golden's poses and camera as a hostlib stand-in project (the recipe of test_mre_cull_gpu)"""
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd.hostlib import camera
    from imageanalysis_amd.hostlib.image_pose import PoseProject
    proj = PoseProject(g['names'], analysis_dir=analysis_dir)
    for im, p0, p1 in zip(proj.image_list, g['poses'], g['poses_opt']):
        for opt, (ned, ypr, quat) in ((False, p0), (True, p1)):
            im.set_camera_pose(ned, ypr[0], ypr[1], ypr[2], opt=opt)
            node = im.node.getChild('camera_pose_opt' if opt else 'camera_pose', True)
            for i in range(4):                  # the reference's stored quaternion, bit for bit
                node.setFloatEnum('quat', i, quat[i])
        im.image_file = os.path.join('/nonexistent', im.name + '.JPG')
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
    getNode('/config/directories', True).setString('images_source', '/nonexistent')
    return proj


def set_switches(module, g):
    for k in SWITCHES:
        setattr(module, k, g['switches'][k])


def reset_switches(module):
    for k, v in zip(SWITCHES, (8, 512, False, None, None, False)):
        setattr(module, k, v)


def log_lines(text):
    """the logger's lines of a captured stdout: without intersect2d's debug print per culled ray,
    and with the run's own directory cut out of the two lines that name it"""
    out = []
    for l in text.splitlines():
        if l.startswith(' returning high angle nans:'):
            continue
        for head in ('Notice: creating models directory =', 'EGG file name:',
                     'Warning: no polygons fully on surface, removing:'):
            if l.startswith(head):
                l = head + ' ' + os.path.basename(l)
        out.append(l)
    return out


def _queries_around(rng, pts, n, outside=0.1):
    """n queries in the points' bounding box, the first `outside` of them then pushed strictly beyond
    one of its four sides (by up to a quarter of the extent), so at least that share is outside"""
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    q = lo + rng.random((n, 2)) * (hi - lo)
    k = int(n * outside)
    rows = np.arange(k)
    axis = rng.integers(0, 2, k)
    off = (1.0 - rng.random(k)) * 0.25 * (hi - lo)[axis]          # (0, a quarter of the extent]
    q[rows, axis] = np.where(rng.integers(0, 2, k) == 1, hi[axis] + off, lo[axis] - off)
    return q


def interp_cases():
    """name -> (points [P,2], values [P], queries [N,2]): the sets surface_interp is held to scipy on"""
    rng = np.random.default_rng(20)
    cases = {}
    tri3 = np.array([[0.0, 0.0], [4.0, 0.5], [1.0, 3.0]])
    special = np.array([[0.0, 0.0], [4.0, 0.5], [1.0, 3.0], [2.0, 0.25], [2.5, 1.75], [0.5, 1.5],
                        [5.0 / 3, 3.5 / 3], [-1.0, -1.0], [5.0, 5.0], [2.0, 0.2], [2.0, 0.3]])
    cases['one_triangle'] = (tri3, np.array([1.0, -2.0, 7.5]), np.vstack([special, _queries_around(rng, tri3, 60, 0.4)]))
    quad = np.array([[0.0, 0.0], [4.0, 0.5], [1.0, 3.0], [4.5, 3.5]])
    cases['four_points'] = (quad, np.array([1.0, -2.0, 7.5, 3.0]),
                            np.vstack([special, quad, _queries_around(rng, quad, 60, 0.4)]))
    # a 21 x 21 lattice: every vertex, every edge midpoint (also the diagonals'), the hull edges
    g = np.arange(21.0)
    lat = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    mids = [lat, lat[lat[:, 0] < 20] + [0.5, 0.0], lat[lat[:, 1] < 20] + [0.0, 0.5],
            lat[(lat[:, 0] < 20) & (lat[:, 1] < 20)] + [0.5, 0.5]]
    t = np.linspace(0, 20, 161)
    hull = [np.stack([t, 0 * t], 1), np.stack([t, 0 * t + 20], 1), np.stack([0 * t, t], 1), np.stack([0 * t + 20, t], 1)]
    cases['lattice'] = (lat, np.sin(lat[:, 0] / 3.0) * 5 + lat[:, 1] ** 2 / 40.0, np.vstack(mids + hull))
    pts = rng.random((2000, 2)) * [300.0, 200.0]
    val = 8 * np.sin(pts[:, 0] / 40.0) + rng.normal(0, 1.0, 2000)
    q = _queries_around(rng, pts, 20000)
    cases['random'] = (pts, val, q)
    # a 600 : 1 skinny cluster inside a random set
    sk = np.stack([100 + rng.random(300) * 60.0, 100 + rng.random(300) * 0.1], 1)
    both = np.vstack([pts[:700], sk])
    cases['skinny'] = (both, np.concatenate([val[:700], rng.normal(0, 1.0, 300)]),
                       np.vstack([_queries_around(rng, both, 4000), _queries_around(rng, sk, 1001, 0.3)]))
    shift = np.array([123456.0, -65432.0])
    cases['shifted'] = (pts + shift, val, q + shift)
    return cases


def intersect2d(interp, ned, v, avg_ground, no_extrapolate=False):
    """what render_panda3d.intersect2d computes, stated for the tests: -> (point, rounds)"""
    from math import atan2, pi, sqrt
    p = list(ned)
    if v[2] <= 0.0:
        return p, 0
    tmp = interp([p[1], p[0]])[0]
    surface = tmp if (no_extrapolate or not np.isnan(tmp)) else avg_ground
    error = abs(p[2] - surface)
    count = 0
    while error > 0.01 and count < 25:
        d_proj = -(ned[2] - surface)
        factor = d_proj / v[2]
        p = [ned[0] + v[0] * factor, ned[1] + v[1] * factor, ned[2] + d_proj]
        tmp = interp([p[1], p[0]])[0]
        if no_extrapolate or not np.isnan(tmp):
            surface = tmp
        error = abs(p[2] - surface)
        count += 1
    dy, dx, dz = ned[0] - p[0], ned[1] - p[1], ned[2] - p[2]
    if atan2(-dz, sqrt(dx * dx + dy * dy)) * 180 / pi < 30:
        return [np.nan] * 3, count
    return p, count
