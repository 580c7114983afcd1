#!/usr/bin/env python3
"""Goldens of the terrain module from the reference's OWN scripts/lib/srtm.py.

Needs a checkout of the reference project, given by the IAMX_REFERENCE environment variable (the
directory that holds its scripts/).  lib/srtm.py is imported with two stand-in modules put into
sys.modules here when the real ones are missing: `pylab` (giving floor) and `navpy` (forwarding to
imageanalysis_amd.hostlib.geodesy: parity with navpy itself is unpinned).

  tests/golden/terrain_tiles.pkl.gz   parse + make_lla_interpolator + initialize on tiles written from
      a seed (tests/terrain_common.py) into a temporary cache directory: one tile, a reference point
      1 km from a tile corner (four tiles), a tile holding 65535 / 10001 / 40000.  width_m != height_m
      so that rows != cols.  Stored: seeds, reference point, the NED axes and grids, a few look-ups
      of the tile's own lla interpolator -- not the tiles.
  tests/golden/terrain_queries.pkl.gz ned_interp at nodes, cell centres, the exact border, just
      outside it and NaN.
  tests/golden/terrain_rays.pkl.gz    interpolate_vector per ray with ned_interp wrapped to log every
      look-up: the point returned, the iteration count, every iteration's error.  Scenes: smooth
      (cameras 80-150 m up, rays down to 15 degrees below the horizon; 257 rays x 3 images), n1 / n63 /
      n64 / n65 (rays per image), edge (a camera on the ground, v[2] = 0 and < 0, NaN rays, a camera
      outside the grid, rays that leave the grid), steep (some shallow rays reach the cap of 25).
  tests/golden/terrain_mid.pkl.gz     the mid scene of tests/golden/ba_mid_in.pkl: the reference's
      project.projectVectors + srtm.interpolate_vectors per image of group 0 (render_panda3d.py:164-205
      with use_direct_pose and use_srtm_surface) over a terrain set as srtm.ned_interp.

A scene is refused when a decision value lies within 1e-6 of its threshold: `error` against 0.01 at
every iteration (relative), v[2] against 0 (absolute; exactly 0 is the case `v[2] = 0`, decided by
`<=`), a look-up's distance from the grid border (absolute, metres).  Rays that end at the cap
oscillate and amplify rounding: they are compared by iters and flags only, may be at most 5 % of the
steep scene's rays and none of any other scene's; checked here on the reference's own run.

    IAMX_REFERENCE=<reference checkout> python tools/gen_terrain_golden.py
"""
import contextlib
import gzip
import io
import os
import pickle
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.path.join(os.environ.get('IAMX_REFERENCE', ''), 'scripts')
GOLD = os.path.join(REPO, 'tests', 'golden')
MIN_MARGIN = 1e-6
CAP_SHARE = 0.05

sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
from imageanalysis_amd.hostlib import geodesy                    # noqa: E402  (before any navpy stand-in)
from imageanalysis_amd.render_panda3d import unit_rays           # noqa: E402
import terrain_common as tc                                      # noqa: E402


def import_reference_srtm():
    try:
        import pylab                                             # noqa: F401
    except ImportError:
        m = types.ModuleType('pylab')
        m.floor = np.floor
        m.__all__ = ['floor']
        sys.modules['pylab'] = m
    if geodesy._navpy is None:
        m = types.ModuleType('navpy')
        m.ned2lla = geodesy.ned2lla
        m.lla2ned = geodesy.lla2ned
        sys.modules['navpy'] = m
    sys.path.insert(0, REF)
    from lib import srtm
    return srtm


def dump(name, rec):
    path = os.path.join(GOLD, 'terrain_%s.pkl.gz' % name)
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        pickle.dump(rec, f, protocol=4)
    size = os.path.getsize(path)
    print('%-28s bytes=%d' % (os.path.basename(path), size))
    if size >= 1000000:
        sys.exit('%s is too large' % path)


# ---- 1. tile handling ----------------------------------------------------------------------------
TILE_CASES = (
    dict(name='one', ref=[45.3, -93.6, 280.0], tiles={'N45W094': (3, None)}),
    dict(name='corner', ref=[45.0064, -92.991, 300.0],
         tiles={'N44W094': (11, None), 'N44W093': (12, None), 'N45W094': (13, None), 'N45W093': (14, None)}),
    dict(name='voids', ref=[45.3, -93.6, 280.0], tiles={'N45W094': (5, (826, 856, 456, 506))}),
)
WIDTH_M, HEIGHT_M, STEP_M = 2400, 1500, 30


def tile_goldens(srtm):
    cases = []
    for case in TILE_CASES:
        cache = tempfile.mkdtemp(prefix='iamx_terrain_tiles_')
        try:
            for tile, (seed, voids) in case['tiles'].items():
                tc.write_tile(cache, tile, seed, voids)
            init = srtm.SRTM.__init__

            def with_cache(self, lat, lon, dict_path, _init=init, _cache=cache):
                _init(self, lat, lon, dict_path)
                self.set_srtm_cache_dir(_cache)
            srtm.SRTM.__init__ = with_cache
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    srtm.tile_dict = {}
                    srtm.initialize(case['ref'], WIDTH_M, HEIGHT_M, STEP_M)
            finally:
                srtm.SRTM.__init__ = init
            assert sorted(srtm.tile_dict) == sorted(case['tiles']), (sorted(srtm.tile_dict), case['tiles'])
            rng = np.random.default_rng(7)
            probes = {}
            for tile, obj in srtm.tile_dict.items():
                # the tile's own interpolator: nodes at and next to its four corners and random points
                q = np.vstack([[obj.lon + a, obj.lat + b] for a in (0.0, 1.0 / 1200, 0.5, 1.0) for b in (0.0, 1.0 / 1200, 0.5, 1.0)]
                              + [[obj.lon - 1e-9, obj.lat + 0.5]]
                              + [np.array([obj.lon, obj.lat]) + rng.random((40, 2))])
                probes[tile] = (q, np.array(obj.lla_interpolate(q), np.float64))
            rec = dict(case, width_m=WIDTH_M, height_m=HEIGHT_M, step_m=STEP_M,
                       tile_order=list(srtm.tile_dict), axis_n=np.array(srtm.ned_interp.grid[0]),
                       axis_e=np.array(srtm.ned_interp.grid[1]), grid=np.array(srtm.ned_interp.values),
                       probes=probes)
            assert rec['grid'].shape == (int(HEIGHT_M / STEP_M) + 1, int(WIDTH_M / STEP_M) + 1)
            if case['name'] == 'voids':
                assert (rec['grid'] < 250).any(), 'no void reached the NED grid'
            cases.append(rec)
            print('tiles/%-8s tiles=%d grid=%r min=%.1f max=%.1f' % (case['name'], len(case['tiles']),
                                                                     rec['grid'].shape, rec['grid'].min(), rec['grid'].max()))
        finally:
            shutil.rmtree(cache, ignore_errors=True)
    dump('tiles', dict(cases=cases))
    return cases[0]


# ---- 2. ned_interp queries -------------------------------------------------------------------------
def query_goldens(srtm, case):
    import scipy.interpolate
    an, ae, grid = case['axis_n'], case['axis_e'], case['grid']
    srtm.ned_interp = scipy.interpolate.RegularGridInterpolator((an, ae), grid, bounds_error=False, fill_value=-32768)
    rng = np.random.default_rng(8)
    nodes = np.stack(np.meshgrid(an, ae, indexing='ij'), -1).reshape(-1, 2)
    centres = np.stack(np.meshgrid((an[:-1] + an[1:]) / 2, (ae[:-1] + ae[1:]) / 2, indexing='ij'), -1).reshape(-1, 2)
    t = rng.uniform(ae[0], ae[-1], 40)
    s = rng.uniform(an[0], an[-1], 40)
    border = np.vstack([np.stack([np.full(40, an[0]), t], 1), np.stack([np.full(40, an[-1]), t], 1),
                        np.stack([s, np.full(40, ae[0])], 1), np.stack([s, np.full(40, ae[-1])], 1)])
    just = np.vstack([np.stack([np.full(40, np.nextafter(an[0], -np.inf)), t], 1),
                      np.stack([np.full(40, np.nextafter(an[-1], np.inf)), t], 1),
                      np.stack([s, np.full(40, np.nextafter(ae[0], -np.inf))], 1),
                      np.stack([s, np.full(40, np.nextafter(ae[-1], np.inf))], 1),
                      [[an[0] - 1.0, 0.0], [0.0, ae[-1] + 1e6], [1e300, 0.0], [-np.inf, 0.0], [np.inf, np.inf]]])
    nan = np.array([[np.nan, 0.0], [0.0, np.nan], [np.nan, np.nan], [np.nan, 1e9], [-1e9, np.nan]])
    rand = np.stack([rng.uniform(an[0], an[-1], 3000), rng.uniform(ae[0], ae[-1], 3000)], 1)
    groups = dict(nodes=nodes, centres=centres, border=border, outside=just, nan=nan, random=rand)
    out = {}
    for k, q in groups.items():
        z = np.array(srtm.ned_interp(q), np.float64)
        one = np.array([srtm.ned_interp([a, b])[0] for a, b in q[:50]])
        assert np.array_equal(one, z[:50], equal_nan=True)
        out[k] = (q, z)
        print('queries/%-8s n=%d fill=%d nan=%d' % (k, len(q), int((z == -32768).sum()), int(np.isnan(z).sum())))
    assert (out['outside'][1] == -32768).all() and np.isnan(out['nan'][1]).all()
    assert not (out['border'][1] == -32768).any()
    dump('queries', dict(axis_n=an, axis_e=ae, grid=grid, groups=out))


# ---- 3. rays ------------------------------------------------------------------------------------------
class Logged(object):
    def __init__(self, f):
        self.f, self.grid, self.values = f, f.grid, f.values
        self.q, self.z = [], []

    def __call__(self, x):
        r = self.f(x)
        self.q.append((float(x[0]), float(x[1])))
        self.z.append(float(r[0]))
        return r


def run_scene(srtm, name, axis_n, axis_e, grid, ned, v, cap_share=0.0):
    """the reference's interpolate_vector for every ray of every image; ned [I, 3], v [I, n, 3]"""
    import scipy.interpolate
    f = Logged(scipy.interpolate.RegularGridInterpolator((axis_n, axis_e), grid, bounds_error=False,
                                                         fill_value=-32768))
    srtm.ned_interp = f
    I, n = v.shape[:2]
    pts = np.empty((I, n, 3))
    iters = np.zeros((I, n), np.uint8)
    flags = np.zeros((I, n), np.uint8)
    err_ptr, errs = [0], []
    margin = dict(error=np.inf, v2=np.inf, border=np.inf)
    for i in range(I):
        for k in range(n):
            start = len(f.z)
            with contextlib.redirect_stdout(io.StringIO()):
                p = srtm.interpolate_vector(ned[i].tolist(), v[i, k])
            pts[i, k] = p
            q, z = f.q[start:], f.z[start:]
            if v[i, k, 2] != 0.0 and not np.isnan(v[i, k, 2]):
                margin['v2'] = min(margin['v2'], abs(v[i, k, 2]))
            if not len(z):
                flags[i, k] |= 1
                assert v[i, k, 2] <= 0.0
                err_ptr.append(len(errs))
                continue
            # the errors, from the look-ups: the ground in force after each
            ground = z[0] if (not np.isnan(z[0]) and z[0] > -32768) else 0.0
            e = [abs(ned[i, 2] + ground)]
            for zz in z[1:]:
                d = -(ned[i, 2] + ground)
                if not np.isnan(zz) and zz > -32768:
                    ground = zz
                e.append(abs(ned[i, 2] + d + ground))
            iters[i, k] = len(z) - 1
            for ee in e:
                if not np.isnan(ee):
                    margin['error'] = min(margin['error'], abs(ee - 0.01) / 0.01)
            # (the loop went on exactly while error > 0.01 and count < 25)
            assert all(x > 0.01 for x in e[:-1]) and (not e[-1] > 0.01 or len(e) == 26), (name, i, k, e)
            if len(e) == 26 and e[-1] > 0.01:
                flags[i, k] |= 2
            for (a, b), zz in zip(q, z):
                if np.isnan(a) or np.isnan(b):
                    continue
                dist = min(abs(a - axis_n[0]), abs(a - axis_n[-1]), abs(b - axis_e[0]), abs(b - axis_e[-1]))
                margin['border'] = min(margin['border'], dist)
                if zz == -32768:
                    flags[i, k] |= 4
            errs.extend(e)
            err_ptr.append(len(errs))
    capped = (flags & 2) != 0
    share = capped.mean()
    if min(margin.values()) < MIN_MARGIN:
        sys.exit('rays/%s sits on a decision: margins %r' % (name, margin))
    if share > cap_share:
        sys.exit('rays/%s: %.1f %% of the rays end at the cap (allowed %.0f %%)' % (name, 100 * share, 100 * cap_share))
    print('rays/%-8s images=%d rays=%d sky=%d capped=%d left=%d nan=%d iters<=%d margins %s' % (
        name, I, n, int(((flags & 1) != 0).sum()), int(capped.sum()), int(((flags & 4) != 0).sum()),
        int(np.isnan(pts).any(axis=2).sum()), int(iters.max()),
        ' '.join('%s=%.3g' % kv for kv in margin.items())))
    return dict(name=name, ned=ned, v=v, pts=pts, iters=iters, flags=flags, err_ptr=np.array(err_ptr, np.int64),
                errors=np.array(errs, np.float64), margins=margin)


def rotation(rng, max_tilt_deg):
    """a camera looking down, tilted by up to max_tilt_deg about a random horizontal axis, any heading:
    columns = the camera's x, y, z (optical) axes in NED"""
    yaw = rng.uniform(0, 2 * np.pi)
    tilt = np.radians(rng.uniform(0, max_tilt_deg))
    axis = rng.uniform(0, 2 * np.pi)
    a = np.array([np.cos(axis), np.sin(axis), 0.0])
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(tilt) * K + (1 - np.cos(tilt)) * K.dot(K)
    cy, sy = np.cos(yaw), np.sin(yaw)
    down = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    return R.dot(down)


def camera_rays(rng, I, n, max_tilt_deg):
    """M [I, 3, 3] = R . IK and a pixel grid uv [n, 2] of a 4000 x 3000 camera with f = 2800 px; the rays
    as render_panda3d.unit_rays gives them"""
    IK = np.linalg.inv(np.array([[2800.0, 0, 2000.0], [0, 2800.0, 1500.0], [0, 0, 1.0]]))
    M = np.array([rotation(rng, max_tilt_deg).dot(IK) for _ in range(I)])
    uv = np.stack([rng.uniform(0, 4000, n), rng.uniform(0, 3000, n)], 1)
    v = np.array([unit_rays(M[i], uv) for i in range(I)], np.float64)
    return M, uv, v


def ray_goldens(srtm):
    import scipy.interpolate
    rng = np.random.default_rng(9)
    axis_n = np.linspace(-HEIGHT_M * 0.5, HEIGHT_M * 0.5, int(HEIGHT_M / STEP_M) + 1)
    axis_e = np.linspace(-WIDTH_M * 0.5, WIDTH_M * 0.5, int(WIDTH_M / STEP_M) + 1)
    nn, ee = np.meshgrid(axis_n, axis_e, indexing='ij')
    smooth = 250.0 + 15.0 * np.sin(nn / 200.0) + 10.0 * np.cos(ee / 150.0) + 0.01 * ee
    steep = 250.0 + 20.0 * np.sin(nn / 40.0) + 12.0 * np.cos(ee / 55.0)
    terrains = dict(smooth=smooth, steep=steep)
    ground = lambda g, p: float(scipy.interpolate.RegularGridInterpolator((axis_n, axis_e), g)(p)[0])  # noqa: E731

    def cameras(g, I, lo=80.0, hi=150.0, spread=150.0):
        ned = np.zeros((I, 3))
        for i in range(I):
            ned[i, :2] = rng.uniform(-spread, spread, 2)
            ned[i, 2] = -(ground(g, ned[i, :2]) + rng.uniform(lo, hi))
        return ned

    scenes = []
    # rays down to 15 degrees below the horizon: the camera's field of view is +-41 degrees across the
    # diagonal, so a tilt of up to 34 degrees leaves the shallowest ray at 90 - 34 - 41 = 15
    for name, n in (('smooth', 257), ('n1', 1), ('n63', 63), ('n64', 64), ('n65', 65)):
        M, uv, v = camera_rays(rng, 3, n, 34.0)
        rec = run_scene(srtm, name, axis_n, axis_e, smooth, cameras(smooth, 3), v)
        rec.update(terrain='smooth', M=M, uv=uv)
        scenes.append(rec)

    # edge: image 0 stands on the ground (0 iterations), with rays at and above the horizon and NaN rays;
    # image 1 is outside the grid (first ground 0.0) and looks into it; image 2 is near the east border
    # and its rays leave the grid during the iteration
    M, uv, v = camera_rays(rng, 3, 64, 30.0)
    ned = cameras(smooth, 3)
    ned[0, 2] = -ground(smooth, ned[0, :2])
    v[0, 5] = [0.6, 0.8, 0.0]
    v[0, 6] = [0.6, 0.0, -0.8]
    v[0, 7] = [np.nan, np.nan, np.nan]
    v[0, 8] = [np.nan, 0.6, 0.8]
    ned[1] = [-900.0, 100.0, -420.0]
    az = rng.uniform(-0.5, 0.5, 64)
    el = np.radians(rng.uniform(35.0, 70.0, 64))
    v[1] = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    v[1, 3] = [0.0, 0.0, 1.0]
    v[1, 4] = [np.nan, 0.0, 1.0]
    v[1, 5] = [0.0, 0.6, np.nan]
    ned[2, :2] = [40.0, 1120.0]
    ned[2, 2] = -(ground(smooth, ned[2, :2]) + 110.0)
    az = rng.uniform(-1.0, 1.0, 64)
    el = np.radians(rng.uniform(15.0, 60.0, 64))
    v[2] = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], 1)
    rec = run_scene(srtm, 'edge', axis_n, axis_e, smooth, ned, v)
    rec.update(terrain='smooth', M=None, uv=None)
    assert (rec['iters'][0] == 0).all() and ((rec['flags'][2] & 4) != 0).sum() >= 8
    assert ((rec['flags'][1] & 4) != 0).all()
    scenes.append(rec)

    # steep: the slope is up to 0.5, rays steeper than 45 degrees converge; a few at 12-20 degrees do not
    M, uv, v = camera_rays(rng, 3, 128, 4.0)
    pick = rng.choice(3 * 128, 12, replace=False)
    for k in pick:
        az, el = rng.uniform(0, 2 * np.pi), np.radians(rng.uniform(12.0, 20.0))
        v[k // 128, k % 128] = [np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)]
    rec = run_scene(srtm, 'steep', axis_n, axis_e, steep, cameras(steep, 3, 90.0, 110.0, 60.0), v, CAP_SHARE)
    rec.update(terrain='steep', M=None, uv=None)
    assert ((rec['flags'] & 2) != 0).any(), 'no ray reached the cap'
    scenes.append(rec)
    dump('rays', dict(axis_n=axis_n, axis_e=axis_e, terrains=terrains, scenes=scenes))


# ---- 4. the mid scene through the reference's Step 5 lines -------------------------------------------
def mid_golden(srtm):
    import scipy.interpolate
    import gen_step5_golden as s5
    s5.mre.setup_paths()
    from lib import camera, groups, project
    work = tempfile.mkdtemp(prefix='iamx_terrain_mid_')
    try:
        inp = s5.build_project('mid', work)
        with contextlib.redirect_stdout(io.StringIO()):
            proj = project.ProjectMgr(work)
            proj.load_images_info()
        group = groups.load(proj.analysis_dir)[0]
        K = inp['K']
        camera.set_K(K[0], K[4], K[2], K[5], optimized=True)
        camera.set_dist_coeffs(list(inp['dist']), optimized=True)
        width, height = camera.get_image_params()
        IK = np.linalg.inv(camera.get_K(optimized=True))
        grid_steps = 8
        grid_list = [[u, v] for v in np.linspace(0, height, grid_steps + 1) for u in np.linspace(0, width, grid_steps + 1)]
        axis_n = np.linspace(-240.0, 420.0, 45)
        axis_e = np.linspace(-300.0, 450.0, 51)
        nn, ee = np.meshgrid(axis_n, axis_e, indexing='ij')
        grid = 6.0 + 3.0 * np.sin(nn / 60.0) + 2.0 * np.cos(ee / 45.0) + 0.004 * nn
        pts, neds, rays = [], [], []
        for name in group:
            image = proj.findImageByName(name)
            proj_list = project.projectVectors(IK, image.get_body2ned(), image.get_cam2body(), grid_list)
            ned, _ypr, _quat = image.get_camera_pose()
            neds.append(list(ned))
            rays.append(np.array([np.asarray(x, np.float64).flatten() for x in proj_list]))
        rec = run_scene(srtm, 'mid', axis_n, axis_e, grid, np.array(neds, np.float64), np.array(rays, np.float64))
        # the module's own list call, as render_panda3d.py:205 makes it
        srtm.ned_interp = scipy.interpolate.RegularGridInterpolator((axis_n, axis_e), grid, bounds_error=False,
                                                                    fill_value=-32768)
        for i, name in enumerate(group):
            with contextlib.redirect_stdout(io.StringIO()):
                p = np.array(srtm.interpolate_vectors(neds[i], list(rays[i])), np.float64)
            assert np.array_equal(p, rec['pts'][i], equal_nan=True)
        poses = [im.get_camera_pose(opt=False) for im in proj.image_list]
        rec.update(names=[im.name for im in proj.image_list], group=list(group), poses=poses, width=width,
                   height=height, K=list(np.array(camera.get_K(False)).ravel()), dist=list(inp['dist']),
                   grid_steps=grid_steps, axis_n=axis_n, axis_e=axis_e, grid=grid)
        dump('mid', rec)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    if not os.path.isfile(os.path.join(REF, 'lib', 'srtm.py')):
        sys.exit('set IAMX_REFERENCE to the reference checkout (the directory holding scripts/)')
    srtm = import_reference_srtm()
    what = sys.argv[1:] or ['tiles', 'rays', 'mid']
    case = None
    if 'tiles' in what:
        case = tile_goldens(srtm)
        query_goldens(srtm, case)
    if 'rays' in what:
        ray_goldens(srtm)
    if 'mid' in what:
        mid_golden(srtm)


if __name__ == '__main__':
    main()
