#!/usr/bin/env python3
"""Goldens of Step 5 ("Create the map") from the reference's OWN scripts/lib/render_panda3d.build_map.

Needs a checkout of the reference project, given by the IAMX_REFERENCE environment variable (the
directory that holds its scripts/).  For the ba_mid and ba_dist scenes of tests/golden/ba_*_in.pkl:

  1. a reference ProjectMgr project in a temporary directory (as tools/gen_mre_golden.py makes it,
     without the displaced observations), then the reference's scripts/4a-optimize.py: optimised
     poses, optimised K / distortion and the refitted matches_grouped;
  2. per case the reference's render_panda3d.build_map(proj, group_list, 0) with
     panda3d.make_textures_opencv patched out (cv2 is absent and the textures are not the subject),
     scipy.interpolate imported first (the reference's file forgets to) and
     scipy.interpolate.LinearNDInterpolator wrapped so that every query and result is logged per ray;
  3. tests/golden/step5_<scene>_<case>.pkl.gz: the inputs (names, groups, poses, camera, the
     matches_grouped bytes, the module switches), the surface.bin bytes, per image z_avg,
     distorted_uv and grid_list, every egg's bytes and the names removed, the logged look-ups, the
     captured stdout (the temporary directory written as <project>), and the smallest margins of the
     decision values against their thresholds.

Cases: default, noextrap (no_extrapolate), ground (force_ground_elevation_m), direct
(use_direct_pose), tilted (cameras pitched so that rays leave the hull and end below 30 degrees, one
camera above the horizon, one camera BELOW the surface -- intersect2d "always assumes the camera is
above ground": from below every downward ray ends at a negative angle, every vertex is NaN and the
egg is removed), outlier (one point moved beyond 10 std).

A scene whose smallest margin is below 1e-6 (relative to the threshold; in units of the printed
digit for the %.2f / %.5f coordinates) is refused: goldens never sit on a decision.

    IAMX_REFERENCE=<reference checkout> python tools/gen_step5_golden.py
"""
import contextlib
import gzip
import io
import os
import pickle
import shutil
import sys
import tempfile
from math import atan2, pi, sqrt

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_mre_golden as mre                                     # noqa: E402  (paths, run_script)

GOLD = mre.GOLD
SCENES = ('mid', 'dist')
CASES = ('default', 'noextrap', 'ground', 'direct', 'tilted', 'outlier')
MIN_MARGIN = 1e-6
# (image index in group 0, pitch_deg or None, ned[2] or None) of the tilted case
TILT = ((1, -52.0, None), (2, -44.0, None), (4, -61.0, None), (5, 38.0, None), (7, None, 21.5))


def build_project(scene, directory):
    from lib import camera, groups, project
    from lib import image as lib_image
    with open(os.path.join(GOLD, 'ba_%s_in.pkl' % scene), 'rb') as f:
        inp = pickle.load(f)
    with contextlib.redirect_stdout(io.StringIO()):
        proj = project.ProjectMgr(directory, create=True)
    K = inp['K']
    camera.set_K(K[0], K[4], K[2], K[5])
    camera.set_dist_coeffs(list(inp['dist']))
    camera.set_image_params(inp['width'], inp['height'])
    proj.image_list = [lib_image.Image(proj.analysis_dir, nm) for nm in inp['names']]
    for im, (ned, ypr, quat) in zip(proj.image_list, inp['poses']):
        im.set_camera_pose(ned, ypr[0], ypr[1], ypr[2])
    proj.save_images_info()
    proj.save()
    groups.save(proj.analysis_dir, inp['groups'])
    with open(os.path.join(proj.analysis_dir, 'matches_grouped'), 'wb') as f:
        pickle.dump(pickle.loads(pickle.dumps(inp['matches'])), f)
    return inp


class Margins(object):
    def __init__(self):
        self.m = {'error': np.inf, 'angle': np.inf, 'diff': np.inf, 'v2': np.inf, 'print': np.inf}

    def add(self, key, value):
        self.m[key] = min(self.m[key], float(value))


def ray_margins(raw, ned, v, avg_ground, no_extrapolate, mg):
    """intersect2d's decisions once more (on the unlogged interpolator), each value against its
    threshold; returns the number of rounds"""
    mg.add('v2', abs(v[2]))
    if v[2] <= 0.0:
        return 0
    p = list(ned)
    tmp = raw([p[1], p[0]])[0]
    surface = tmp if (no_extrapolate or not np.isnan(tmp)) else avg_ground
    error = abs(p[2] - surface)
    count = 0
    while True:
        if not np.isnan(error):
            mg.add('error', abs(error - 0.01) / 0.01)
        if not (error > 0.01 and count < 25):
            break
        d_proj = -(ned[2] - surface)
        factor = d_proj / v[2]
        p = [ned[0] + v[0] * factor, ned[1] + v[1] * factor, ned[2] + d_proj]
        tmp = raw([p[1], p[0]])[0]
        if no_extrapolate or not np.isnan(tmp):
            surface = tmp
        error = abs(p[2] - surface)
        count += 1
    dy, dx, dz = ned[0] - p[0], ned[1] - p[1], ned[2] - p[2]
    angle = atan2(-dz, sqrt(dx * dx + dy * dy)) * 180 / pi
    if not np.isnan(angle):
        mg.add('angle', abs(angle - 30.0) / 30.0)
    return count


def print_margin(values, digits, mg):
    """distance of every printed number from the rounding boundary of its last digit, in units of
    that digit (0.5 = as far as it gets)"""
    t = np.asarray(values, np.float64).ravel()
    t = t[~np.isnan(t)] * 10.0 ** digits
    if t.size:
        mg.add('print', np.min(np.abs(t - np.floor(t) - 0.5)))


def run_case(scene, case, base, work):
    import scipy.interpolate
    from lib import camera, groups, project
    from lib import panda3d as ref_panda3d
    from lib import render_panda3d as ref_render
    d = os.path.join(work, '%s_%s' % (scene, case))
    shutil.copytree(base, d)
    with contextlib.redirect_stdout(io.StringIO()):
        proj = project.ProjectMgr(d)
        proj.load_images_info()
    group_list = groups.load(proj.analysis_dir)
    mpath = os.path.join(proj.analysis_dir, 'matches_grouped')
    in_group = [proj.findImageByName(n) for n in group_list[0]]

    switches = dict(grid_steps=8, texture_resolution=512, use_direct_pose=False,
                    force_ground_elevation_m=None, use_srtm_surface=None, no_extrapolate=False)
    if case == 'noextrap':
        switches['no_extrapolate'] = True
    elif case == 'ground':
        switches['force_ground_elevation_m'] = 3.25
    elif case == 'direct':
        switches['use_direct_pose'] = True
    elif case == 'tilted':
        for k, pitch, down in TILT:
            im = in_group[k]
            ned, ypr, _q = im.get_camera_pose(opt=True)
            if pitch is not None:
                ypr[1] = pitch
            if down is not None:
                ned[2] = down
            im.set_camera_pose(ned, ypr[0], ypr[1], ypr[2], opt=True)
    elif case == 'outlier':
        matches = pickle.load(open(mpath, 'rb'))
        k = [i for i, m in enumerate(matches) if m[1] == 0][17]
        matches[k][0] = [matches[k][0][0], matches[k][0][1], matches[k][0][2] - 150.0]
        with open(mpath, 'wb') as f:
            pickle.dump(matches, f)
    matches_in = open(mpath, 'rb').read()
    poses = [im.get_camera_pose(opt=False) for im in proj.image_list]
    poses_opt = [im.get_camera_pose(opt=True) for im in proj.image_list]

    # the logging interpolator and the per-ray bookkeeping
    Orig = scipy.interpolate.LinearNDInterpolator
    state = {'raw': None, 'q': [], 'z': [], 'ray_ptr': [0], 'rays': []}

    class Logged(object):
        def __init__(self, tri, values):
            self.f = Orig(tri, values)
            state['raw'] = self.f

        def __call__(self, x):
            r = self.f(x)
            state['q'].append((float(x[0]), float(x[1])))
            state['z'].append(float(r[0]))
            return r

    orig_intersect = ref_render.intersect2d

    def spy_intersect(interp, ned, v, avg_ground):
        state['rays'].append((list(ned), np.array(v, np.float64), float(avg_ground)))
        r = orig_intersect(interp, ned, v, avg_ground)
        state['ray_ptr'].append(len(state['z']))
        return r

    saved = {k: getattr(ref_render, k) for k in switches}
    orig_tex = ref_panda3d.make_textures_opencv
    out = io.StringIO()
    try:
        for k, v in switches.items():
            setattr(ref_render, k, v)
        scipy.interpolate.LinearNDInterpolator = Logged
        ref_render.intersect2d = spy_intersect
        ref_panda3d.make_textures_opencv = lambda *a, **k: None
        with contextlib.redirect_stdout(out):
            ref_render.build_map(proj, group_list, 0)
    finally:
        scipy.interpolate.LinearNDInterpolator = Orig
        ref_render.intersect2d = orig_intersect
        ref_panda3d.make_textures_opencv = orig_tex
        for k, v in saved.items():
            setattr(ref_render, k, v)

    # margins
    mg = Margins()
    rounds = [ray_margins(state['raw'], ned, v, ag, switches['no_extrapolate'], mg)
              for ned, v, ag in state['rays']]
    ptr = np.array(state['ray_ptr'], np.int64)
    assert [int(b - a - 1) if b > a else 0 for a, b in zip(ptr[:-1], ptr[1:])] == rounds
    matches = pickle.loads(matches_in)
    z = np.array([m[0] for m in matches if m[1] == 0])[:, 2]
    avg, std = -np.mean(z), np.std(z)
    mg.add('diff', np.min(np.abs(np.abs(-z - avg) - 10 * std)) / (10 * std))
    width, height = camera.get_image_params()
    per_image = {}
    for im in in_group:
        grid = np.array(im.grid_list, np.float64)
        uv = np.array(im.distorted_uv, np.float64)
        print_margin(grid, 2, mg)
        print_margin(uv[:, 0] / float(width), 5, mg)
        print_margin(1.0 - uv[:, 1] / float(height), 5, mg)
        per_image[im.name] = dict(z_avg=im.z_avg, distorted_uv=uv, grid_list=grid)
    if switches['force_ground_elevation_m']:
        # (no interpolator: the only ray decision is the sign of v[2])
        from lib import project as ref_project
        IK = np.linalg.inv(camera.get_K(optimized=True))
        u = np.linspace(0, width, 9)
        v = np.linspace(0, height, 9)
        grid_uv = [[a, b] for b in v for a in u]
        for im in in_group:
            for vec in ref_project.projectVectors(IK, im.get_body2ned(opt=True), im.get_cam2body(), grid_uv):
                mg.add('v2', abs(vec[2]))

    models = os.path.join(proj.analysis_dir, 'models')
    eggs, removed = {}, []
    for im in in_group:
        name = os.path.splitext(im.name)[0] + '.egg'
        path = os.path.join(models, name)
        if os.path.exists(path):
            eggs[name] = open(path, 'rb').read()
        else:
            removed.append(name)
    rec = dict(scene=scene, case=case, switches=switches, names=[im.name for im in proj.image_list],
               groups=group_list, width=width, height=height, poses=poses, poses_opt=poses_opt,
               camera=dict(K=list(camera.get_K(False).ravel()), K_opt=list(camera.get_K(True).ravel()),
                           dist=list(camera.get_dist_coeffs(False)),
                           dist_opt=list(camera.get_dist_coeffs(True))),
               matches_in=matches_in,
               surface_bin=open(os.path.join(models, 'surface.bin'), 'rb').read(),
               images=per_image, eggs=eggs, removed=removed,
               lookups=dict(ray_ptr=ptr, q=np.array(state['q'], np.float64).reshape(-1, 2),
                            z=np.array(state['z'], np.float64),
                            ray_image=[im.name for im in in_group] if len(ptr) > 1 else []),
               stdout=out.getvalue().replace(d, '<project>'), margins=mg.m,
               margin=float(min(mg.m.values())))
    if rec['margin'] < MIN_MARGIN:
        sys.exit('%s/%s sits on a decision: margins %r' % (scene, case, mg.m))
    path = os.path.join(GOLD, 'step5_%s_%s.pkl.gz' % (scene, case))
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        pickle.dump(rec, f, protocol=4)
    nan_rays = int(sum(np.isnan(g['grid_list']).any(axis=1).sum() for g in per_image.values()))
    print('%-30s rays=%d look-ups=%d nan=%d removed=%d margin=%.3g (%s) bytes=%d' % (
        os.path.basename(path), len(state['rays']), len(state['z']), nan_rays, len(removed), rec['margin'],
        min(mg.m, key=mg.m.get), os.path.getsize(path)))


def main():
    if not os.path.isfile(os.path.join(mre.REF, 'lib', 'render_panda3d.py')):
        sys.exit('set IAMX_REFERENCE to the reference checkout (the directory holding scripts/)')
    mre.setup_paths()
    import scipy.interpolate                                     # noqa: F401  (render_panda3d.py forgets to)
    work = tempfile.mkdtemp(prefix='iamx_step5_golden_')
    try:
        for scene in SCENES:
            base = os.path.join(work, scene)
            build_project(scene, base)
            mre.run_script('4a-optimize.py', [base])
            for case in CASES:
                run_case(scene, case, base, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
