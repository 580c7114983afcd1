#!/usr/bin/env python3
"""Goldens of the two chain tools run between optimiser passes, from the reference's OWN scripts:
scripts/3c-match-triangulation.py --method triangulate and scripts/4b-colocated-feats.py.

Needs a checkout of the reference project, given by the IAMX_REFERENCE environment variable (the
directory that holds its scripts/).  For the ba_mid and ba_dist scenes of tests/golden/ba_*_in.pkl:

  1. a reference ProjectMgr project in a temporary directory (as tools/gen_step5_golden.py makes
     it), then the reference's scripts/4a-optimize.py: optimised poses, optimised K / distortion and
     the refitted matches_grouped.  Group 1 has two images, which the reference's optimiser does not
     take; its images get a camera_pose_opt here (the initial pose displaced by up to 0.8 m and 0.4
     degrees, deterministic), so that the --group 1 cases work on poses and not on zeros;
  2. per case the reference's script through runpy with builtins.input patched to 'y'.  Two things
     are supplied for these runs, and nothing else is changed:
       * builtins.math -- 4b-colocated-feats.py never imports math, so its compute_angle() lands in
         its own bare `except` and answers 0 for every pair (4c-colocated-cams.py carries the same
         function with acos imported: the intent is not in doubt);
       * cv2.undistortPoints on the imported shim module, taken from tests/undistort_restatement.py
         (cv2 is not installed; parity with cv2 itself is unpinned);
  3. tests/golden/chain_<tool>_<scene>_<case>.pkl.gz: the inputs (names, groups, both kinds of poses,
     both kinds of K / distortion, the matches_grouped bytes read), the matches_grouped bytes written
     (None when the script did not write), the mark list in marking order (a spy on
     match_culling.mark_feature), stdout with the temporary directory written as <project>, and
       triangulate: per written chain cond_2(r) of the 3x3 system (a spy on line_solver's solve) and
                    the smallest |x[2]| / max(1, |x|) (the "WHOA!" decision);
       colocated:   the smallest |angle - min_angle| / min_angle over all pairs looked at.

Cases -- triangulate: default, group1 (--group 1).  colocated: default (1 degree, nothing marked,
file not rewritten), close (three camera_pose_opt positions moved to within 0.3-1.5 m of a
neighbour; at least one chain deleted, one chain that keeps >= min_chain_len members after losing
one, one member marked more than once -- asserted), wide (--min-angle 12), group1 (--group 1
--min-angle 12).

A case whose smallest margin is below 1e-6 is refused: goldens never sit on a decision.

    IAMX_REFERENCE=<reference checkout> python tools/gen_chain_tools_golden.py
"""
import builtins
import contextlib
import gzip
import io
import math
import os
import pickle
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_mre_golden as mre                                     # noqa: E402  (paths, run_script)
import gen_step5_golden as step5                                 # noqa: E402  (build_project)

GOLD = mre.GOLD
SCENES = ('mid', 'dist')
MIN_MARGIN = 1e-6
TRI_CASES = {'default': [], 'group1': ['--group', '1']}
COLO_CASES = {'default': [], 'close': [], 'wide': ['--min-angle', '12'],
              'group1': ['--group', '1', '--min-angle', '12']}
# the close case: (image moved, the neighbour it lands next to, offset in metres) by position in group 0
CLOSE = ((3, 2, (0.25, -0.15, 0.05)), (4, 2, (-0.6, 0.7, -0.1)), (9, 8, (1.1, 0.8, 0.3)))


def _arg(argv, name, default, kind):
    return kind(argv[argv.index(name) + 1]) if name in argv else default


def _load_project(d):
    from lib import project
    with contextlib.redirect_stdout(io.StringIO()):
        proj = project.ProjectMgr(d)
        proj.load_images_info()
    return proj


def give_group1_poses(d):
    from lib import groups
    proj = _load_project(d)
    rng = np.random.default_rng(41)
    for name in groups.load(proj.analysis_dir)[1]:
        im = proj.findImageByName(name)
        ned, ypr, _q = im.get_camera_pose(opt=False)
        ned = [float(v + o) for v, o in zip(ned, rng.uniform(-0.8, 0.8, 3))]
        ypr = [float(v + o) for v, o in zip(ypr, rng.uniform(-0.4, 0.4, 3))]
        im.set_camera_pose(ned, ypr[0], ypr[1], ypr[2], opt=True)
    proj.save_images_info()


def _record(scene, case, argv, d, matches_in):
    from lib import camera, groups
    proj = _load_project(d)
    width, height = camera.get_image_params()
    return dict(scene=scene, case=case, argv=argv, names=[im.name for im in proj.image_list],
                groups=groups.load(proj.analysis_dir), width=width, height=height,
                poses=[im.get_camera_pose(opt=False) for im in proj.image_list],
                poses_opt=[im.get_camera_pose(opt=True) for im in proj.image_list],
                camera=dict(K=list(camera.get_K(False).ravel()), K_opt=list(camera.get_K(True).ravel()),
                            dist=list(camera.get_dist_coeffs(False)),
                            dist_opt=list(camera.get_dist_coeffs(True))),
                matches_in=matches_in)


def _write(rec, tool):
    if rec['margin'] < MIN_MARGIN:
        sys.exit('%s %s/%s sits on a decision: margin %g' % (tool, rec['scene'], rec['case'], rec['margin']))
    path = os.path.join(GOLD, 'chain_%s_%s_%s.pkl.gz' % (tool, rec['scene'], rec['case']))
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        pickle.dump(rec, f, protocol=4)
    return path


def run_triangulate(scene, case, argv, base, work):
    from lib import line_solver
    d = os.path.join(work, '%s_tri_%s' % (scene, case))
    shutil.copytree(base, d)
    mpath = os.path.join(d, 'ImageAnalysis', 'matches_grouped')
    matches_in = open(mpath, 'rb').read()
    rec = _record(scene, case, argv, d, matches_in)
    conds = []
    orig = line_solver.solve

    def spy_solve(r, q):
        conds.append(float(np.linalg.cond(np.asarray(r, np.float64), 2)))
        return orig(r, q)
    line_solver.solve = spy_solve
    try:
        stdout = mre.run_script('3c-match-triangulation.py', [d, '--method', 'triangulate'] + argv)
    finally:
        line_solver.solve = orig
    written = [int(l.split()[0]) for l in stdout.splitlines() if '>>>' in l]
    assert len(written) == len(conds)
    out = pickle.load(open(mpath, 'rb'))
    whoa = sum('WHOA!' in l for l in stdout.splitlines())
    x = np.array([out[i][0] for i in written], np.float64).reshape(-1, 3)
    margin = float(np.min(np.abs(x[:, 2]) / np.maximum(1.0, np.linalg.norm(x, axis=1)))) if len(x) else 1.0
    rec.update(matches_out=open(mpath, 'rb').read(), stdout=stdout.replace(d, '<project>'),
               written=written, cond=conds, n_whoa=int(whoa), margin=margin)
    path = _write(rec, 'triangulate')
    print('%-40s written=%d whoa=%d max cond=%.3g margin=%.3g bytes=%d' % (
        os.path.basename(path), len(written), whoa, max(conds) if conds else 0, margin, os.path.getsize(path)))


def _angles(proj, group_list, group_index, matches):
    """every angle 4b-colocated-feats.py looks at, by its compute_angle with math supplied"""
    out = []
    names = group_list[group_index]
    for k, match in enumerate(matches):
        if match[1] != group_index:
            continue
        for i, m1 in enumerate(match[2:]):
            for j, m2 in enumerate(match[2:]):
                if i < j:
                    i1, i2 = proj.image_list[m1[0]], proj.image_list[m2[0]]
                    if i1.name in names and i2.name in names:
                        ned1 = i1.get_camera_pose(opt=True)[0]
                        ned2 = i2.get_camera_pose(opt=True)[0]
                        v1 = np.array(match[0]) - np.array(ned1)
                        v2 = np.array(match[0]) - np.array(ned2)
                        tmp = np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2))
                        out.append((k, i, j, math.acos(min(tmp, 1.0)) * 180.0 / math.pi))
    return out


def run_colocated(scene, case, argv, base, work):
    from lib import match_culling as ref_cull
    d = os.path.join(work, '%s_colo_%s' % (scene, case))
    shutil.copytree(base, d)
    if case == 'close':
        from lib import groups
        proj = _load_project(d)
        in_group = [proj.findImageByName(n) for n in groups.load(proj.analysis_dir)[0]]
        for k, near, off in CLOSE:
            ned, ypr, _q = in_group[k].get_camera_pose(opt=True)
            target = in_group[near].get_camera_pose(opt=True)[0]
            ned = [target[0] + off[0], target[1] + off[1], target[2] + off[2]]
            in_group[k].set_camera_pose(ned, ypr[0], ypr[1], ypr[2], opt=True)
        proj.save_images_info()
    mpath = os.path.join(d, 'ImageAnalysis', 'matches_grouped')
    matches_in = open(mpath, 'rb').read()
    stamp = os.stat(mpath).st_mtime_ns
    rec = _record(scene, case, argv, d, matches_in)
    marked = []
    orig_mark = ref_cull.mark_feature

    def spy_mark(matches, mi, fi, e, _orig=orig_mark):
        marked.append((int(mi), int(fi)))
        return _orig(matches, mi, fi, e)
    ref_cull.mark_feature = spy_mark
    had_math = hasattr(builtins, 'math')
    builtins.math = math
    try:
        stdout = mre.run_script('4b-colocated-feats.py', [d] + argv)
    finally:
        ref_cull.mark_feature = orig_mark
        if not had_math:
            del builtins.math
    rewritten = os.stat(mpath).st_mtime_ns != stamp or open(mpath, 'rb').read() != matches_in
    group_index = _arg(argv, '--group', 0, int)
    min_angle = _arg(argv, '--min-angle', 1.0, float)
    proj = _load_project(d)
    angles = _angles(proj, rec['groups'], group_index, pickle.loads(matches_in))
    assert [(k, i) for k, i, _j, a in angles if a < min_angle] == marked
    margin = min([abs(a - min_angle) / min_angle for _k, _i, _j, a in angles] or [1.0])
    min_chain_len = 3
    n_in, n_out = len(pickle.loads(matches_in)), len(pickle.load(open(mpath, 'rb')))
    if case == 'default':
        assert not marked and not rewritten
    if case == 'close':
        before = pickle.loads(matches_in)
        per_chain = {}
        for k, i in marked:
            per_chain.setdefault(k, set()).add(i)
        assert n_out < n_in, 'no chain deleted'
        assert any(len(before[k]) - 2 - len(s) >= min_chain_len for k, s in per_chain.items()), \
            'no chain survives a lost member'
        assert len(set(marked)) < len(marked), 'no member marked more than once'
    rec.update(matches_out=open(mpath, 'rb').read() if rewritten else None,
               stdout=stdout.replace(d, '<project>'), marked=marked, min_angle=min_angle,
               group_index=group_index, min_chain_len=min_chain_len, n_pairs=len(angles),
               margin=float(margin))
    path = _write(rec, 'colocated')
    print('%-40s pairs=%d marked=%d chains %d -> %d margin=%.3g bytes=%d' % (
        os.path.basename(path), len(angles), len(marked), n_in, n_out, margin, os.path.getsize(path)))


def main():
    if not os.path.isfile(os.path.join(mre.REF, '4b-colocated-feats.py')):
        sys.exit('set IAMX_REFERENCE to the reference checkout (the directory holding scripts/)')
    mre.setup_paths()
    sys.path.insert(0, os.path.join(mre.REPO, 'tests'))
    import cv2                                                   # the shim (oracle/shims)
    import undistort_restatement
    had = hasattr(cv2, 'undistortPoints')
    assert not had, 'a cv2 with undistortPoints of its own: these goldens pin the restatement'
    cv2.undistortPoints = undistort_restatement.cv2_undistortPoints
    work = tempfile.mkdtemp(prefix='iamx_chain_golden_')
    try:
        for scene in SCENES:
            base = os.path.join(work, scene)
            step5.build_project(scene, base)
            mre.run_script('4a-optimize.py', [base])
            give_group1_poses(base)
            for case, argv in TRI_CASES.items():
                run_triangulate(scene, case, argv, base, work)
            for case, argv in COLO_CASES.items():
                run_colocated(scene, case, argv, base, work)
    finally:
        del cv2.undistortPoints
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
