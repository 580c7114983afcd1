#!/usr/bin/env python3
"""Goldens of the cull step (scripts/4b-mre-by-image.py) from the reference's OWN scripts.

Needs a checkout of the reference project, given by the IAMX_REFERENCE environment variable
(the directory that holds its scripts/).  For the ba_mid and ba_dist scenes of tests/golden/ba_*_in.pkl:

  1. a reference ProjectMgr project in a temporary directory (meta/*.json, config.json,
     groups.json, matches_grouped), a deterministic few percent of the observations displaced
     by 20-200 px and one chain given a second observation from an image it already has;
  2. the reference's scripts/4a-optimize.py, then for each case its scripts/4b-mre-by-image.py,
     both through runpy with builtins.input patched to 'y' (oracle/shims on the path for
     props / cv2, as oracle/check_dropin.py does);
  3. tests/golden/mre_<scene>_<case>.pkl.gz: the matches_grouped 4b read (bytes), groups, image
     names, initial and optimized poses, K / distortion (initial and optimized), the captured
     stdout, the marked (match, feature) list in marking order, the matches_grouped bytes 4b
     wrote, and the smallest relative distance of any decision value from its threshold.

    IAMX_REFERENCE=<reference checkout> python tools/gen_mre_golden.py
"""
import builtins
import contextlib
import gzip
import io
import os
import pickle
import runpy
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.path.join(os.environ.get('IAMX_REFERENCE', ''), 'scripts')
GOLD = os.path.join(REPO, 'tests', 'golden')

CASES = {
    'default': [],
    'sd2max8': ['--stddev', '2', '--max', '8'],
    'strong': ['--strong'],
    'initial': ['--initial-pose'],
}
SCENES = ('mid', 'dist')


def setup_paths():
    sys.path[:0] = [os.path.join(REPO, 'oracle', 'shims'), REF, REPO]
    sys.path.append(os.path.join(REF, 'lib', 'archive'))
    import transformations as _tf

    class _Numpy1Compat(object):
        """the archived transformations.py means numpy 1.x's array(copy=False)"""
        def __getattr__(self, k):
            return getattr(np, k)

        @staticmethod
        def array(obj, *a, **k):
            if k.get('copy', True) is False:
                k.pop('copy')
                return np.asarray(obj, *a, **k)
            return np.array(obj, *a, **k)
    _tf.numpy = _Numpy1Compat()


def perturb(matches, seed):
    """displace ~4 % of the observations by 20-200 px, duplicate one member of one chain"""
    rng = np.random.default_rng(seed)
    flat = [(i, j) for i, m in enumerate(matches) for j in range(2, len(m))]
    pick = rng.choice(len(flat), max(3, len(flat) * 4 // 100), replace=False)
    for k in sorted(pick.tolist()):
        i, j = flat[k]
        ang = rng.uniform(0, 2 * np.pi)
        r = rng.uniform(20, 200)
        u, v = matches[i][j][1]
        matches[i][j][1] = [float(u + r * np.cos(ang)), float(v + r * np.sin(ang))]
    # a chain with two observations from the same image (the second displaced by 60 px)
    i = int(rng.integers(0, len(matches)))
    img, (u, v) = matches[i][2]
    matches[i].append([img, [float(u + 60.0), float(v - 35.0)]])
    return i


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
    matches = pickle.loads(pickle.dumps(inp['matches']))
    dup = perturb(matches, 11 if scene == 'mid' else 12)
    groups.save(proj.analysis_dir, inp['groups'])
    with open(os.path.join(proj.analysis_dir, 'matches_grouped'), 'wb') as f:
        pickle.dump(matches, f)
    return inp, dup


def run_script(name, argv):
    old_argv, old_input = sys.argv, builtins.input
    sys.argv = [name] + argv
    builtins.input = lambda prompt='': (print(prompt, end=''), 'y')[1]
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            runpy.run_path(os.path.join(REF, name), run_name='__main__')
    finally:
        sys.argv, builtins.input = old_argv, old_input
    return out.getvalue()


def poses(directory, opt):
    from lib import project
    with contextlib.redirect_stdout(io.StringIO()):
        p = project.ProjectMgr(directory)
        p.load_images_info()
    return [im.get_camera_pose(opt=opt) for im in p.image_list]


def main():
    if not os.path.isfile(os.path.join(REF, '4b-mre-by-image.py')):
        sys.exit('set IAMX_REFERENCE to the reference checkout (the directory holding scripts/)')
    setup_paths()
    from lib import camera
    from lib import match_culling as ref_cull
    from lib import optimizer as ref_opt
    work = tempfile.mkdtemp(prefix='iamx_mre_golden_')
    try:
        for scene in SCENES:
            base = os.path.join(work, scene)
            inp, dup = build_project(scene, base)
            run_script('4a-optimize.py', [base])
            matches_in = open(os.path.join(base, 'ImageAnalysis', 'matches_grouped'), 'rb').read()
            camera_state = dict(K=list(camera.get_K(False).ravel()), K_opt=list(camera.get_K(True).ravel()),
                                dist=list(camera.get_dist_coeffs(False)),
                                dist_opt=list(camera.get_dist_coeffs(True)))
            for case, argv in CASES.items():
                d = os.path.join(work, '%s_%s' % (scene, case))
                shutil.copytree(base, d)
                marked, errors = [], []
                orig_mark, orig_fun = ref_cull.mark_feature, ref_opt.Optimizer.fun

                def spy_mark(matches, mi, fi, e, _orig=orig_mark):
                    marked.append((int(mi), int(fi)))
                    return _orig(matches, mi, fi, e)

                def spy_fun(self, *a, _orig=orig_fun):
                    r = _orig(self, *a)
                    errors.append(np.array(r, np.float64))
                    return r
                ref_cull.mark_feature, ref_opt.Optimizer.fun = spy_mark, spy_fun
                try:
                    stdout = run_script('4b-mre-by-image.py', [d] + argv)
                finally:
                    ref_cull.mark_feature, ref_opt.Optimizer.fun = orig_mark, orig_fun
                matches_out = open(os.path.join(d, 'ImageAnalysis', 'matches_grouped'), 'rb').read()
                # decision margins: mark threshold (and --max), the report's mre + 3 std rule
                r = errors[-1]
                e = np.sqrt(r[0::2] * r[0::2] + r[1::2] * r[1::2])
                mre_e = np.sum(np.sort(e)) / len(e)
                sd = np.sqrt(np.sum((mre_e - e) ** 2) / len(e))
                trim = float(argv[argv.index('--stddev') + 1]) if '--stddev' in argv else 5.0
                margins = [np.min(np.abs(e - (mre_e + sd * trim))) / (mre_e + sd * trim)]
                if '--max' in argv:
                    mx = float(argv[argv.index('--max') + 1])
                    margins.append(np.min(np.abs(e - mx)) / mx)
                rep_thr = np.mean(np.abs(r)) + 3 * np.std(r)
                cam_means = [float(l.split(' - mean: ')[1].split()[0]) for l in stdout.splitlines()
                             if ' - mean: ' in l]
                rec = dict(scene=scene, case=case, argv=argv, names=list(inp['names']),
                           groups=inp['groups'], width=inp['width'], height=inp['height'],
                           poses=poses(d, False), poses_opt=poses(d, True), camera=camera_state,
                           matches_in=matches_in, dup_chain=dup, stdout=stdout, marked=marked,
                           matches_out=matches_out, n_obs=len(e),
                           margin=float(min(margins)), report_threshold=float(rep_thr),
                           n_report=len(cam_means))
                path = os.path.join(GOLD, 'mre_%s_%s.pkl.gz' % (scene, case))
                with gzip.GzipFile(path, 'wb', mtime=0) as f:
                    pickle.dump(rec, f, protocol=4)
                print('%-28s obs=%d marked=%d margin=%.3g bytes=%d' % (
                    os.path.basename(path), len(e), len(marked), rec['margin'], os.path.getsize(path)))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == '__main__':
    main()
