"""The cull step on the device: iamx_ba_reproj_stats / iamx_ba_mark_outliers against numpy on the
f64 residual of iamx_ba_residual, then mre_by_image + mark_outliers + delete_marked_features and the
4b-mre-by-image.py twin against the reference's own runs (tests/golden/mre_*.pkl.gz,
tools/gen_mre_golden.py)."""
import contextlib
import glob
import gzip
import io
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
CASES = sorted(glob.glob(os.path.join(GOLD, 'mre_*.pkl.gz')))
CALIB = np.array([3666.6665, 3666.6665, 2736.0, 1824.0, -0.1, 0.05, 0.001, -0.002, 0.01])


# ---------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------
def _problem(counts, n_pts, seed, outliers=0.02):
    rng = np.random.default_rng(seed)
    C = len(counts)
    cams = np.zeros((C, 7))
    cams[:, :3] = rng.normal(0, 20, (C, 3)) + [0, 0, -100]
    cams[:, 3:] = [0.7071, 0, -0.7071, 0] + rng.normal(0, 0.02, (C, 4))
    pts = rng.normal(0, 30, (n_pts, 3))
    ci = np.repeat(np.arange(C), counts).astype(np.int32)
    O = ci.size
    pi = rng.integers(0, n_pts, O).astype(np.int32)
    uv = rng.uniform(0, 4000, (max(O, 1), 2))[:O]
    return cams, pts, ci, pi, uv


def _run(cams, pts, ci, pi, uv, counts, trim, max_error):
    import torch
    from imageanalysis_amd import kernels
    dev = torch.device('cuda:0')
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (cams, pts, ci, pi, uv, CALIB)]
    ptr = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=ptr[1:])
    r = kernels.ba_residual(*t)
    cs, summ, e = kernels.ba_reproj_stats(*t, torch.from_numpy(ptr).to(dev))
    idx, esel = kernels.ba_mark_outliers(e, summ, trim, max_error)
    torch.cuda.synchronize()
    s = summ.cpu().numpy()
    n = int(s[kernels.REPROJ_COUNT])
    return dict(r=r.cpu().numpy(), cam=cs.cpu().numpy(), summary=s, e=e.cpu().numpy(),
                idx=idx[:n].cpu().numpy(), esel=esel[:n].cpu().numpy())


def _check(counts, n_pts=500, seed=0, trim=2.0, max_error=None):
    from imageanalysis_amd import kernels as K
    counts = np.asarray(counts, np.int64)
    prob = _problem(counts, n_pts, seed)
    a = _run(*prob, counts, trim, max_error)
    b = _run(*prob, counts, trim, max_error)
    for k in a:                                                   # run to run: identical bits
        assert a[k].tobytes() == b[k].tobytes(), k
    r, e, s = a['r'], a['e'], a['summary']
    O = counts.sum()
    du, dv = r[0::2], r[1::2]
    assert np.array_equal(e, np.sqrt(du * du + dv * dv))          # separately rounded, as numpy
    ref = np.array([np.linalg.norm(r[2 * o:2 * o + 2]) for o in range(min(O, 4000))])
    assert np.all(np.abs(e[:len(ref)] - ref) <= np.spacing(ref))  # np.linalg.norm: within 1 ulp
    ptr = np.concatenate([[0], np.cumsum(counts)])
    for c in range(len(counts)):
        seg = e[ptr[c]:ptr[c + 1]]
        assert a['cam'][c, 2] == len(seg)
        if len(seg):
            m = np.mean(np.abs(seg))
            assert abs(a['cam'][c, 0] - m) <= 1e-13 * m
            assert a['cam'][c, 1] == np.amax(seg)
        else:
            assert a['cam'][c, 0] == 0 and a['cam'][c, 1] == 0     # count 0: the flag
    close = lambda x, y, tol: abs(x - y) <= tol * abs(y)          # noqa: E731
    assert s[K.REPROJ_N] == O and s[K.REPROJ_EMPTY_CAMS] == np.sum(counts == 0)
    assert close(s[K.REPROJ_MEAN_ABS_R], np.mean(np.abs(r)), 1e-12)
    assert close(s[K.REPROJ_STD_R], np.std(r), 1e-12)
    assert s[K.REPROJ_MAX_ABS_R] == np.amax(np.abs(r))
    assert close(s[K.REPROJ_SUM_E], np.sum(e), 1e-12)
    mre = np.sum(e) / O
    sd = np.sqrt(np.sum((mre - e) ** 2) / O)
    assert close(s[K.REPROJ_STDDEV_E], sd, 1e-12)
    thr = s[K.REPROJ_THRESHOLD]
    assert close(thr, mre + sd * trim, 1e-12)
    flag = e > thr
    if max_error is not None:
        flag |= e > max_error
    assert np.array_equal(a['idx'], np.nonzero(flag)[0]) and s[K.REPROJ_COUNT] == flag.sum()
    assert np.array_equal(a['esel'], e[a['idx']])
    # and the numpy threshold decides the same (no value within 1e-9 of it in these problems)
    want = e > mre + sd * trim
    if max_error is not None:
        want |= e > max_error
    assert np.array_equal(flag, want)
    return a


def test_one_observation():
    _check([0, 1, 0], n_pts=3)


def test_odd_with_empty_cameras_leading_and_trailing():
    a = _check([0, 0, 37, 1, 0, 255, 256, 257, 3, 0, 0], max_error=3000.0)
    assert a['summary'][7] == 5


def test_single_camera_holds_everything():
    _check([20001], n_pts=3000, trim=1.0)


def test_configs3_size():
    rng = np.random.default_rng(5)
    counts = rng.multinomial(1_960_000, np.ones(2812) / 2812)
    counts[[0, 17, 2811]] = 0
    _check(counts, n_pts=400_000, seed=3, trim=1.5)


# ---------------------------------------------------------------------------------------------
# end to end on the reference's runs
# ---------------------------------------------------------------------------------------------
def _load(path):
    with gzip.open(path, 'rb') as f:
        return pickle.load(f)


def _project(g):
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd.hostlib import camera
    from imageanalysis_amd.hostlib.image_pose import PoseProject
    proj = PoseProject(g['names'])
    for im, p0, p1 in zip(proj.image_list, g['poses'], g['poses_opt']):
        for opt, (ned, ypr, quat) in ((False, p0), (True, p1)):
            im.set_camera_pose(ned, ypr[0], ypr[1], ypr[2], opt=opt)
            node = im.node.getChild('camera_pose_opt' if opt else 'camera_pose', True)
            for i in range(4):                  # the reference's stored quaternion, bit for bit
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


def _trim(g):
    a = g['argv']
    return (float(a[a.index('--stddev') + 1]) if '--stddev' in a else 5.0,
            float(a[a.index('--max') + 1]) if '--max' in a else None)


def _outlier_lines(text):
    out = []
    for l in text.splitlines():
        if l.startswith('  outlier - match index:'):
            f = l.split()
            out.append((int(f[4]), int(f[7]), float(f[9])))
    return out


def _report_lines(text):
    lines = text.splitlines()
    # (the reference's Optimizer.fun prints an 'mre: ' line of its own first: the last one is 4b's)
    keep = [[l for l in lines if l.startswith('mre: ')][-1]] + \
        [l for l in lines if ' - mean: ' in l or l.startswith('mre = ')]
    i = lines.index("Report of images that aren't fitting well:")
    names = lines[i + 1 + sum(' - mean: ' in l for l in lines)]
    return keep, names


@pytest.mark.parametrize('path', CASES, ids=os.path.basename)
def test_cull_matches_reference(path):
    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd import optimizer
    g = _load(path)
    assert g['margin'] > 1e-9
    proj = _project(g)
    matches = pickle.loads(g['matches_in'])
    trim, mx = _trim(g)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        opt = optimizer.Optimizer('/nonexistent')
        opt.setup(proj, g['groups'], 0, matches, optimized='--initial-pose' not in g['argv'])
        rep = cull.mre_by_image(opt, matches, proj=proj)
        print('mre: %.3f std: %.3f max: %.2f' % (rep.mre, rep.std, rep.max))
        print("Report of images that aren't fitting well:")
        worst = [l for l in rep.by_cam if l[0] > rep.mre + 3 * rep.std]
        for l in worst:
            print("%s - mean: %.3f max: %.3f" % (l[2], l[0], l[1]))
        print(''.join(l[2] + ' ' for l in worst))
        n = cull.mark_outliers(matches, rep, trim, max_error=mx)
        if n:
            cull.delete_marked_features(matches, 3, strong='--strong' in g['argv'])
    assert rep.n_error == 2 * g['n_obs']
    # marks: the same (match, feature) pairs in the same order
    ours, theirs = _outlier_lines(out.getvalue()), _outlier_lines(g['stdout'])
    assert [(m, f) for m, f, _ in ours] == [tuple(x) for x in g['marked']] == [(m, f) for m, f, _ in theirs]
    # the printed error is repr(float): our projection and the reference's cv2 path may round the
    # last digit differently, so the numbers are compared to 1e-9 relative
    for (_, _, a), (_, _, b) in zip(ours, theirs):
        assert abs(a - b) <= 1e-9 * b
    # the report: names and order exact, the 3-decimal numbers equal
    (k1, n1), (k2, n2) = _report_lines(out.getvalue()), _report_lines(g['stdout'])
    assert k1 == k2 and n1 == n2
    # the rewritten matches_grouped
    want = g['matches_out'] if g['marked'] else g['matches_in']
    assert pickle.dumps(matches) == want


LIB_STANDIN = {
    '__init__.py': '',
    'groups.py': textwrap.dedent('''\
        import json, os
        def load(path):
            return json.load(open(os.path.join(path, 'groups.json')))
        '''),
    'project.py': textwrap.dedent('''\
        import os, pickle, sys
        sys.path.insert(0, os.environ['IAMX_TEST_DIR'])
        from test_mre_cull_gpu import _project
        class ProjectMgr(object):
            """stand-in: the poses / camera of the golden record in the project directory"""
            def __init__(self, project_dir):
                self.analysis_dir = os.path.join(project_dir, 'ImageAnalysis')
                self._g = pickle.load(open(os.path.join(project_dir, 'record.pkl'), 'rb'))
            def load_images_info(self):
                p = _project(self._g)
                self.image_list = p.image_list
                self.findIndexByName = p.findIndexByName
        '''),
}


@pytest.mark.parametrize('path', [p for p in CASES if p.endswith(('mid_default.pkl.gz', 'dist_strong.pkl.gz'))],
                         ids=os.path.basename)
def test_twin_script_writes_reference_bytes(path, tmp_path):
    import json
    g = _load(path)
    lib = tmp_path / 'standin' / 'lib'
    lib.mkdir(parents=True)
    for name, text in LIB_STANDIN.items():
        (lib / name).write_text(text)
    proj = tmp_path / 'project'
    (proj / 'ImageAnalysis').mkdir(parents=True)
    (proj / 'ImageAnalysis' / 'matches_grouped').write_bytes(g['matches_in'])
    (proj / 'ImageAnalysis' / 'groups.json').write_text(json.dumps(g['groups']))
    rec = {k: v for k, v in g.items() if k not in ('matches_in', 'matches_out', 'stdout')}
    (proj / 'record.pkl').write_bytes(pickle.dumps(rec))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / 'standin'), REPO]),
               IAMX_TEST_DIR=os.path.dirname(os.path.abspath(__file__)))
    cmd = ['timeout', '-k', '10', '300', sys.executable,
           os.path.join(REPO, 'imageanalysis_amd', 'scripts', '4b-mre-by-image.py'), str(proj)] + g['argv']
    p = subprocess.run(cmd, input='y\n', capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Save these changes? (y/n):' in p.stdout
    assert (proj / 'ImageAnalysis' / 'matches_grouped').read_bytes() == g['matches_out']
    ours, theirs = _outlier_lines(p.stdout), _outlier_lines(g['stdout'])
    assert [x[:2] for x in ours] == [x[:2] for x in theirs]
