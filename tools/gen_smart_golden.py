#!/usr/bin/env python3
"""Goldens of the 'smart' strategy from the reference's OWN scripts/lib/matcher.smart_pair_matches and
find_matches(strategy='smart').

Needs a checkout of the reference project, given by the IAMX_REFERENCE environment variable (the
directory that holds its scripts/).  For every case of tests/smart_reference.py the reference's
function runs on its own lib.image.Image objects (des_list float32, kp_list of cv2.KeyPoint with the
case's sizes, the case's camera poses, camera 5472 x 3648) under oracle/shims, with these stand-ins
made here:

  the_matcher.knnMatch(k = 3)      exact brute force (ties to the lowest train row), DMatch.distance
                                   = float32(sqrt(d2)); a train image of two rows gives two
  cv2.findHomography(.., 0)        the restated least-squares fit (smart_reference.fit)
  cv2.findHomography(.., RANSAC, tol)
                                   the float64 restatement of this package's rule
                                   (tests/verify_reference.consensus, seed 0), then the restated fit on
                                   its inliers (the consensus model where that fit fails)
  cv2.perspectiveTransform         as restated (smart_reference.transform)

so the Python-level rules -- the pose prior, the walk over three neighbours, bins, gates, the strict
`>`, the pass loop, filter_duplicates -- are the reference's own, and the consensus and the refit are
this package's (parity with cv2 is UNPINNED).

tests/golden/smart_<case>.pkl.gz: the inputs, reproj and H0 of the prior, per pass and per bin members
/ fit / unique as the reference PRINTS them, the taken bins, the pass count, the final lists and the
smallest margins.  smart_prior_edges: the prior alone at its corners.  smart_strip: the pair loop on
the inputs of tests/golden/find_matches_strip.pkl (read, not duplicated) with seeded keypoint sizes.

A case is refused unless every decision of every pass keeps its outcome when every raw_dist moves by
+- BAND_PX (the bin tests and the metric comparisons between a row's candidates), no size_diff is
within 1e-9 of 1.25 and no ratio within 1e-9 of match_ratio unless the quotient is exact, and the
consensus checks of gen_ratio_golden.check_bin hold: goldens never sit on a decision.

    IAMX_REFERENCE=<reference checkout> python tools/gen_smart_golden.py [case ...]
"""
import contextlib
import gzip
import io
import os
import pickle
import re
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.path.join(os.environ.get('IAMX_REFERENCE', ''), 'scripts')
GOLD = os.path.join(REPO, 'tests', 'golden')
BAND_PX = 0.01                  # 20 float32 ulps of a pixel coordinate (2^-11 at 4096 .. 8191)
STRIP_HYPOTHESES = 2048         # what matcher.smart_matches runs with by default
STRIP_SIZE_SEED = 101           # seeds 100 .. 147 were tried: 101, 113, 115 and 141 are not refused, 101 by the widest margin


class Refused(Exception):
    pass


def check_walk(log, match_ratio):
    """the refusal rule on the decisions smart_reference.walk() logged; -> smallest margins"""
    m = dict(ratio=np.inf, size=np.inf, metric=np.inf, bin=np.inf)
    cut = np.asarray([32, 64, 128, 256, 512, 1024, 2048], np.float64)
    for e in log:
        if e[0] == 'ratio':
            d = abs(e[1] - match_ratio)
            if d != 0.0:                                   # (an exact quotient: 150 / 200)
                m['ratio'] = min(m['ratio'], d)
        elif e[0] == 'size':
            d = abs(e[1] - 1.25)
            if not (e[2] and d == 0.0):
                m['size'] = min(m['size'], d)
        elif e[0] == 'bin':
            m['bin'] = min(m['bin'], float(np.abs(cut - e[1]).min()))
        elif e[0] == 'row':
            cands, pick = e[1], e[2]
            hi = (cands[pick][0] + BAND_PX) * cands[pick][1]
            for k, (raw, f) in enumerate(cands):
                if k != pick:
                    m['metric'] = min(m['metric'], (raw - BAND_PX) * f - hi)
    if m['ratio'] < 1e-9 or m['size'] < 1e-9:
        raise Refused('a ratio or a size quotient within 1e-9 of its threshold')
    if m['bin'] <= BAND_PX:
        raise Refused('a best_dist within BAND_PX of a cutoff')
    if m['metric'] <= 0:
        raise Refused("a row's choice depends on raw_dist inside the band")
    return m


def main():
    if not os.path.isdir(os.path.join(REF, 'lib')):
        sys.exit('IAMX_REFERENCE must name a checkout of the reference project')
    sys.dont_write_bytecode = True
    sys.path[:0] = [HERE, os.path.join(REPO, 'tests')]
    import gen_mre_golden as mre                     # (paths: oracle/shims, the reference, its archive)
    mre.setup_paths()
    import cv2                                      # the shim of oracle/shims
    from props import getNode
    from lib import camera, matcher
    from lib import image as ref_image
    from lib import smart as ref_smart
    import gen_ratio_golden as grg
    import smart_reference as sr
    import verify_reference as vr

    class Exact(object):
        def knnMatch(self, des1, des2, k=2):
            assert k == 3
            idx, d2 = sr.knn3_exact(np.asarray(des1), np.asarray(des2))
            dist = np.sqrt(d2.astype(np.float64)).astype(np.float32)
            return [[cv2.DMatch(q, int(i[j]), d[j]) for j in range(3) if i[j] >= 0]
                    for q, (i, d) in enumerate(zip(idx, dist))]

    state = dict(hyp=sr.HYPOTHESES, cons=[], reproj=[], H0=[])

    def find_homography(src, dst, method=0, tol=None):
        pts = np.concatenate([np.asarray(src, np.float32).reshape(-1, 2),
                              np.asarray(dst, np.float32).reshape(-1, 2)], axis=1)
        if method == 0:
            H, st = sr.fit(pts)
            assert st == sr.FIT_OK
            state['H0'].append(H)
            return H, np.ones((len(pts), 1), np.uint8)
        assert method == cv2.RANSAC
        c = vr.consensus(pts, float(tol), vr.HOMOGRAPHY, state['hyp'], sr.SEED)
        c['points'] = pts
        state['cons'].append(c)
        if c['status'] != vr.OK:
            return None, np.zeros((len(pts), 1), np.uint8)
        h = c['best'][0]
        with np.errstate(invalid='ignore'):
            mask = c['err'][h] <= c['tol2']
        H, st = sr.fit(pts, mask)
        if st != sr.FIT_OK:
            H = c['models64'][h].reshape(3, 3)
        return H, mask.astype(np.uint8).reshape(-1, 1)

    real_project = cv2.projectPoints

    def project_points(*a):
        out = real_project(*a)
        state['reproj'].append(np.asarray(out[0], np.float64).reshape(-1, 2).copy())
        return out

    cv2.findHomography = find_homography
    cv2.projectPoints = project_points
    cv2.perspectiveTransform = lambda src, H: sr.transform(H, np.asarray(src, np.float32).reshape(-1, 2)).reshape(-1, 1, 2)
    tmp = tempfile.mkdtemp(prefix='iamx_smart_golden_')
    os.makedirs(os.path.join(tmp, 'meta'), exist_ok=True)
    quiet = lambda out=None: contextlib.redirect_stdout(out if out is not None else io.StringIO())

    def setup(min_pairs, match_ratio=sr.MATCH_RATIO):
        for n_ in list(getNode('/images', True).__dict__):
            del getNode('/images', True).__dict__[n_]
        ref_smart.smart_node.__dict__.clear()
        camera.set_K(vr.KMAT[0, 0], vr.KMAT[1, 1], vr.KMAT[0, 2], vr.KMAT[1, 2])
        camera.set_dist_coeffs([0.0, 0.0, 0.0, 0.0, 0.0])
        camera.set_image_params(sr.W_PX, sr.H_PX)
        camera.set_mount_params(0.0, -90.0, 0.0)
        getNode('/config/detector', True).setString('detector', 'SIFT')
        getNode('/config/detector', True).setFloat('scale', 0.4)
        mnode = getNode('/config/matcher', True)
        mnode.__dict__.pop('ground_m', None)
        mnode.setFloat('match_ratio', match_ratio)
        mnode.setInt('min_pairs', int(min_pairs))
        with quiet():
            matcher.configure()
        matcher.the_matcher = Exact()
        return mnode

    def images(pose, names=('A', 'B')):
        out = []
        for k, n_ in enumerate(names):
            im = ref_image.Image(tmp, n_)
            im.set_camera_pose(pose['ned%d' % (k + 1)], *pose['ypr%d' % (k + 1)])
            im.match_list = {}
            node = ref_smart.smart_node.getChild(n_, True)
            node.setFloat('srtm_surface_m', pose['srtm'][k])
            if pose['yaw_error'][k] != 0.0:
                node.setFloat('yaw_error', pose['yaw_error'][k])
            out.append(im)
        if pose['forced_ground'] is not None:
            getNode('/config/matcher', True).setFloat('ground_m', pose['forced_ground'])
        return out

    def attach(im, des, xy, size):
        im.des_list = None if des is None else np.asarray(des).astype(np.float32)
        im.kp_list = [cv2.KeyPoint(float(x), float(y), float(s)) for (x, y), s in zip(xy, size)]

    def parse(text):
        """per pass: stats [7, 3] as printed, and 1 + the last bin with a 'Filtered matches' line"""
        passes, cur = [], -1
        for line in text.splitlines():
            if line.startswith('collect stats'):
                passes.append(dict(stats=np.full((7, 3), -1, np.int32), taken=0))
            m = re.match(r'bin: (\d+) cutoff: \S+ len: (\d+)', line)
            if m:
                cur = int(m.group(1))
                passes[-1]['stats'][cur, 0] = int(m.group(2))
            m = re.match(r' fit: (\d+) unique: (\d+)', line)
            if m:
                passes[-1]['stats'][cur, 1:] = [int(m.group(1)), int(m.group(2))]
            if line.startswith('Filtered matches:'):
                passes[-1]['taken'] = cur + 1
        return passes

    def dump(name, gold):
        path = os.path.join(GOLD, 'smart_%s.pkl.gz' % name)
        with gzip.GzipFile(path, 'wb', mtime=0) as f:
            pickle.dump(gold, f, protocol=4)
        size = os.path.getsize(path)
        print('  ->', os.path.relpath(path, REPO), size, 'bytes')
        assert size < 1000000

    want = set(sys.argv[1:])
    arr = lambda l: np.asarray(l, np.int32).reshape(-1, 2)
    # ---- the pair cases -------------------------------------------------------------------
    for name in sr.ALL_CASES:
        if want and name not in want:
            continue
        inp = sr.case(name)
        results, pairs_out = [], []
        for k, p in enumerate(inp['pairs']):
            setup(inp['min_pairs'])
            pose = sr.case_poses(name, k)
            i1, i2 = images(pose)
            attach(i1, p['des1'], p['xy1'], p['size1'])
            attach(i2, p['des2'], p['xy2'], p['size2'])
            for key in ('cons', 'reproj', 'H0'):
                del state[key][:]
            out, raised = io.StringIO(), None
            try:
                with quiet(out):
                    fwd, rev = matcher.smart_pair_matches(i1, i2, False, True)
            except ZeroDivisionError as exc:
                fwd, rev, raised = [], [], str(exc)
            passes = parse(out.getvalue())
            H0, reproj = np.asarray(state['H0'][0], np.float64), state['reproj'][0]
            Hld, _s = sr.fit(np.concatenate([reproj.astype(np.float32), _grid(sr).astype(np.float32)], axis=1),
                             dtype=np.longdouble)
            pin = dict(p, H0=H0)
            pairs_out.append(dict(pin, pose=pose))
            # the restatement replays the reference's decisions, with a log to read the margins from
            wlog, clog = [], []
            one = dict(inp, pairs=[pin])
            margin = {}
            guarded = p['des1'] is None or p['des2'] is None or len(p['des1']) <= 1 or len(p['des2']) <= 1
            if raised is None:
                res = sr.restate(one, sr.host_ransac(state['hyp'], sr.SEED, clog), log=wlog)[0]
                assert np.array_equal(res['fwd'], arr(fwd)) and np.array_equal(res['rev'], arr(rev)), name
                if guarded:                      # (the reference walks one pass over no matches at all)
                    assert len(passes) == 1 and (passes[0]['stats'][:, 0] == 0).all() and not res['passes']
                    passes = []
                assert len(res['passes']) == len(passes), (name, len(res['passes']), len(passes))
                for a, b in zip(res['passes'], passes):
                    assert np.array_equal(a['stats'], b['stats']) and a['taken'] == b['taken'], (name, a['stats'], b['stats'])
                try:
                    margin = check_walk(wlog, inp['match_ratio'])
                    margin['consensus'] = min([grg.check_bin(c, vr) for c in state['cons']] + [np.inf])
                except (Refused, grg.Refused) as exc:
                    sys.exit('case %s refused: %s' % (name, exc))
            results.append(dict(fwd=arr(fwd), rev=arr(rev), passes=passes, raised=raised, reproj=reproj,
                                H0=H0, margin=margin, bins_run=len(state['cons']),
                                prior_noise=sr.transfer_error(H0, Hld, reproj)))
            print('%-10s rows %4s x %4s  passes %d  taken %s  unique %s  result %d%s  margins %s'
                  % (name, 'None' if p['des1'] is None else len(p['des1']), 'None' if p['des2'] is None else len(p['des2']),
                     len(passes), [q['taken'] for q in passes], [int(q['stats'][:, 2].max()) for q in passes],
                     len(fwd), ' RAISED' if raised else '',
                     {k_: float('%.3g' % v) for k_, v in margin.items()}))
        dump(name, dict(inp, pairs=pairs_out, hypotheses=state['hyp'], seed=sr.SEED, cutoffs=list(sr.CUTOFFS),
                        tol=sr.tolerance(sr.W_PX, sr.H_PX), band_px=BAND_PX, results=results))
    # ---- the prior at its corners ----------------------------------------------------------
    if not want or 'prior_edges' in want:
        edges = []
        for what, pose in sr.prior_edges():
            setup(25)
            i1, i2 = images(pose)
            attach(i1, None, [], [])
            attach(i2, None, [], [])
            for key in ('cons', 'reproj', 'H0'):
                del state[key][:]
            with quiet():
                assert matcher.smart_pair_matches(i1, i2, False, True) == ([], [])
            reproj, H0 = state['reproj'][0], np.asarray(state['H0'][0], np.float64)
            pts = np.concatenate([reproj.astype(np.float32), _grid(sr).astype(np.float32)], axis=1)
            Hld, _s = sr.fit(pts, dtype=np.longdouble)
            noise = sr.transfer_error(H0, Hld, reproj)
            edges.append(dict(what=what, pose=pose, reproj=reproj, H0=H0, noise=noise))
            print('prior_edges %-36s reproj x %.1f .. %.1f  fit noise %.3g px' % (what, reproj[:, 0].min(), reproj[:, 0].max(), noise))
        dump('prior_edges', dict(edges=edges, width=sr.W_PX, height=sr.H_PX, K=vr.KMAT.copy()))
    # ---- the pair loop on the strip ---------------------------------------------------------
    if not want or 'smart_strip' in want:
        strip(locals())
    shutil.rmtree(tmp, ignore_errors=True)


def _grid(sr):
    return np.array([[u, v] for v in np.linspace(0, sr.H_PX, 9) for u in np.linspace(0, sr.W_PX, 9)], np.float64)


def strip(env):
    """find_matches(strategy='smart') on the inputs of find_matches_strip.pkl: sort False and True,
    a second call each; match lists, the /smart tree and the pose records as
    test_find_matches_loop.check_against compares them"""
    cv2, camera, matcher, getNode = env['cv2'], env['camera'], env['matcher'], env['getNode']
    ref_image, ref_smart, state, quiet, Exact = env['ref_image'], env['ref_smart'], env['state'], env['quiet'], env['Exact']
    from transformations import euler_from_quaternion, quaternion_multiply
    with open(os.path.join(GOLD, 'find_matches_strip.pkl'), 'rb') as f:
        g = pickle.load(f)
    rng = np.random.default_rng(STRIP_SIZE_SEED)
    sizes = [(np.round(rng.uniform(2.0, 3.2, len(x)) * 64) / 64).astype(np.float32) for x in g['xy']]
    state['hyp'] = STRIP_HYPOTHESES

    def tree(node):
        out = {}
        for k, v in node.__dict__.items():
            out[k] = tree(v) if hasattr(v, 'getChild') else (list(v) if isinstance(v, list) else v)
        return out

    def pose_record(im):
        ac = im.node.getChild('aircraft_pose', True)
        cp = im.node.getChild('camera_pose', True)
        return dict(yaw_error_deg=ac.getFloat('yaw_error_deg') if ac.hasChild('yaw_error_deg') else None,
                    aircraft_quat=[ac.getFloatEnum('quat', k) for k in range(4)],
                    camera_ypr=[cp.getFloat('yaw_deg'), cp.getFloat('pitch_deg'), cp.getFloat('roll_deg')],
                    camera_quat=[cp.getFloatEnum('quat', k) for k in range(4)])

    class Proj(object):
        pass

    # every pair the loop reaches -- both sort orders, both calls -- is replayed through the restatement
    # with a log, from the H0 the reference's own prior produced, and goes through the refusal rule
    sr = env['sr']
    walk = dict(ratio=np.inf, size=np.inf, metric=np.inf, bin=np.inf, pairs=0, decisions=0)
    ref_pair = matcher.smart_pair_matches

    def checked_pair(i1, i2, review=False, est_rotation=False):
        n0 = len(state['H0'])
        fwd, rev = ref_pair(i1, i2, review, est_rotation)
        xy = [np.float32([kp.pt for kp in im.kp_list]).reshape(-1, 2) for im in (i1, i2)]
        size = [np.float32([kp.size for kp in im.kp_list]) for im in (i1, i2)]
        idx, d2 = sr.knn3_exact(np.asarray(i1.des_list), np.asarray(i2.des_list))
        wlog = []
        res = sr.smart_pair(idx, d2, xy[0], xy[1], size[0], size[1], len(xy[0]), len(xy[1]), state['H0'][n0],
                            sr.tolerance(g['width'], g['height']), g['min_pairs'],
                            sr.host_ransac(STRIP_HYPOTHESES, 0, lean=True), g['match_ratio'], log=wlog)
        assert np.array_equal(res['fwd'], np.asarray(fwd, np.int32).reshape(-1, 2)), (i1.name, i2.name)
        try:
            m = check_walk(wlog, g['match_ratio'])
        except Refused as exc:
            sys.exit('smart_strip refused at %s vs %s (choose another STRIP_SIZE_SEED): %s' % (i1.name, i2.name, exc))
        for k, v in m.items():
            walk[k] = min(walk[k], v)
        walk['pairs'] += 1
        walk['decisions'] += len(wlog)
        return fwd, rev

    matcher.smart_pair_matches = checked_pair
    runs = {}
    for sort in (False, True):
        for n_ in list(getNode('/images', True).__dict__):
            del getNode('/images', True).__dict__[n_]
        ref_smart.smart_node.__dict__.clear()
        K = g['K']
        camera.set_K(K[0], K[4], K[2], K[5])
        camera.set_dist_coeffs([0.0, 0.0, 0.0, 0.0, 0.0])
        camera.set_image_params(g['width'], g['height'])
        camera.set_mount_params(*g['mount'])
        getNode('/config/detector', True).setString('detector', 'SIFT')
        getNode('/config/detector', True).setFloat('scale', 0.4)
        mnode = getNode('/config/matcher', True)
        mnode.__dict__.pop('ground_m', None)
        mnode.setFloat('match_ratio', g['match_ratio'])
        mnode.setInt('min_pairs', g['min_pairs'])
        with quiet():
            matcher.configure()
        matcher.the_matcher = Exact()
        tmp = tempfile.mkdtemp(prefix='iamx_smart_strip_')
        os.makedirs(os.path.join(tmp, 'meta'), exist_ok=True)
        proj = Proj()
        proj.analysis_dir = tmp
        proj.image_list = [ref_image.Image(tmp, n_) for n_ in g['names']]
        body2cam = camera.get_body2cam()
        for i, im in enumerate(proj.image_list):
            rep = g['reported'][i]
            im.set_aircraft_pose(*g['aircraft_lla'], *rep['ypr'])
            ned2body = [im.node.getChild('aircraft_pose').getFloatEnum('quat', k) for k in range(4)]
            y, p, r = euler_from_quaternion(quaternion_multiply(ned2body, body2cam), 'rzyx')
            im.set_camera_pose(rep['ned'], y * 180.0 / np.pi, p * 180.0 / np.pi, r * 180.0 / np.pi)
            im.des_list = g['des'][i].astype(np.float32)
            im.kp_list = [cv2.KeyPoint(float(x), float(y_), float(s)) for (x, y_), s in zip(g['xy'][i], sizes[i])]
            im.match_list = {}
            ref_smart.smart_node.getChild(im.name, True).setFloat('srtm_surface_m', g['ground'])
        calls = []
        for call in range(2):
            del state['cons'][:]
            with quiet():
                matcher.find_matches(proj, np.array(K).reshape(3, 3), strategy='smart', sort=sort)
            try:
                margin = min([env['grg'].check_bin(c, env['vr']) for c in state['cons']] + [np.inf])
            except env['grg'].Refused as exc:
                sys.exit('smart_strip refused (choose another STRIP_SIZE_SEED): %s' % exc)
            print('   smallest consensus margin %.3g' % margin)
            calls.append(dict(
                match_lists=[{k: [list(map(int, p_)) for p_ in v] for k, v in im.match_list.items()}
                             for im in proj.image_list],
                smart=pickle.loads(pickle.dumps(tree(ref_smart.smart_node))),
                poses=[pose_record(im) for im in proj.image_list], bins_run=len(state['cons'])))
            ml = calls[-1]['match_lists']
            print('smart_strip sort=%s call %d: %d pairs, %d with matches, %d consensus calls'
                  % (sort, call, sum(len(m) for m in ml) // 2, sum(1 for m in ml for v in m.values() if len(v)) // 2,
                     len(state['cons'])))
        runs[bool(sort)] = dict(calls=calls)
        shutil.rmtree(tmp, ignore_errors=True)
    matcher.smart_pair_matches = ref_pair
    print('   %d pairs replayed, %d logged decisions, smallest margins %s'
          % (walk['pairs'], walk['decisions'], {k: float('%.3g' % walk[k]) for k in ('ratio', 'size', 'metric', 'bin')}))
    path = os.path.join(GOLD, 'smart_strip.pkl.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        pickle.dump(dict(sizes=sizes, size_seed=STRIP_SIZE_SEED, hypotheses=STRIP_HYPOTHESES, seed=0,
                         srtm_surface_m=g['ground'], runs=runs, band_px=BAND_PX, margin=walk), f, protocol=4)
    size = os.path.getsize(path)
    print('  ->', os.path.relpath(path, REPO), size, 'bytes')
    assert size < 1000000


if __name__ == '__main__':
    main()
