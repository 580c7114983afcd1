#!/usr/bin/env python3
"""Goldens of the 'bruteforce' strategy from the reference's OWN
scripts/lib/matcher.bruteforce_pair_matches and find_matches(strategy='bruteforce').

Needs a checkout of the reference project, given by the IAMX_REFERENCE environment variable (the
directory that holds its scripts/).  For every case of tests/brute_reference.py the reference's
function runs on image stand-ins (des_list float32, kp_list of cv2.KeyPoint with the case's sizes,
camera 5472 x 3648, the matcher nodes, matcher.configure()) under oracle/shims, with two stand-ins
made here:

  the_matcher.knnMatch(k = 3)      exact brute force (ties to the lowest train row), DMatch.distance
                                   = float32(sqrt(d2)); a train image of two rows gives two
  cv2.findHomography(.., RANSAC, tol)
                                   the float64 restatement of this package's rule
                                   (tests/verify_reference.consensus) at 256 hypotheses, seed 0

so the Python-level rules -- guards, the walk over three neighbours, the 41 x 21 cells and their
wraps, the gate, the strict `>` on fitted inliers, the early exit, filter_duplicates -- are the
reference's own and the consensus is this package's (parity with cv2 is UNPINNED).

tests/golden/brute_<case>.pkl.gz: the inputs, per pair the forward and reverse lists and what the
reference PRINTS -- per distance bin walked (bin, len, best fitted, best of bin), per taken cell
(filtered, fitted) -- with, in the order of the walk, every findHomography call (members, fitted) and
which of them were taken, and the smallest margins.  brute_strip: the pair loop on the inputs of
tests/golden/find_matches_strip.pkl (read, not duplicated) with seeded keypoint sizes.

A case is refused unless, for every cell the reference hands to findHomography, the checks of
gen_ratio_golden.check_bin hold; for every chosen row, the float32 and the float64 distance quotient
round to the same bin and neither raw_dist / step_d nor vangle / step_a lies within 1e-6 of a
half-integer; no size_diff is within 1e-9 of 1.25 and no ratio within 1e-9 of match_ratio unless the
quotient is exact; and no two metrics of a row are closer than 1e-12 unless they are equal: goldens
never sit on a decision, and they hold under either NumPy.

    IAMX_REFERENCE=<reference checkout> python tools/gen_brute_golden.py [case ...]
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
STRIP_HYPOTHESES = 256
STRIP_SIZE_SEED = 101
HALF = 1e-6


class Refused(Exception):
    pass


def check_choices(log, match_ratio, step_d, step_a):
    """the refusal rule on the decisions brute_reference.choose() logged; -> smallest margins"""
    m = dict(ratio=np.inf, size=np.inf, metric=np.inf, dbin=np.inf, abin=np.inf)
    for e in log:
        if e[0] == 'ratio':
            d = abs(e[1] - match_ratio)
            if d != 0.0:                                   # (an exact quotient: 150 / 200)
                m['ratio'] = min(m['ratio'], d)
        elif e[0] == 'size':
            d = abs(e[1] - 1.25)
            if not (e[2] and d == 0.0):
                m['size'] = min(m['size'], d)
        elif e[0] == 'row':
            cands, pick = e[1], e[2]
            for k, c in enumerate(cands):
                if k != pick and c != cands[pick]:         # (equal metrics: the strict `<` decides, exactly)
                    m['metric'] = min(m['metric'], abs(c - cands[pick]))
        elif e[0] == 'choice':
            _q, _t, raw, vangle = e[1:]
            x64 = float(raw) / step_d
            x32 = float(np.float32(raw) / np.float32(step_d))
            if int(round(x64)) != int(round(x32)):
                raise Refused('the float32 and the float64 distance quotient round to different bins')
            for key, x in (('dbin', x64), ('dbin', x32), ('abin', vangle / step_a)):
                m[key] = min(m[key], abs(x - np.floor(x) - 0.5))
    if m['ratio'] < 1e-9 or m['size'] < 1e-9:
        raise Refused('a ratio or a size quotient within 1e-9 of its threshold')
    if m['metric'] < 1e-12:
        raise Refused("a row's choice lies between two metrics closer than 1e-12")
    if m['dbin'] <= HALF or m['abin'] <= HALF:
        raise Refused('a bin quotient within 1e-6 of a half-integer')
    return m


def parse(text):
    """what the reference printed for one pair -> dict(lines [(position, the bin number printed, len,
    best, best_of_bin)] -- the number printed is not the bin after a taken cell, see
    brute_reference.walk_cells --, calls
    [(members, fitted)] in walk order, taken: positions in calls, filtered [(filtered, fitted)])"""
    out = dict(lines=[], calls=[], taken=[], filtered=[])
    for line in text.splitlines():
        m = re.match(r'bin: (\d+) len: (\d+) (\d+) (\d+)$', line)
        if m:
            out['lines'].append((len(out['lines']),) + tuple(int(v) for v in m.groups()))
        m = re.match(r'CALL (\d+) (\d+)$', line)
        if m:
            out['calls'].append((int(m.group(1)), int(m.group(2))))
        m = re.match(r'Filtered matches: (\d+) Fitted matches: (\d+)$', line)
        if m:
            out['taken'].append(len(out['calls']) - 1)
            out['filtered'].append((int(m.group(1)), int(m.group(2))))
    return out


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
    import brute_reference as br
    import gen_ratio_golden as grg
    import verify_reference as vr

    class Exact(object):
        def knnMatch(self, des1, des2, k=2):
            assert k == 3
            idx, d2 = br.knn3_exact(np.asarray(des1), np.asarray(des2))
            dist = np.sqrt(d2.astype(np.float64)).astype(np.float32)
            return [[cv2.DMatch(q, int(i[j]), d[j]) for j in range(3) if i[j] >= 0]
                    for q, (i, d) in enumerate(zip(idx, dist))]

    class Image(object):
        def __init__(self, name, des, xy, size):
            self.name = name
            self.des_list = None if des is None else np.asarray(des).astype(np.float32)
            self.kp_list = [cv2.KeyPoint(float(x), float(y), float(s)) for (x, y), s in zip(xy, size)]
            self.match_list = {}

    state = dict(hyp=br.HYPOTHESES, cons=[])

    def find_homography(src, dst, method, tol):
        assert method == cv2.RANSAC
        pts = np.concatenate([np.asarray(src, np.float32).reshape(-1, 2),
                              np.asarray(dst, np.float32).reshape(-1, 2)], axis=1)
        if len(pts) < 4:
            # (min_pairs < 4: cv2 itself raises on fewer than four points.  The package does not look at
            #  such a cell; to the walk that is a cell without inliers -- 0 is never above the best, and
            #  leaves best_of_bin as it is -- so the stand-in answers that, and records no call)
            return None, np.zeros((len(pts), 1), np.uint8)
        c = vr.consensus(pts, float(tol), vr.HOMOGRAPHY, state['hyp'], br.SEED)
        c['points'] = pts
        state['cons'].append(c)
        if c['status'] != vr.OK:
            print('CALL %d 0' % len(pts))
            return None, np.zeros((len(pts), 1), np.uint8)
        h = c['best'][0]
        with np.errstate(invalid='ignore'):
            mask = c['err'][h] <= c['tol2']
        print('CALL %d %d' % (len(pts), int(mask.sum())))       # (into the text parse() reads)
        return c['models64'][h].reshape(3, 3), mask.astype(np.uint8).reshape(-1, 1)

    cv2.findHomography = find_homography
    quiet = lambda out=None: contextlib.redirect_stdout(out if out is not None else io.StringIO())

    def setup(min_pairs, match_ratio, w, h):
        getNode('/config/detector', True).setString('detector', 'SIFT')
        getNode('/config/detector', True).setFloat('scale', 0.4)
        mnode = getNode('/config/matcher', True)
        mnode.setFloat('match_ratio', match_ratio)
        mnode.setInt('min_pairs', int(min_pairs))
        camera.set_image_params(int(w), int(h))
        with quiet():
            matcher.configure()
        matcher.the_matcher = Exact()

    def dump(name, gold):
        path = os.path.join(GOLD, 'brute_%s.pkl.gz' % name)
        with gzip.GzipFile(path, 'wb', mtime=0) as f:
            pickle.dump(gold, f, protocol=4)
        size = os.path.getsize(path)
        print('  ->', os.path.relpath(path, REPO), size, 'bytes')
        assert size <= 120000                        # (no larger than the ratio_* / smart_* goldens)

    want = set(sys.argv[1:])
    arr = lambda l: np.asarray(l, np.int32).reshape(-1, 2)
    for name in br.ALL_CASES:
        if want and name not in want:
            continue
        inp = br.case(name)
        w, h = int(inp['width']), int(inp['height'])
        step_d = br.step_dist(w, h)
        results = []
        for p in inp['pairs']:
            setup(p['min_pairs'], inp['match_ratio'], w, h)
            i1, i2 = Image('A', p['des1'], p['xy1'], p['size1']), Image('B', p['des2'], p['xy2'], p['size2'])
            del state['cons'][:]
            out, raised = io.StringIO(), None
            try:
                with quiet(out):
                    fwd, rev = matcher.bruteforce_pair_matches(i1, i2)
            except ZeroDivisionError as exc:
                fwd, rev, raised = [], [], str(exc)
            printed = parse(out.getvalue())
            margin = {}
            if raised is None:
                # the restatement replays the reference's decisions, with a log to read the margins from
                wlog = []
                res = br.restate(dict(inp, pairs=[p]), br.host_ransac(state['hyp'], br.SEED), log=wlog)[0]
                assert np.array_equal(res['fwd'], arr(fwd)) and np.array_equal(res['rev'], arr(rev)), name
                assert res['calls'] == printed['calls'] and res['taken'] == printed['taken'], name
                if p['des1'] is None or p['des2'] is None or len(p['des1']) <= 1 or len(p['des2']) <= 1:
                    # (under raw_matches' guards the reference walks its 41 bins over no matches at all)
                    assert len(printed['lines']) == br.ND and all(l[2:] == (0, 0, 0) for l in printed['lines'])
                    printed['lines'] = []
                assert res['lines'] == printed['lines'], (name, res['lines'], printed['lines'])
                try:
                    margin = check_choices(wlog, inp['match_ratio'], step_d, br.STEP_A)
                    margin['consensus'] = min([grg.check_bin(c, vr) for c in state['cons']] + [np.inf])
                except (Refused, grg.Refused) as exc:
                    sys.exit('case %s refused: %s' % (name, exc))
            results.append(dict(printed, fwd=arr(fwd), rev=arr(rev), raised=raised, margin=margin))
            print('%-9s rows %4s x %4s  walked %2d  calls %3d  taken %s  result %d%s  margins %s'
                  % (name, 'None' if p['des1'] is None else len(p['des1']),
                     'None' if p['des2'] is None else len(p['des2']), len(printed['lines']), len(printed['calls']),
                     printed['filtered'], len(fwd), ' RAISED' if raised else '',
                     {k_: float('%.3g' % v) for k_, v in margin.items()}))
        dump(name, dict(inp, hypotheses=state['hyp'], seed=br.SEED, tol=br.tolerance(w, h), step_d=step_d,
                        results=results))
    if not want or 'strip' in want:
        strip(locals())


def strip(env):
    """find_matches(strategy='bruteforce') on the inputs of find_matches_strip.pkl: sort False and
    True, a second call each; match lists, the /smart tree and the pose records as
    test_find_matches_loop.check_against compares them"""
    cv2, camera, matcher, getNode = env['cv2'], env['camera'], env['matcher'], env['getNode']
    state, quiet, Exact, br, grg, vr = env['state'], env['quiet'], env['Exact'], env['br'], env['grg'], env['vr']
    from lib import image as ref_image
    from lib import smart as ref_smart
    from transformations import euler_from_quaternion, quaternion_multiply
    with open(os.path.join(GOLD, 'find_matches_strip.pkl'), 'rb') as f:
        g = pickle.load(f)
    rng = np.random.default_rng(STRIP_SIZE_SEED)
    sizes = [(np.round(rng.uniform(2.0, 3.2, len(x)) * 64) / 64).astype(np.float32) for x in g['xy']]
    state['hyp'] = STRIP_HYPOTHESES
    step_d, tol = br.step_dist(g['width'], g['height']), br.tolerance(g['width'], g['height'])

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

    # every pair the loop reaches is replayed through the restatement with a log and goes through the
    # refusal rule
    walk = dict(ratio=np.inf, size=np.inf, metric=np.inf, dbin=np.inf, abin=np.inf, pairs=0)
    ref_pair = matcher.bruteforce_pair_matches

    def checked_pair(i1, i2, review=False):
        fwd, rev = ref_pair(i1, i2, review)
        xy = [np.float32([kp.pt for kp in im.kp_list]).reshape(-1, 2) for im in (i1, i2)]
        size = [np.float32([kp.size for kp in im.kp_list]) for im in (i1, i2)]
        idx, d2 = br.knn3_exact(np.asarray(i1.des_list), np.asarray(i2.des_list))
        wlog = []
        res = br.brute_pair(idx, d2, xy[0], xy[1], size[0], size[1], len(xy[0]), len(xy[1]), tol, g['min_pairs'],
                            br.host_ransac(STRIP_HYPOTHESES, 0, lean=True), g['match_ratio'], step_d, log=wlog)
        assert np.array_equal(res['fwd'], np.asarray(fwd, np.int32).reshape(-1, 2)), (i1.name, i2.name)
        try:
            m = check_choices(wlog, g['match_ratio'], step_d, br.STEP_A)
        except Refused as exc:
            sys.exit('brute_strip refused at %s vs %s (choose another STRIP_SIZE_SEED): %s' % (i1.name, i2.name, exc))
        for k, v in m.items():
            walk[k] = min(walk[k], v)
        walk['pairs'] += 1
        return fwd, rev

    matcher.bruteforce_pair_matches = checked_pair
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
        tmp = tempfile.mkdtemp(prefix='iamx_brute_strip_')
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
                matcher.find_matches(proj, np.array(K).reshape(3, 3), strategy='bruteforce', sort=sort)
            try:
                margin = min([grg.check_bin(c, vr) for c in state['cons']] + [np.inf])
            except grg.Refused as exc:
                sys.exit('brute_strip refused (choose another STRIP_SIZE_SEED): %s' % exc)
            print('   smallest consensus margin %.3g' % margin)
            calls.append(dict(
                match_lists=[{k: [list(map(int, p_)) for p_ in v] for k, v in im.match_list.items()}
                             for im in proj.image_list],
                smart=pickle.loads(pickle.dumps(tree(ref_smart.smart_node))),
                poses=[pose_record(im) for im in proj.image_list], cells_run=len(state['cons'])))
            ml = calls[-1]['match_lists']
            print('brute_strip sort=%s call %d: %d pairs, %d with matches, %d consensus calls'
                  % (sort, call, sum(len(m) for m in ml) // 2, sum(1 for m in ml for v in m.values() if len(v)) // 2,
                     len(state['cons'])))
        runs[bool(sort)] = dict(calls=calls)
        shutil.rmtree(tmp, ignore_errors=True)
    matcher.bruteforce_pair_matches = ref_pair
    print('   %d pairs replayed, smallest margins %s'
          % (walk['pairs'], {k: float('%.3g' % walk[k]) for k in ('ratio', 'size', 'metric', 'dbin', 'abin')}))
    path = os.path.join(GOLD, 'brute_strip.pkl.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        pickle.dump(dict(sizes=sizes, size_seed=STRIP_SIZE_SEED, hypotheses=STRIP_HYPOTHESES, seed=0,
                         srtm_surface_m=g['ground'], runs=runs, margin=walk), f, protocol=4)
    size = os.path.getsize(path)
    print('  ->', os.path.relpath(path, REPO), size, 'bytes')
    assert size <= 120000


if __name__ == '__main__':
    main()
