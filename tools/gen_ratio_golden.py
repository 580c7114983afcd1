#!/usr/bin/env python3
"""Goldens of the 'bestratio' strategy from the reference's OWN scripts/lib/matcher.ratio_pair_matches.

Needs a checkout of the reference project, given by the IAMX_REFERENCE environment variable (the
directory that holds its scripts/).  For every case of tests/ratio_reference.py the reference's
function runs on image stand-ins (des_list float32, kp_list of cv2.KeyPoint, as oracle/gen_golden.py
sets them up for G1: camera 5472 x 3648, the matcher nodes, matcher.configure()), with two stand-ins
made here:

  the_matcher.knnMatch        exact brute force (ties to the lowest train row), DMatch.distance =
                              float32(sqrt(d2))
  cv2.findHomography(.., RANSAC, tol)
                              the float64 restatement of this package's rule
                              (tests/verify_reference.consensus) at 256 hypotheses, seed 0

so the Python-level rules -- guards, ratio, bins, gates, the strict `>`, filter_duplicates -- are the
reference's own and the consensus is this package's (parity with cv2 is UNPINNED).

tests/golden/ratio_<case>.pkl.gz: the inputs, per pair the forward and reverse lists, per bin
members / fit / unique and the chosen bin as the reference PRINTS them, and the smallest margins.

A case is refused unless, for every bin the reference hands to findHomography, float64 and longdouble
agree on the winning hypothesis and on its mask and no error of the winning model lies within
verify_reference.BAND of tol^2: goldens never sit on a decision.

    IAMX_REFERENCE=<reference checkout> python tools/gen_ratio_golden.py
"""
import contextlib
import gzip
import io
import os
import pickle
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.path.join(os.environ.get('IAMX_REFERENCE', ''), 'scripts')
GOLD = os.path.join(REPO, 'tests', 'golden')


class Refused(Exception):
    pass


def check_bin(c, vr):
    """the refusal rule on one consensus dict; -> smallest relative distance of an error from tol^2"""
    if c['status'] != vr.OK:
        return np.inf
    h = c['best'][0]
    # the winner must win whatever side of tol^2 the errors inside the band fall on
    lower, upper = c['lower'], c['upper']
    if (upper[:h] >= lower[h]).any() or (upper[h + 1:] > lower[h]).any() or lower[h] != upper[h]:
        raise Refused('the winning hypothesis depends on errors inside the guard band')
    # ... and in longdouble: every model's errors under the longdouble model
    pts_n = c['err'].shape[1]
    eld = vr.errors(c['modelsld'], c['points'], vr.HOMOGRAPHY, np.longdouble)
    tld = np.longdouble(c['tol2'])
    ok = np.isfinite(c['modelsld'].astype(np.float64)).all(1)
    with np.errstate(invalid='ignore'):
        cnt = np.where(ok, (eld <= tld).sum(1), 0)
        if int(np.argmax(cnt)) != h:
            raise Refused('float64 and longdouble disagree on the winning hypothesis')
        if ((eld[h] <= tld) != (c['err'][h] <= c['tol2'])).any() or not c['stable']:
            raise Refused('float64 and longdouble disagree on the mask')
        rel = np.abs(c['err'][h] / c['tol2'] - 1.0)
    rel = rel[np.isfinite(rel)]
    assert len(c['err'][h]) == pts_n
    if (rel <= vr.BAND).any():
        raise Refused('an error within BAND of tol^2')
    return float(rel.min()) if len(rel) else np.inf


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
    import ratio_reference as rr
    import verify_reference as vr

    class Exact(object):
        def knnMatch(self, des1, des2, k=2):
            assert k == 2
            idx, d2 = rr.knn2_exact(np.asarray(des1), np.asarray(des2))
            dist = np.sqrt(d2.astype(np.float64)).astype(np.float32)
            return [[cv2.DMatch(q, int(i[0]), d[0]), cv2.DMatch(q, int(i[1]), d[1])]
                    for q, (i, d) in enumerate(zip(idx, dist))]

    class Image(object):
        def __init__(self, name, des, xy):
            self.name = name
            self.des_list = np.asarray(des).astype(np.float32)
            self.kp_list = [cv2.KeyPoint(float(x), float(y), 3.0) for x, y in xy]
            self.match_list = {}

    log = []

    def find_homography(src, dst, method, tol):
        assert method == cv2.RANSAC
        pts = np.concatenate([np.asarray(src, np.float32).reshape(-1, 2),
                              np.asarray(dst, np.float32).reshape(-1, 2)], axis=1)
        c = vr.consensus(pts, float(tol), vr.HOMOGRAPHY, rr.HYPOTHESES, rr.SEED)
        c['points'] = pts
        log.append(c)
        if c['status'] != vr.OK:
            return None, np.zeros((len(pts), 1), np.uint8)
        h = c['best'][0]
        with np.errstate(invalid='ignore'):
            mask = c['err'][h] <= c['tol2']
        return c['models64'][h].reshape(3, 3), mask.astype(np.uint8).reshape(-1, 1)

    cv2.findHomography = find_homography
    for name in rr.CASES:
        inp = rr.case(name)
        getNode('/config/detector', True).setString('detector', 'SIFT')
        getNode('/config/detector', True).setFloat('scale', 0.4)
        mnode = getNode('/config/matcher', True)
        mnode.setFloat('match_ratio', 0.75)
        mnode.setInt('min_pairs', int(inp['min_pairs']))
        camera.set_image_params(int(inp['width']), int(inp['height']))
        with contextlib.redirect_stdout(io.StringIO()):
            matcher.configure()
        matcher.the_matcher = Exact()
        results = []
        for p in inp['pairs']:
            i1, i2 = Image('A', p['des1'], p['xy1']), Image('B', p['des2'], p['xy2'])
            del log[:]
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                fwd, rev = matcher.ratio_pair_matches(i1, i2)
            # the figures the reference prints: per bin len / fit / unique, the bins it takes
            stats = np.full((len(rr.CUTOFFS), 3), -1, np.int32)
            stats[:, 0] = 0
            chosen, cur = -1, -1
            for line in out.getvalue().splitlines():
                m = re.match(r'bin: (\d+) cutoff: \S+ len: (\d+)', line)
                if m:
                    cur = int(m.group(1))
                    stats[cur, 0] = int(m.group(2))
                m = re.match(r' fit: (\d+) unique: (\d+)', line)
                if m:
                    stats[cur, 1], stats[cur, 2] = int(m.group(1)), int(m.group(2))
                if line.startswith('Filtered matches:'):
                    chosen = cur
            try:
                margin = min([check_bin(c, vr) for c in log] + [np.inf])
            except Refused as exc:
                sys.exit('case %s refused: %s' % (name, exc))
            arr = lambda l: np.asarray(l, np.int32).reshape(-1, 2)
            results.append(dict(fwd=arr(fwd), rev=arr(rev), stats=stats, chosen=chosen,
                                margin=margin, bins_run=len(log)))
            print('%-10s rows %4d x %4d  len %s  fit %s  unique %s  chosen %d  result %d  margin %.3g'
                  % (name, len(p['des1']), len(p['des2']), stats[:, 0].tolist(), stats[:, 1].tolist(),
                     stats[:, 2].tolist(), chosen, len(fwd), margin))
        gold = dict(inp, hypotheses=rr.HYPOTHESES, seed=rr.SEED, cutoffs=list(rr.CUTOFFS),
                    tol=rr.tolerance(int(inp['width']), int(inp['height'])), results=results)
        path = os.path.join(GOLD, 'ratio_%s.pkl.gz' % name)
        with gzip.GzipFile(path, 'wb', mtime=0) as f:
            pickle.dump(gold, f, protocol=4)
        print('  ->', os.path.relpath(path, REPO), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
