#!/usr/bin/env python3
"""What iamx_verify_pairs (csrc/match_verify.hip) costs.

  kernel   4096 pairs x 2000 matches and 4096 x 200, 2048 hypotheses, both models: the launch by
           device events, two warm-up launches, five timed.  Operations: the scoring pass only,
           19 f64 operations per (hypothesis, match) for the homography and 31 for the fundamental
           matrix (every add, multiply, divide one operation; the solve and the mask pass are left
           out of the count), over the kernel time, beside 78.6 Tf64op/s -- half the FP32 vector
           rate of 157.3 TFLOPS: the public FP64 vector figure of the MI355X.
           Inputs: flat-field (homography) and relief (fundamental) scenes of
           tests/verify_reference.py with a quarter outliers, 64 distinct pairs tiled.
  --essential
           the essential model (iamx_verify_pairs_essential, five-point samples) beside the
           fundamental one on the same relief scenes, 4096 x 2000 and 4096 x 200 matches at 256 and at
           2048 hypotheses, timed the same way.  The split into solve and scoring is a straight line
           through the two sizes of n (time = solve + n * per match): the samples, and so the solve,
           do not depend on what is scored.
  --e2e N  bench.e2e_bench(N)'s rendered survey: seconds of matcher.find_matches, then of
           matcher.verify_matches('homography') and ('fundamental') on copies of its match lists.

    python tools/verify_rate.py [--pairs 4096] [--hypotheses 2048] [--essential] [--e2e 512] [--out FILE]"""
import argparse
import copy
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import torch  # noqa: E402

from imageanalysis_amd import kernels, matcher  # noqa: E402
import verify_reference as vr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=4096)
ap.add_argument('--hypotheses', type=int, default=2048)
ap.add_argument('--e2e', type=int, default=0)
ap.add_argument('--essential', action='store_true')
ap.add_argument('--out', default=None)
args = ap.parse_args()
lines = []
OPS = {'homography': 19, 'fundamental': 31}
F64_PEAK = 78.6e12


def say(s):
    print(s, flush=True)
    lines.append(s)


def kernel_rates():
    say('iamx_verify_pairs, %d pairs, %d hypotheses, device events, 2 warm-up + 5 timed launches:'
        % (args.pairs, args.hypotheses))
    for n in (2000, 200):
        for model, relief in (('homography', 0.0), ('fundamental', 25.0)):
            distinct = [vr.scene(n, 0.75, relief, 9000 + k)[0] for k in range(4 if n > 500 else 64)]
            pts = np.concatenate([distinct[k % len(distinct)] for k in range(args.pairs)])
            m_off = np.arange(args.pairs + 1, dtype=np.int64) * n
            d_pts = torch.from_numpy(pts).cuda()
            d_off = torch.from_numpy(m_off).cuda()
            ts = []
            for k in range(7):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                mask, _m, best, status = kernels.verify_pairs(d_pts, d_off, model, vr.TOL,
                                                              args.hypotheses, 0)
                b.record()
                b.synchronize()
                if k >= 2:
                    ts.append(a.elapsed_time(b))
            ts = np.array(ts)
            ops = float(args.pairs) * n * args.hypotheses * OPS[model]
            assert int((status != 0).sum()) == 0
            say('  %-11s n = %4d   %8.2f ms (%.2f .. %.2f)   %.2f us per pair   %5.2f Tf64op/s scoring'
                ' = %4.1f %% of 78.6   inliers kept %.3f'
                % (model, n, ts.mean(), ts.min(), ts.max(), ts.mean() * 1e3 / args.pairs,
                   ops / (ts.mean() * 1e-3) / 1e12, 100 * ops / (ts.mean() * 1e-3) / F64_PEAK,
                   float(mask.float().mean())))


def _timed(d_pts, d_off, model, hypotheses, K=None):
    ts = []
    for k in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        mask, _m, _best, status = kernels.verify_pairs(d_pts, d_off, model, vr.TOL, hypotheses, 0, K=K)
        b.record()
        b.synchronize()
        if k >= 2:
            ts.append(a.elapsed_time(b))
    assert int((status != 0).sum()) == 0
    return np.array(ts), float(mask.float().mean())


def essential_rates():
    say('iamx_verify_pairs_essential beside iamx_verify_pairs fundamental, %d pairs, relief scenes with a '
        'quarter outliers, device events, 2 warm-up + 5 timed launches:' % args.pairs)
    for hypotheses in (256, 2048):
        mean = {}
        for n in (2000, 200):
            distinct = [vr.scene(n, 0.75, 25.0, 9000 + k)[0] for k in range(4 if n > 500 else 64)]
            pts = np.concatenate([distinct[k % len(distinct)] for k in range(args.pairs)])
            d_pts = torch.from_numpy(pts).cuda()
            d_off = torch.from_numpy(np.arange(args.pairs + 1, dtype=np.int64) * n).cuda()
            for model, K in (('fundamental', None), ('essential', vr.KMAT)):
                ts, kept = _timed(d_pts, d_off, model, hypotheses, K)
                mean[(model, n)] = ts.mean()
                say('  %-11s %4d hypotheses  n = %4d   %8.2f ms (%.2f .. %.2f)   %7.2f us per pair   '
                    'inliers kept %.3f' % (model, hypotheses, n, ts.mean(), ts.min(), ts.max(),
                                           ts.mean() * 1e3 / args.pairs, kept))
        for model in ('fundamental', 'essential'):
            per = (mean[(model, 2000)] - mean[(model, 200)]) / 1800.0
            solve = mean[(model, 200)] - 200 * per
            say('  %-11s %4d hypotheses  line through n = 200 and 2000: %.2f ms that do not depend on n '
                '(solve), %.2f ms per 1000 matches (scoring and mask)' % (model, hypotheses, solve, 1000 * per))


class _Done(Exception):
    pass


def e2e(n_images):
    import bench
    got = {}
    orig = matcher.find_matches

    def find_and_verify(proj, K, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        orig(proj, K, **kw)
        torch.cuda.synchronize()
        got['find_matches'] = time.perf_counter() - t
        for im in proj.image_list:
            if im.kp_list is None:
                im.load_features()
        from imageanalysis_amd.matchpairs import MatchPairs

        def dup(v):
            return MatchPairs(v.array().copy()) if isinstance(v, MatchPairs) else copy.deepcopy(v)
        lists = [dict((k, dup(v)) for k, v in im.match_list.items()) for im in proj.image_list]
        for transform in ('homography', 'fundamental'):
            for im, ml in zip(proj.image_list, lists):
                im.match_list = dict((k, dup(v)) for k, v in ml.items())
                im.uv_list = None
            torch.cuda.synchronize()
            t = time.perf_counter()
            counts = matcher.verify_matches(proj, K, transform, hypotheses=args.hypotheses)
            torch.cuda.synchronize()
            got[transform] = (time.perf_counter() - t, counts)
        raise _Done()

    matcher.find_matches = find_and_verify
    try:
        bench.e2e_bench(n_images)
    except _Done:
        pass
    finally:
        matcher.find_matches = orig
    say('rendered survey of bench.e2e_bench(%d):' % n_images)
    say('  matcher.find_matches                      %8.3f s' % got['find_matches'])
    for transform in ('homography', 'fundamental'):
        sec, c = got[transform]
        say('  matcher.verify_matches %-12s       %8.3f s   (undistortion of every keypoint included)'
            '   %d pairs, %d -> %d matches, %d lists emptied, %d no model'
            % (transform, sec, c['pairs'], c['matches_in'], c['matches_out'], c['lists_emptied'],
               c['no_model']))


if args.essential:
    essential_rates()
else:
    kernel_rates()
if args.e2e:
    e2e(args.e2e)
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
