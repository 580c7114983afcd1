#!/usr/bin/env python3
"""The surface-consistency cull (4c-surface-outliers) on two synthetic surveys: BASELINE config 4's
shape (2812 nadir images on a lawn-mower grid, about 700 observations each, pair-wise chains) and one
of 5000 observations per image:

  * iamx_surface_knn_fit alone, device-resident arguments, by device events; the pixel pair distances
    it evaluates per second (sum of n_i^2 over the images per launch, five f64 operations each) beside
    the f64 vector peak of the MI355X (78.6 TFLOP/s by its published specification, half the 157.3
    TFLOP/s FP32 vector figure) -- a fraction to read, not a gate;
  * the whole match_culling.cull_surface call on the array-backed Chains: observation table on the
    host, upload, every round's kernels and statistics;
  * the restatement's own neighbour and fit step (scipy.spatial.cKDTree + the closed-form line of
    tests/surface_cull_restatement.py) on this host's cores, on --loop-images images, EXTRAPOLATED to
    the survey by observations and labelled so.  It is NOT the reference's loop (Python 2, KDTree and
    np.polyfit per feature), which cannot run on today's project.

Every figure is taken --repeats times; the text gives the median and the spread (min .. max).

    python tools/surface_cull_rate.py [--out profiles/r25_surface_cull_rate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

F64_VECTOR_PEAK = 78.6e12
FLOP_PER_PAIR = 5                       # two differences, two products, one sum


def spread(xs):
    xs = sorted(xs)
    return '%.4g (min %.4g .. max %.4g, n=%d)' % (xs[len(xs) // 2], xs[0], xs[-1], len(xs))


def survey(rows, cols, per_image, seed, bad=0.002):
    """nadir cameras on a rows x cols grid at 100 m, per_image / 2 features between each camera and its
    next one along the row (pair-wise chains), `bad` of them displaced vertically -> Chains arrays, cam"""
    rng = np.random.default_rng(seed)
    C = rows * cols
    cam = np.array([[40.0 * r, 60.0 * c, -100.0] for r in range(rows) for c in range(cols)])
    a = np.repeat(np.arange(C), per_image // 2)
    b = np.where((a % cols) == cols - 1, a - 1, a + 1)
    mid = (cam[a] + cam[b]) / 2
    pts = np.stack([mid[:, 0] + rng.uniform(-45, 45, len(a)), mid[:, 1] + rng.uniform(-35, 35, len(a)),
                    rng.uniform(-1.0, 1.0, len(a))], 1)
    hit = rng.uniform(size=len(a)) < bad
    pts[hit, 2] += rng.uniform(15, 40, int(hit.sum()))
    img = np.stack([a, b], 1).ravel().astype(np.int32)
    d = np.repeat(pts, 2, 0) - cam[img]
    uv = np.stack([2736.0 + 3648.0 * d[:, 1] / d[:, 2], 1824.0 - 3648.0 * d[:, 0] / d[:, 2]], 1)
    uv += rng.normal(0, 0.3, uv.shape)
    return img, uv, np.arange(0, 2 * len(a) + 1, 2, dtype=np.int64), pts, cam, int(hit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--loop-images', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from scipy.spatial import cKDTree
    import surface_cull_restatement as sr
    from imageanalysis_amd import kernels, match_cleanup
    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd.hostlib.image_pose import PoseProject

    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    clock = time.perf_counter
    say('surface cull on synthetic surveys (%s); host cores for the restatement: %d'
        % (torch.cuda.get_device_name(0), len(os.sched_getaffinity(0))))
    for label, rows, cols, per_image in (('config-4 shape', 38, 74, 700), ('dense images', 10, 20, 5000)):
        t = clock()
        img, uv, ptr, pts, cam, n_bad = survey(rows, cols, per_image, 25)
        chains = match_cleanup.Chains(img, uv, ptr)
        chains.group[:] = 0
        chains.ned[:] = pts
        chains.has_ned[:] = True
        names = ['IMG_%05d' % i for i in range(len(cam))]
        proj = PoseProject(names)
        for im, p in zip(proj.image_list, cam):
            im.set_camera_pose(p.tolist(), 0.0, 0.0, 0.0, opt=True)
        table = cull.observation_table(proj, chains, [names], 0).upload()
        sizes = np.diff(table.img_ptr)
        pairs = int((sizes.astype(np.int64) ** 2).sum())
        say()
        say('%s: %d images, %d chains (%d displaced), %d observations (%d .. %d per image), %d pixel pairs '
            '(built in %.1f s)' % (label, len(cam), len(ptr) - 1, n_bad, len(img), sizes.min(), sizes.max(),
                                   pairs, clock() - t))
        ts = []
        for _ in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            kernels.surface_knn_fit(table.d_img_ptr, table.d_uv, table.d_ned, table.d_chain, 30, 10)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 1e3)
        med = sorted(ts[1:])[len(ts[1:]) // 2]
        say('    iamx_surface_knn_fit alone (device events, first launch dropped) s: %s' % spread(ts[1:]))
        say('        %.3g pair distances/s = %.3g f64 FLOP/s = %.2f %% of the %.1f TFLOP/s f64 vector peak '
            '(insertions, walks and fits not counted)'
            % (pairs / med, FLOP_PER_PAIR * pairs / med, 100 * FLOP_PER_PAIR * pairs / med / F64_VECTOR_PEAK,
               F64_VECTOR_PEAK / 1e12))
        tc, rounds = [], None
        for _ in range(a.repeats + 1):
            chains.marked = np.zeros(len(chains.img), bool)
            t = clock()
            with open(os.devnull, 'w') as null:
                old, sys.stdout = sys.stdout, null
                try:
                    rounds = cull.cull_surface(proj, chains, [names], 0)
                finally:
                    sys.stdout = old
            tc.append(clock() - t)
        assert chains.untouched()
        say('    cull_surface, whole call (table, upload, %d rounds, marking): first %.4g s, then s: %s'
            % (len(rounds), tc[0], spread(tc[1:])))
        say('        culled per round: %s' % [len(r) for r in rounds])
        pick = np.linspace(0, len(cam) - 1, min(a.loop_images, len(cam))).astype(int)
        th = []
        for _ in range(a.repeats):
            t = clock()
            for im in pick.tolist():
                lo, hi = int(table.img_ptr[im]), int(table.img_ptr[im + 1])
                u, ned = table.uv[lo:hi], table.ned[lo:hi].tolist()
                d, idx = cKDTree(u).query(u, k=min(30, hi - lo))
                for i in range(hi - lo):
                    m = sr.walk(d[i] * d[i], 10)
                    sr.line(d[i, :m].tolist(), [sr.dist3(ned[i], ned[j]) for j in idx[i, :m].tolist()])
            th.append(clock() - t)
        have = int(sizes[pick].sum())
        say('    cKDTree + closed-form line on this host (one thread), %d images = %d observations, measured s: %s; '
            'EXTRAPOLATED by observations to one round of the survey s: %s'
            % (len(pick), have, spread(th), spread([x * len(img) / have for x in th])))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
