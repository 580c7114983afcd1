#!/usr/bin/env python3
"""Rate of the coarse-to-fine dense sweep (imageanalysis_amd/dense.py, REFINEMENT RULES) on tools/dense_rate.py's
rendered scene: a coarse level of 684 x 456 views with 64 planes, a fine level of 1368 x 912 views at ratio 4
(T = 253 planes), 4 neighbours, r = 3.

    python tools/dense_refine_rate.py [--width 1368 --height 912] [--planes 64] [--ratio 4] [--radius 3]
                                      [--repeats 3] [--baseline-lib LIBIAMX.SO] [--out FILE]

Reported, each `repeats` times with the spread, the variants of one comparison alternating inside a repeat:
  guide          iamx_dense_guide alone by device events (the coarse map of view 0 -> its window table)
  guided sweep   iamx_dense_sweep_guided per reference image by device events -- the entry reads the table
                 back and checks it before the launch, so each call includes that copy and one stream
                 synchronise -- with the mean and the largest window of the table it walked
  plain sweep    iamx_dense_sweep on the same fine views with `planes` and with T planes; --baseline-lib:
                 the same two from another build of the library (the parent commit's), in the same windows
  per plane      each sweep's time over the planes a tile walks on average: whether time scales with that
  refine         the whole dense.refine call for the five views (guides, sweeps, uploads, the check), per
                 reference image"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from imageanalysis_amd import _lib, dense, kernels  # noqa: E402
from dense_rate import make_views, spread  # noqa: E402

LAUNCHES = 10                          # of a sweep kernel per timed window
GUIDE_LAUNCHES = 200


def load_library(path):
    """another build of libiamx.so, its entries typed from this tree's header where it has them"""
    h = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(h, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return h


def device_views(host):
    rays = kernels._dev(host[0].rays, torch.float64)
    G = kernels._dev(np.stack([v.G for v in host]), torch.float32)
    return [dense.View(G[k], v.K, v.dist, v.R, v.C, rays=rays) for k, v in enumerate(host)]


def timed(variants, launches, repeats):
    """variants: name -> a function that enqueues one call.  -> name -> ms per call, one per repeat; the
    variants alternate inside every repeat, each after a warm-up call"""
    out = dict((name, []) for name in variants)
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _k in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / launches)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1368, help='of the fine views; the coarse ones are half')
    ap.add_argument('--height', type=int, default=912)
    ap.add_argument('--planes', type=int, default=64, help='of the coarse level')
    ap.add_argument('--ratio', type=int, default=4)
    ap.add_argument('--radius', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--baseline-lib', help='another libiamx.so whose iamx_dense_sweep is timed beside this one')
    ap.add_argument('--out', help='also write the lines to this file')
    args = ap.parse_args()
    if args.width % 2 or args.height % 2:
        ap.error('an even fine size wanted: the coarse views are half of it')
    dev = _lib.require_gpu()
    log = open(args.out, 'w') if args.out else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + '\n')
            log.flush()

    w, h, D, r = args.width, args.height, args.planes, args.radius
    T = dense.refine_planes(D, args.ratio)
    t0 = time.time()
    fine, coarse = device_views(make_views(w, h)), device_views(make_views(w // 2, h // 2))
    torch.cuda.synchronize()
    say('5 views of %d x %d and of %d x %d rendered in %.1f s; coarse %d planes, ratio %d: T = %d; r = %d, 4 neighbours, '
        'depths 80 .. 125 m' % (w, h, w // 2, h // 2, time.time() - t0, D, args.ratio, T, r))
    w_far, w_near = 1.0 / 125.0, 1.0 / 80.0
    ranges = [(80.0, 125.0)] * 5
    neighbours = [[j for j in range(5) if j != i] for i in range(5)]
    coarse_maps = dense.depth_maps(coarse, neighbours, ranges, planes=D, radius=r)
    say('coarse level: %.2f of the pixels survive the check' % float(coarse_maps.keep.float().mean()))

    L = _lib.lib()
    P = kernels._ptr
    nan = torch.full_like(coarse_maps.depth[0], float('nan'))
    guide_depth = torch.where(coarse_maps.keep[0] != 0, coarse_maps.depth[0], nan).contiguous()
    windows = torch.empty(kernels.dense_tiles(h, w) + (2,), dtype=torch.int32, device=dev)

    def guide():
        _lib.check(L.iamx_dense_guide(P(guide_depth), w // 2, h // 2, w, h, w_far, w_near, T, r, args.ratio, P(windows),
                                      _lib.stream_ptr()), 'iamx_dense_guide')
    ms = timed({'guide': guide}, GUIDE_LAUNCHES, args.repeats)['guide']
    count = windows[..., 1].float()
    mean_count, max_count = float(count.mean()), int(count.max())
    say('guide kernel, %d x %d tiles (%d launches per repeat): %s' % (windows.shape[1], windows.shape[0], GUIDE_LAUNCHES, spread(ms)))
    say('window table of view 0: %.1f of %d planes per tile on average, at most %d, %d tiles empty'
        % (mean_count, T, max_count, int((count == 0).sum())))

    out = [torch.empty((h, w), dtype=torch.int32, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev),
           torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w, 3), dtype=torch.float32, device=dev)]
    nb = torch.stack([fine[j].G for j in neighbours[0]]).contiguous()
    pose = kernels._dev(kernels.dense_camera(fine[0])[:12], torch.float64)
    cams = kernels._dev(np.stack([kernels.dense_camera(fine[j]) for j in neighbours[0]]), torch.float64)
    front = (P(fine[0].G), P(fine[0].rays), P(nb), P(pose), P(cams), w, h, 4)
    back = tuple(P(t) for t in out)

    def plain(lib, planes):
        def launch():
            _lib.check(lib.iamx_dense_sweep(*(front + (planes, w_far, w_near, r, 4.0, 0.6) + back + (_lib.stream_ptr(),))),
                       'iamx_dense_sweep')
        return launch

    def guided():
        _lib.check(L.iamx_dense_sweep_guided(*(front + (T, w_far, w_near, r, 4.0, 0.6, P(windows)) + back +
                                               (_lib.stream_ptr(),))), 'iamx_dense_sweep_guided')

    variants = {'guided sweep, T = %d' % T: guided}
    walked = {'guided sweep, T = %d' % T: mean_count}
    libs = [('', L)] + ([(' (baseline library)', load_library(args.baseline_lib))] if args.baseline_lib else [])
    for tag, lib in libs:
        for planes in (D, T):
            if planes <= kernels.DENSE_MAX_PLANES:
                name = 'plain sweep, %d planes%s' % (planes, tag)
                variants[name], walked[name] = plain(lib, planes), float(planes)
    guided()
    torch.cuda.synchronize()
    kept = float(torch.isfinite(out[2]).float().mean())
    times = timed(variants, LAUNCHES, args.repeats)
    say('per reference image of %d x %d (%d launches per repeat, the variants alternating):' % (w, h, LAUNCHES))
    for name, ms in times.items():
        med = sorted(ms)[len(ms) // 2]
        say('  %-44s %s; %.4f ms per plane walked' % (name + ':', spread(ms), med / walked[name]))
    say('  the guided sweep keeps %.2f of the pixels' % kept)

    dense.refine(fine, neighbours, ranges, coarse_maps, D, ratio=args.ratio, radius=r)
    ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        maps = dense.refine(fine, neighbours, ranges, coarse_maps, D, ratio=args.ratio, radius=r)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / 5.0)
    count = maps.windows[..., 1].float()
    say('refine, whole call over 5 views, per reference image: %s; %.1f planes per tile on average, at most %d; '
        '%.2f of the pixels survive the check' % (spread(ms), float(count.mean()), int(count.max()),
                                                  float(maps.keep.float().mean())))
    if log:
        log.close()


if __name__ == '__main__':
    main()
