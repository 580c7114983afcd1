#!/usr/bin/env python3
"""Rate of the robust DSM fusion (imageanalysis_amd/dense.py, ROBUST FUSION RULES; csrc/dense_fuse.hip) beside
the mean it stands next to, on the many-views cloud of tools/dense_rate.py: its five rendered 684 x 456 views
swept once, repeated to `views` views and cross-checked, about 50 M surviving points into a raster at 0.25 m.

    python tools/dense_fuse_rate.py [--views 200] [--gsd 0.25] [--bins 32] [--repeats 3] [--out FILE]

Reported, each `repeats` times after a warm-up, with the spread:
  fuse           the whole dense.fuse call (the frame from the points' bounds, the kernels, the resolve) with
                 method 'mean' -- the yardstick -- and 'robust' at the defaults and at levels 1 and 4
  each kernel    by device events inside one robust sequence per level count: iamx_dense_fuse_range, every
                 level's iamx_dense_fuse_hist and iamx_dense_fuse_select, iamx_dense_fuse_sum, and the mean's
                 iamx_dense_splat; every point pass as a multiple of the splat and of a plain device copy of the
                 25 bytes per point it reads (24 of ned, 1 of keep), the select beside a copy of the 2 x 4 bins
                 + 2 x 16 bytes per cell it moves (hist read and zeroed, window read and written)
  contention     the same point passes over the cloud with every point once (the first five views): what the
                 passes cost when a cell's atomics are a fortieth as many"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dense_rate  # noqa: E402
from imageanalysis_amd import _lib, dense, kernels  # noqa: E402

_ptr = kernels._ptr


def timed(launch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(launch(), 'launch')
    e1.record()
    return e0, e1


def kernel_times(ned, keep, frame, bins, levels, wmin, share, repeats):
    """one robust sequence per repeat, an event pair around every launch -> {name: [ms per repeat]}, and the mean's
    splat and the copies beside it"""
    x0, y1, gsd, W, H = frame
    dev = ned.device
    L, s = _lib.lib(), _lib.stream_ptr()
    P, Kp = ned.reshape(-1, 3), keep.reshape(-1)
    n = int(P.shape[0])
    pts = (_ptr(P), _ptr(Kp), n, x0, y1, gsd, W, H)
    count = torch.empty((H, W), dtype=torch.int32, device=dev)
    support = torch.empty((H, W), dtype=torch.int32, device=dev)
    total = torch.empty((H, W), dtype=torch.int64, device=dev)
    window = torch.empty((H, W, 2), dtype=torch.int64, device=dev)
    hist = torch.zeros((H, W, bins), dtype=torch.int32, device=dev)
    P2, K2 = torch.empty_like(P), torch.empty_like(Kp)
    cell_bytes = torch.empty(W * H * (4 * bins + 16), dtype=torch.uint8, device=dev)
    cell_copy = torch.empty_like(cell_bytes)
    out = {}
    for rep in range(repeats + 1):
        ev = []
        count.zero_(), support.zero_(), total.zero_(), hist.zero_()
        window[..., 0] = torch.iinfo(torch.int64).max
        window[..., 1] = torch.iinfo(torch.int64).min
        ev.append(('range', timed(lambda: L.iamx_dense_fuse_range(*(pts + (_ptr(count), _ptr(window), s))))))
        for level in range(1, levels + 1):
            ev.append(('hist %d' % level, timed(lambda: L.iamx_dense_fuse_hist(*(pts + (_ptr(window), bins, wmin, _ptr(hist), s))))))
            ev.append(('select %d' % level, timed(lambda: L.iamx_dense_fuse_select(
                _ptr(count), W, H, bins, wmin, share if level == 1 else 256, _ptr(hist), _ptr(window), s))))
        ev.append(('sum', timed(lambda: L.iamx_dense_fuse_sum(*(pts + (_ptr(window), _ptr(support), _ptr(total), s))))))
        count.zero_(), total.zero_()
        ev.append(('splat (mean)', timed(lambda: L.iamx_dense_splat(*(pts + (_ptr(count), _ptr(total), s))))))

        def copy_points():
            P2.copy_(P)
            K2.copy_(Kp)
            return 0

        def copy_cells():
            cell_copy.copy_(cell_bytes)
            return 0
        ev.append(('copy of 25 B a point', timed(copy_points)))
        ev.append(('copy of 4 bins + 16 B a cell', timed(copy_cells)))
        torch.cuda.synchronize()
        if rep:
            for name, (e0, e1) in ev:
                out.setdefault(name, []).append(e0.elapsed_time(e1))
    return out


def report(say, times, n, cells, bins):
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    splat, copy, cell_copy = med['splat (mean)'], med['copy of 25 B a point'], med['copy of 4 bins + 16 B a cell']
    for name, ms in times.items():
        line = '  %-30s %s' % (name, dense_rate.spread(ms))
        if name.startswith('select'):
            line += '; %.2f x the copy of its cells\' bytes, %.2f x the splat' % (med[name] / cell_copy, med[name] / splat)
        elif not name.startswith('copy'):
            line += '; %.2f x the splat, %.2f x the copy, %.1f G points/s' % (med[name] / splat, med[name] / copy, n / med[name] / 1e6)
        else:
            b = 25.0 * n if 'point' in name else (4.0 * bins + 16) * cells
            line += '; %.2f TB/s read + as much written' % (b / med[name] / 1e9)
        say(line)
    passes = [k for k in med if not k.startswith(('copy', 'select', 'splat'))]
    say('  the %d point passes together %.3f ms = %.2f x the splat; the selects %.3f ms'
        % (len(passes), sum(med[k] for k in passes), sum(med[k] for k in passes) / splat,
           sum(med[k] for k in med if k.startswith('select'))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=200)
    ap.add_argument('--gsd', type=float, default=0.25)
    ap.add_argument('--bins', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', help='also write the lines to this file')
    args = ap.parse_args()
    dev = _lib.require_gpu()
    log = open(args.out, 'w') if args.out else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + '\n')
            log.flush()

    w, h = 684, 456
    host = dense_rate.make_views(w, h)
    rays = kernels._dev(host[0].rays, torch.float64)
    G = kernels._dev(np.stack([v.G for v in host]), torch.float32)
    views = [dense.View(G[k], v.K, v.dist, v.R, v.C, rays=rays) for k, v in enumerate(host)]
    neighbours = [[j for j in range(5) if j != i] for i in range(5)]
    maps = dense.depth_maps(views, neighbours, [(80.0, 125.0)] * 5, planes=64, radius=3)
    V = max(5, args.views // 5 * 5)
    many = [views[k % 5] for k in range(V)]
    many_nb = [[5 * (k // 5) + j for j in neighbours[k % 5]] for k in range(V)]
    keep, ned = kernels.dense_check(maps.depth.repeat(V // 5, 1, 1).contiguous(), many, many_nb)
    big = dense.DepthMaps(keep=keep, ned=ned)
    n_alive = int(keep.sum())
    say('%d views of %d x %d, %d points of which %d survive the check; gsd %.2f m, %d bins' % (V, w, h, keep.numel(), n_alive, args.gsd, args.bins))

    # ---- the whole call ----
    modes = [('mean', dict(method='mean'))] + [('robust, levels %d%s' % (lv, ' (default)' if lv == 2 else ''),
                                                dict(method='robust', bins=args.bins, levels=lv)) for lv in (2, 1, 4)]
    surface = None
    whole = {}
    for name, kw in modes:
        times = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            surface = dense.fuse(many, big, args.gsd, **kw)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        whole[name] = sorted(times[1:])[len(times[1:]) // 2]
        extra = ''
        if surface.support is not None:
            extra = '; support / count %.3f' % (float(surface.support.sum()) / float(surface.count.sum()))
        say('fuse, %-28s %s; %.2f x the mean%s' % (name + ':', dense_rate.spread(times[1:]), whole[name] / whole['mean'], extra))
    H, W = surface.shape
    frame = (surface.x0, surface.y1, surface.gsd, W, H)
    say('the raster is %d x %d cells, %.0f surviving points a cell; per cell %d bytes (4 bins + 40), %.1f MB in all'
        % (W, H, n_alive / float(W * H), 4 * args.bins + 40, kernels.dense_fuse_bytes(W, H, args.bins) / 1e6))

    # ---- each kernel ----
    bins, _levels, wmin, share = kernels.dense_fuse_check(args.bins, 2, None, 256, args.gsd)
    n = keep.numel()
    for levels in (2, 1, 4):
        times = kernel_times(ned, keep, frame, bins, levels, wmin, share, args.repeats)
        say('kernels of a robust sequence, levels %d, over the %d views (every point %d times: the atomics\' worst case):' % (levels, V, V // 5))
        report(say, times, n, W * H, bins)
    once_keep, once_ned = keep[:5].contiguous(), ned[:5].contiguous()
    times = kernel_times(once_ned, once_keep, frame, bins, 2, wmin, share, args.repeats)
    say('the same, levels 2, over the first five views (%d points, every point once):' % once_keep.numel())
    report(say, times, once_keep.numel(), W * H, bins)
    if log:
        log.close()


if __name__ == '__main__':
    main()
