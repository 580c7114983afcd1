#!/usr/bin/env python3
"""Rate of the semi-global mode of the dense stage (imageanalysis_amd/dense.py, SEMI-GLOBAL RULES) on
tools/dense_rate.py's rendered scene: 684 x 456 views, 4 neighbours, 64 planes, r = 3.

    python tools/dense_sgm_rate.py [--width 684 --height 456] [--planes 64] [--radius 3] [--repeats 3] [--out FILE]

Reported by device events, each `repeats` times with the spread, after a warm-up of every launch:
  sweep            iamx_dense_sweep alone and iamx_dense_sweep_volume (the same launch with the cost
                   volume written), the two alternating inside one repeat
  each direction   iamx_dense_sgm_direction adding into the total (what directions 1 .. 7 of a call do)
                   and, for direction 0, storing; then iamx_dense_sgm_paths, the eight in a row
  select           iamx_dense_sgm_select
beside each the bytes the stage moves (volume h w planes, total 2 h w planes, the maps) and a plain
device copy of as many bytes (half read, half written), as the project does elsewhere; then
  depth_maps       the whole call over the five views, per reference image, regularize 'none' and 'sgm'"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from imageanalysis_amd import _lib, dense, kernels  # noqa: E402
from dense_rate import make_views, spread  # noqa: E402

LAUNCHES = 20                          # per timed window


def timed(fn, repeats, launches=LAUNCHES):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _k in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / launches)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=684)
    ap.add_argument('--height', type=int, default=456)
    ap.add_argument('--planes', type=int, default=64)
    ap.add_argument('--radius', type=int, default=3)
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

    w, h, D, r = args.width, args.height, args.planes, args.radius
    p1, p2 = dense.SGM_P1, dense.SGM_P2
    host = make_views(w, h)
    rays = kernels._dev(host[0].rays, torch.float64)
    G = kernels._dev(np.stack([v.G for v in host]), torch.float32)
    views = [dense.View(G[k], v.K, v.dist, v.R, v.C, rays=rays) for k, v in enumerate(host)]
    torch.cuda.synchronize()
    say('%d views of %d x %d; %d planes, r = %d, 4 neighbours, depths 80 .. 125 m; P1 = %d, P2 = %d, 8 paths'
        % (len(views), w, h, D, r, p1, p2))
    w_far, w_near = 1.0 / 125.0, 1.0 / 80.0
    neighbours = [[j for j in range(5) if j != i] for i in range(5)]
    P = kernels._ptr
    L = _lib.lib()

    def copy_line(nbytes):
        """a device copy that moves nbytes in all: half read, half written"""
        n = max(1, nbytes // 2)
        src = torch.empty(n, dtype=torch.uint8, device=dev)
        dst = torch.empty(n, dtype=torch.uint8, device=dev)
        src.zero_()
        t = timed(lambda: dst.copy_(src), args.repeats)
        med = sorted(t)[len(t) // 2]
        return 'a device copy of those bytes: median %.3f ms (%.2f TB/s)' % (med, nbytes / (med * 1e-3) / 1e12)

    # ---- the sweep, without and with the volume ----
    out = [torch.empty((h, w), dtype=torch.int32, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev),
           torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w, 3), dtype=torch.float32, device=dev)]
    volume = torch.empty((h, w, D), dtype=torch.uint8, device=dev)
    total = torch.empty((h, w, D), dtype=torch.int16, device=dev)
    nb = torch.stack([views[j].G for j in neighbours[0]]).contiguous()
    pose = kernels._dev(kernels.dense_camera(views[0])[:12], torch.float64)
    cams = kernels._dev(np.stack([kernels.dense_camera(views[j]) for j in neighbours[0]]), torch.float64)
    head = (P(views[0].G), P(rays), P(nb), P(pose), P(cams), w, h, 4, D, w_far, w_near, r, 4.0, 0.6) + tuple(P(t) for t in out)

    def sweep():
        _lib.check(L.iamx_dense_sweep(*(head + (_lib.stream_ptr(),))), 'iamx_dense_sweep')

    def sweep_volume():
        _lib.check(L.iamx_dense_sweep_volume(*(head + (P(volume), _lib.stream_ptr()))), 'iamx_dense_sweep_volume')

    sweep()
    sweep_volume()
    torch.cuda.synchronize()
    plain, with_vol = [], []
    for _ in range(args.repeats):                            # (alternating: one repeat of each after the other)
        plain += timed(sweep, 1)
        with_vol += timed(sweep_volume, 1)
    vol_bytes = h * w * D
    say('sweep alone, per reference image (%d launches per repeat): %s' % (LAUNCHES, spread(plain)))
    say('sweep with the volume (%d bytes written more): %s' % (vol_bytes, spread(with_vol)))
    say('  the emission costs median %+.3f ms; %s'
        % (sorted(with_vol)[len(with_vol) // 2] - sorted(plain)[len(plain) // 2], copy_line(2 * vol_bytes)))
    invalid = float((volume == 255).float().mean())
    say('  %.3f of the costs are 255' % invalid)

    # ---- the directions ----
    def direction(k, accumulate):
        def run():
            _lib.check(L.iamx_dense_sgm_direction(P(volume), w, h, D, k, accumulate, p1, p2, 127, P(total), _lib.stream_ptr()),
                       'iamx_dense_sgm_direction')
        return run

    names = ['(%+d,%+d)' % d for d in kernels.DENSE_SGM_DIRECTIONS]
    say('direction 0 %s storing (reads the volume, writes the total: %d bytes): %s'
        % (names[0], 3 * vol_bytes, spread(timed(direction(0, 0), args.repeats))))
    for k in range(8):
        n_paths = h if k < 2 else (w if k < 4 else w + h - 1)
        say('direction %d %s adding (%d waves; volume read, total read and written: %d bytes): %s'
            % (k, names[k], n_paths, 5 * vol_bytes, spread(timed(direction(k, 1), args.repeats))))
    say('  %s' % copy_line(5 * vol_bytes))

    def paths():
        _lib.check(L.iamx_dense_sgm_paths(P(volume), w, h, D, 8, p1, p2, 127, P(total), _lib.stream_ptr()), 'iamx_dense_sgm_paths')

    say('iamx_dense_sgm_paths, 8 directions (%d bytes): %s' % ((3 + 7 * 5) * vol_bytes, spread(timed(paths, args.repeats))))
    say('  %s' % copy_line((3 + 7 * 5) * vol_bytes))

    # ---- select ----
    sel = [torch.empty((h, w), dtype=torch.int32, device=dev), torch.empty((h, w), dtype=torch.uint8, device=dev),
           torch.empty((h, w), dtype=torch.int16, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev)]
    step = (w_near - w_far) / (D - 1)

    def select():
        _lib.check(L.iamx_dense_sgm_select(P(total), P(volume), w, h, D, w_far, step, dense.sgm_max_cost(0.6),
                                           *([P(t) for t in sel] + [_lib.stream_ptr()])), 'iamx_dense_sgm_select')

    paths()
    sel_bytes = 2 * vol_bytes + h * w * (1 + 11)
    say('select (total read, one cost and 11 bytes of maps per pixel: %d bytes): %s' % (sel_bytes, spread(timed(select, args.repeats))))
    say('  %s; %.2f of the pixels kept by select, %.2f by the sweep'
        % (copy_line(sel_bytes), float(torch.isfinite(sel[3]).float().mean()), float(torch.isfinite(out[2]).float().mean())))

    # ---- depth_maps, the whole call ----
    ranges = [(80.0, 125.0)] * 5
    for mode in ('none', 'sgm', 'none', 'sgm'):
        maps = dense.depth_maps(views, neighbours, ranges, planes=D, radius=r, regularize=mode)
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            maps = dense.depth_maps(views, neighbours, ranges, planes=D, radius=r, regularize=mode)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / 5.0)
        say("depth_maps(regularize='%s'), whole call over 5 views, per reference image: %s; %.2f of the pixels survive the check"
            % (mode, spread(times), float(maps.keep.float().mean())))
    if log:
        log.close()


if __name__ == '__main__':
    main()
