#!/usr/bin/env python3
"""Rate of the dense-surface stage (imageanalysis_amd/dense.py) on a rendered scene at the size of a
20 MP frame at 1/8 scale: 684 x 456 views, 4 neighbours, 64 planes, r = 3.

    python tools/dense_rate.py [--width 684 --height 456] [--planes 64] [--radius 3] [--views 200]
                               [--repeats 3] [--out FILE]

Five cameras 100 m above rolling ground (a cross, 25 m apart), rendered on the host by ray casting.
Reported, each `repeats` times with the spread:
  sweep kernel   iamx_dense_sweep alone by device events, outputs allocated before, after a warm-up;
                 beside it what the tap count implies: every (pixel, plane, neighbour) reads
                 3 (2r + 1)(r + 1) 8 / 2 bytes of LDS (a row of 2r + 2 floats per two pixels, once
                 for the mean and twice -- reference and warped tile -- for the centred sums)
  depth_maps     the whole call for the five views (sweeps, uploads, the check), per reference image
  dense_check    over `views` views (the five, repeated, each block its own neighbourhood)
  fuse           the frame, the splat and the resolve for the same views"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from imageanalysis_amd import _lib, dense, kernels, synth  # noqa: E402

CENTRES = ((0.0, 0.0), (0.0, 25.0), (25.0, 0.0), (0.0, -25.0), (-25.0, 0.0))
DIST = (-0.05, 0.01, 0.0005, -0.0003, 0.002)
TEXEL = 0.2
LAUNCHES = 40                          # of the sweep kernel per timed window


def ground(n, e):
    """NED down of the surface: rolling relief of a few metres"""
    return 3.0 * np.sin(n / 23.0) * np.cos(e / 31.0) + 1.5 * np.sin((n + e) / 11.0)


def host_rays(K, dist, h, w):
    fx, fy, cx, cy = K
    k1, k2, p1, p2, k3 = dist
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(20):
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        x = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / rad
        y = (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / rad
    return np.ascontiguousarray(np.stack([x, y], 2))


def make_views(w, h, seed=1):
    focal = synth.FX * w / synth.W_PX
    K = np.array([focal, focal, (w - 1) / 2.0, (h - 1) / 2.0])
    rays = host_rays(K, DIST, h, w)
    side = int(2 * (0.75 * 100.0 * w / focal + 40.0) / TEXEL)
    tex = synth.ground_texture(side, side, 3)[:, :, 0].astype(np.float64)
    rng = np.random.default_rng(seed)
    nadir = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    views = []
    for c in CENTRES:
        a, b, g = rng.uniform(-0.03, 0.03, 3)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1.0, 0], [-np.sin(b), 0, np.cos(b)]])
        Rx = np.array([[1.0, 0, 0], [0, np.cos(g), -np.sin(g)], [0, np.sin(g), np.cos(g)]])
        R = Rz.dot(Ry).dot(Rx).dot(nadir)
        C = np.array([c[0], c[1], -100.0])
        dirs = np.concatenate([rays, np.ones((h, w, 1))], 2).dot(R)
        t = np.full((h, w), 100.0)
        for _ in range(12):                                  # the relief is gentle: a fixed point
            P = C + dirs * t[:, :, None]
            t = (ground(P[:, :, 0], P[:, :, 1]) - C[2]) / dirs[:, :, 2]
        P = C + dirs * t[:, :, None]
        r = np.clip(P[:, :, 0] / TEXEL + side / 2.0, 0, side - 1.001)
        q = np.clip(P[:, :, 1] / TEXEL + side / 2.0, 0, side - 1.001)
        r0, q0 = np.floor(r).astype(int), np.floor(q).astype(int)
        fr, fq = r - r0, q - q0
        img = (tex[r0, q0] * (1 - fq) + tex[r0, q0 + 1] * fq) * (1 - fr) + \
              (tex[r0 + 1, q0] * (1 - fq) + tex[r0 + 1, q0 + 1] * fq) * fr
        views.append(dense.View(np.rint(img).astype(np.float32), K, DIST, R, C, rays=rays))
    return views


def spread(ms):
    ms = sorted(ms)
    return 'median %.3f ms (min %.3f, max %.3f; %s)' % (ms[len(ms) // 2], ms[0], ms[-1],
                                                        ', '.join('%.3f' % m for m in ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=684)
    ap.add_argument('--height', type=int, default=456)
    ap.add_argument('--planes', type=int, default=64)
    ap.add_argument('--radius', type=int, default=3)
    ap.add_argument('--views', type=int, default=200)
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
    t0 = time.time()
    host = make_views(w, h)
    rays = kernels._dev(host[0].rays, torch.float64)
    G = kernels._dev(np.stack([v.G for v in host]), torch.float32)
    views = [dense.View(G[k], v.K, v.dist, v.R, v.C, rays=rays) for k, v in enumerate(host)]
    torch.cuda.synchronize()
    say('%d views of %d x %d rendered in %.1f s; %d planes, r = %d, 4 neighbours, depths 80 .. 125 m'
        % (len(views), w, h, time.time() - t0, D, r))
    w_far, w_near = 1.0 / 125.0, 1.0 / 80.0
    neighbours = [[j for j in range(5) if j != i] for i in range(5)]

    # ---- the sweep kernel alone ----
    out = [torch.empty((h, w), dtype=torch.int32, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev),
           torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w, 3), dtype=torch.float32, device=dev)]
    nb = torch.stack([views[j].G for j in neighbours[0]]).contiguous()
    pose = kernels._dev(kernels.dense_camera(views[0])[:12], torch.float64)
    cams = kernels._dev(np.stack([kernels.dense_camera(views[j]) for j in neighbours[0]]), torch.float64)
    L = _lib.lib()

    def launch():
        _lib.check(L.iamx_dense_sweep(kernels._ptr(views[0].G), kernels._ptr(rays), kernels._ptr(nb), kernels._ptr(pose),
                                      kernels._ptr(cams), w, h, 4, D, w_far, w_near, r, 4.0, 0.6, *[kernels._ptr(t) for t in out],
                                      _lib.stream_ptr()), 'iamx_dense_sweep')
    launch()
    torch.cuda.synchronize()
    kept = float(torch.isfinite(out[2]).float().mean())
    inner = (h - 2 * r) * (w - 2 * r)
    lds_bytes = inner * D * 4 * 3 * (2 * r + 1) * (r + 1) * 8 / 2.0
    times = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _k in range(LAUNCHES):
            launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / LAUNCHES)
    med = sorted(times)[len(times) // 2]
    say('sweep kernel, per reference image (%d launches per repeat): %s; %.2f of the pixels kept' % (LAUNCHES, spread(times), kept))
    say('  tap count: %d interior pixels x %d planes x 4 neighbours x %d B = %.2f GB of LDS reads = %.2f TB/s; '
        '%.2f G pixel-plane-neighbour steps/s'
        % (inner, D, 3 * (2 * r + 1) * (r + 1) * 4, lds_bytes / 1e9, lds_bytes / (med * 1e-3) / 1e12,
           inner * D * 4 / (med * 1e-3) / 1e9))

    # ---- depth_maps, the whole call ----
    ranges = [(80.0, 125.0)] * 5
    maps = dense.depth_maps(views, neighbours, ranges, planes=D, radius=r)
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        maps = dense.depth_maps(views, neighbours, ranges, planes=D, radius=r)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / 5.0)
    say('depth_maps, whole call over 5 views, per reference image: %s; %.2f of the pixels survive the check'
        % (spread(times), float(maps.keep.float().mean())))

    # ---- dense_check and fuse over many views ----
    V = max(5, args.views // 5 * 5)
    many = [views[k % 5] for k in range(V)]
    many_nb = [[5 * (k // 5) + j for j in neighbours[k % 5]] for k in range(V)]
    depth = maps.depth.repeat(V // 5, 1, 1).contiguous()
    keep = ned = None
    times = []
    for _ in range(args.repeats + 1):
        del keep, ned
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep, ned = kernels.dense_check(depth, many, many_nb)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    say('dense_check over %d views (call, with its uploads): %s' % (V, spread(times[1:])))
    big = dense.DepthMaps(depth=depth, keep=keep, ned=ned)
    times = []
    for _ in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        surface = dense.fuse(many, big, 0.25)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    H, W = surface.shape
    say('fuse over %d views, %d points into %d x %d cells at 0.25 m: %s'
        % (V, int(keep.sum()), W, H, spread(times[1:])))
    if log:
        log.close()


if __name__ == '__main__':
    main()
