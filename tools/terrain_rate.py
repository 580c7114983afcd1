#!/usr/bin/env python3
"""Rates of the terrain module (profiles/r20_terrain_rate.txt), three repeats of each:

  device (needs the GPU):
    rays      10 000 images x 81 rays against a 201 x 201 terrain: iamx_terrain_rays alone (device
              events, inputs resident) and the whole srtm.intersect call with upload and download
    heights   srtm.heights for 10 000 cameras: the kernel alone and the whole call
  host:
    init      srtm.initialize(ref, 6000, 6000, 30) on one tile written from a seed
  reference (needs IAMX_REFERENCE=<checkout>, runs on the host):
    lib.srtm.interpolate_vectors on 2 000 of the same rays, extrapolated to 810 000, and
    SRTM.parse + make_lla_interpolator on the same tile

    python tools/terrain_rate.py [device] [host] [reference]
"""
import contextlib
import io
import os
import socket
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, 'tests'), HERE]
import terrain_common as tc                                      # noqa: E402

IMAGES, STEPS, REPEATS, REF_RAYS = 10000, 8, 3, 2000
REF_LLA = [45.3, -93.6, 280.0]


def scene():
    """a 6000 x 6000 m terrain at 30 m (201 x 201) and 10 000 nadir-ish cameras 120 m above it"""
    rng = np.random.default_rng(20)
    axis = np.linspace(-3000.0, 3000.0, 201)
    nn, ee = np.meshgrid(axis, axis, indexing='ij')
    grid = 280.0 + 25.0 * np.sin(nn / 400.0) + 18.0 * np.cos(ee / 300.0)
    ned = np.zeros((IMAGES, 3))
    ned[:, :2] = rng.uniform(-2500.0, 2500.0, (IMAGES, 2))
    ned[:, 2] = -(280.0 + 25.0 * np.sin(ned[:, 0] / 400.0) + 18.0 * np.cos(ned[:, 1] / 300.0) + 120.0)
    IK = np.linalg.inv(np.array([[3666.0, 0, 2736.0], [0, 3666.0, 1824.0], [0, 0, 1.0]]))
    M = np.empty((IMAGES, 3, 3))
    for i in range(IMAGES):
        yaw, roll, pitch = rng.uniform(0, 2 * np.pi), rng.normal(0, 0.05), rng.normal(0, 0.05)
        cy, sy, cr, sr, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch)
        R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]).dot(
            np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])).dot(np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]]))
        M[i] = R.dot(IK)
    uv = np.array([[u, v] for v in np.linspace(0, 3648, STEPS + 1) for u in np.linspace(0, 5472, STEPS + 1)])
    return axis, grid, M, ned, uv


def device():
    import torch
    from imageanalysis_amd import kernels, srtm
    from imageanalysis_amd.kernels import F64, U8, _dev, _ptr, check, lib, stream_ptr
    axis, grid, M, ned, uv = scene()
    print('device: %s, %d images x %d rays = %d rays, terrain %d x %d' % (
        torch.cuda.get_device_name(0), IMAGES, len(uv), IMAGES * len(uv), len(axis), len(axis)))
    srtm.adopt(srtm.GridInterpolator((axis, axis), grid))
    T = srtm.ned_interp.device()
    Md, nd, uvd = _dev(M, F64).reshape(-1, 9), _dev(ned, F64), _dev(uv, F64)
    pts = torch.empty((IMAGES, len(uv), 3), dtype=F64, device=Md.device)
    iters = torch.empty((IMAGES, len(uv)), dtype=U8, device=Md.device)
    flags = torch.empty_like(iters)

    def launch():
        check(lib().iamx_terrain_rays(*T._args(), _ptr(Md), _ptr(nd), IMAGES, _ptr(uvd), len(uv), _ptr(pts),
                                      _ptr(iters), _ptr(flags), stream_ptr()), 'iamx_terrain_rays')
    launch()
    torch.cuda.synchronize()
    for r in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        print('rays     kernel            repeat %d  %9.3f ms' % (r, a.elapsed_time(b)))
    it = iters.cpu().numpy()
    print('rays     rounds per ray: mean %.2f max %d; flagged %d' % (it.mean(), it.max(), int((flags != 0).sum())))
    srtm.intersect(M[:16], ned[:16], uv)
    for r in range(REPEATS):
        t = time.perf_counter()
        srtm.intersect(M, ned, uv)
        print('rays     intersect (whole) repeat %d  %9.3f ms' % (r, 1e3 * (time.perf_counter() - t)))
    q = _dev(ned[:, :2], F64)
    z = torch.empty(IMAGES, dtype=F64, device=q.device)
    for r in range(REPEATS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        check(lib().iamx_terrain_heights(*T._args(), _ptr(q), IMAGES, _ptr(z), stream_ptr()), 'iamx_terrain_heights')
        b.record()
        torch.cuda.synchronize()
        if r:
            print('heights  kernel            repeat %d  %9.3f ms' % (r - 1, a.elapsed_time(b)))
    for r in range(REPEATS):
        t = time.perf_counter()
        srtm.heights(ned[:, :2])
        print('heights  whole call        repeat %d  %9.3f ms' % (r, 1e3 * (time.perf_counter() - t)))


def host():
    from imageanalysis_amd import srtm
    print('host: %s' % socket.gethostname())
    cache = tempfile.mkdtemp(prefix='iamx_terrain_rate_')
    tc.write_tile(cache, 'N45W094', 3)
    srtm.default_cache_dir = cache
    for r in range(REPEATS):
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            srtm.initialize(REF_LLA, 6000, 6000, 30)
        print('init     mirror initialize (one tile, 201 x 201)  repeat %d  %9.3f ms' % (r, 1e3 * (time.perf_counter() - t)))
    return cache


def reference(cache):
    import scipy
    import scipy.interpolate
    import gen_terrain_golden as gen
    from imageanalysis_amd.render_panda3d import unit_rays
    ref = gen.import_reference_srtm()
    print('reference: scripts/lib/srtm.py on the CPU of %s, SciPy %s' % (socket.gethostname(), scipy.__version__))
    axis, grid, M, ned, uv = scene()
    ref.ned_interp = scipy.interpolate.RegularGridInterpolator((axis, axis), grid, bounds_error=False, fill_value=-32768)
    images = REF_RAYS // len(uv) + 1
    rays = [(ned[i].tolist(), unit_rays(M[i], uv)) for i in range(images)]
    for r in range(REPEATS):
        t = time.perf_counter()
        n = 0
        for p, v in rays:
            ref.interpolate_vectors(p, v)
            n += len(v)
        dt = time.perf_counter() - t
        print('rays     lib.srtm.interpolate_vectors, %d rays  repeat %d  %9.3f ms = %.3f ms per ray; %d rays: %.0f s' % (
            n, r, 1e3 * dt, 1e3 * dt / n, IMAGES * len(uv), dt / n * IMAGES * len(uv)))
    for r in range(REPEATS):
        with contextlib.redirect_stdout(io.StringIO()):
            tile = ref.SRTM(REF_LLA[0], REF_LLA[1], '../srtm')
            tile.set_srtm_cache_dir(cache)
            t = time.perf_counter()
            tile.parse()
            tile.make_lla_interpolator()
            dt = time.perf_counter() - t
        print('init     lib.srtm parse + make_lla_interpolator (one tile)  repeat %d  %9.3f ms' % (r, 1e3 * dt))


def main():
    what = sys.argv[1:] or ['device', 'host']
    cache = None
    if 'device' in what:
        device()
    if 'host' in what or 'reference' in what:
        cache = host()
    if 'reference' in what:
        reference(cache)
    if cache:
        import shutil
        shutil.rmtree(cache, ignore_errors=True)


if __name__ == '__main__':
    main()
