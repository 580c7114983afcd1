#!/usr/bin/env python3
"""The true orthophoto's blend (ortho.render_dense(bands=), csrc/ortho_dsm.hip's owner and layer
passes, csrc/ortho_raster.hip's pyramid kernels) on the stand-in project of tools/ortho_dense_rate.py:
the recorded Step 5 scene step5_mid_default with synthetic frames of a quarter of the camera's size
and a synthetic DSM over the sparse mosaic's frame.

  * the whole ortho.render_dense(bands=B) call alternating with the whole
    ortho.render_dense(mode='best') call on the same project, frames and DSM, --repeats times each;
  * per image, by device events, the owner pass, the layer pass, the reduces and the accumulates of
    its pyramid, each beside a plain device copy that moves the same number of bytes (a copy of n
    bytes reads n and writes n): the median of --repeats launches.  Bytes counted per pixel of the
    work box and of its regions: owner 14 read + 14 written (metric, index, count: an upper bound, it
    writes only where it sees and wins); layer 4 read (index) + 16 written, plus the frame's taps, not
    counted; reduce 16 read per source pixel + 16 written per reduced pixel; accumulate 16 (layer) +
    16 (the coarser layer's pixels) + 16 (accumulator) read and 16 written.

No figure is a gate.  Every figure is given as median and spread (min .. max).  Real frames and
mosaics larger than the Infinity Cache are NOT measured here.

    python tools/ortho_dense_multiband_rate.py [--out profiles/r31_ortho_dense_multiband_rate.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def spread(xs):
    xs = sorted(xs)
    return '%.4g (min %.4g .. max %.4g, n=%d)' % (xs[len(xs) // 2], xs[0], xs[-1], len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--gsd', type=float, default=0.5, help='DSM cell, metres')
    ap.add_argument('--upsample', type=int, default=2)
    ap.add_argument('--bands', type=int, default=5)
    ap.add_argument('--images', type=int, default=8, help='images timed one by one')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import tempfile
    import torch
    import ortho_common as oc
    import step5_common as s5
    from imageanalysis_amd import _deps, dense, kernels, ortho
    from imageanalysis_amd import render_panda3d as rp
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd._lib import check, lib, stream_ptr

    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    clock = time.perf_counter
    g = oc.golden('step5_mid_default')
    work = tempfile.mkdtemp(prefix='ortho_dense_multiband_rate_')
    proj = s5.project(g, work)
    ref = getNode('/config/ned_reference', True)
    for k, v in (('lat_deg', 45.0), ('lon_deg', -93.0), ('alt_m', 280.0)):
        ref.setFloat(k, v)
    s5.set_switches(rp, g)
    names = list(g['groups'][0])
    h, w = g['height'] // 4, g['width'] // 4
    gen = torch.Generator(device='cuda').manual_seed(27)
    frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device='cuda', generator=gen) for _ in names]

    # the DSM over the sparse mosaic's frame (tools/ortho_dense_rate.py's)
    _names, grids, _uv, _w, _h = oc.scene_input('step5_mid_default')
    rf = ortho.raster_frame(grids, a.gsd)
    rng = np.random.default_rng(27)
    dsm = np.full((rf.H, rf.W), float(np.nanmean(grids[:, :, 2])), np.float32) + rng.normal(0, 0.2, (rf.H, rf.W)).astype(np.float32)
    for _ in range(12):
        r, c = rng.integers(0, rf.H - 20), rng.integers(0, rf.W - 30)
        dsm[r:r + 20, c:c + 30] += np.float32(rng.uniform(4, 12))
    surface = dense.Surface(torch.from_numpy(dsm).cuda(), torch.ones((rf.H, rf.W), dtype=torch.int32, device='cuda'),
                            rf.x0, rf.y1, a.gsd)
    say('true orthophoto, %d bands, on %s: %d images, frames %d x %d, DSM %d x %d cells at %.3f m, upsample %d: mosaic %d x %d'
        % (a.bands, torch.cuda.get_device_name(0), len(names), w, h, rf.W, rf.H, a.gsd, a.upsample, rf.W * a.upsample,
           rf.H * a.upsample))

    # ---- the whole calls, alternating ----
    quiet = io.StringIO()
    tb, tm = [], []
    for rep in range(a.repeats + 1):
        torch.cuda.synchronize()
        t = clock()
        with contextlib.redirect_stdout(quiet):
            best = ortho.render_dense(proj, g['groups'], 0, surface, mode='best', upsample=a.upsample, frames=frames)
        torch.cuda.synchronize()
        tb.append(clock() - t)
        t = clock()
        with contextlib.redirect_stdout(quiet):
            blend = ortho.render_dense(proj, g['groups'], 0, surface, upsample=a.upsample, frames=frames, bands=a.bands)
        torch.cuda.synchronize()
        tm.append(clock() - t)
    say('render_dense(mode=best), whole call, %d x %d pixels, %d frames shrunk: first %.4g s, then s: %s'
        % (best.shape[1], best.shape[0], ortho.render_dense_stats['prefiltered'], tb[0], spread(tb[1:])))
    say('render_dense(bands=%d), whole call, %d levels used: first %.4g s, then s: %s' % (a.bands, blend.bands, tm[0], spread(tm[1:])))
    say('index and count equal mode best\'s: %s; pixels whose colour differs: %.3f of the covered'
        % (bool(torch.equal(best.index, blend.index) and torch.equal(best.count.view(torch.int16), blend.count.view(torch.int16))),
           float(((best.bgr != blend.bgr).any(dim=2) & (best.index >= 0)).sum()) / max(int((best.index >= 0).sum()), 1)))
    del best, blend

    # ---- the kernels, per image (the frames at their full size) ----
    camera = _deps.camera()
    K = np.asarray(camera.get_K(optimized=True), np.float64)
    dist = np.array(camera.get_dist_coeffs(optimized=True), np.float64).ravel()[:5]
    width, height = camera.get_image_params()
    cams = [(K, width, height, dist) + tuple(dense.image_pose(proj.findImageByName(n))) for n in names]
    comp = ortho._DenseComposer(surface, 'best', a.upsample, None, names, a.bands, cams, [(h, w)] * len(names))
    L, p = lib(), kernels._ptr
    n = (comp.Ho, comp.Wo)
    metric = torch.empty(n, dtype=torch.float64, device='cuda')
    index = torch.empty(n, dtype=torch.int32, device='cuda')
    count = torch.empty(n, dtype=torch.uint16, device='cuda')
    bgr = torch.empty(n + (3,), dtype=torch.uint8, device='cuda')

    def timed(fn, moved, before=None):
        """-> (us of fn, us of a plain copy that moves `moved` bytes), --repeats each after one warm-up"""
        src = torch.empty(max(moved // 2, 1), dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(src)
        tk, tc = [], []
        for _ in range(a.repeats + 1):
            if before is not None:
                before()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            fn()
            e[1].record()
            e[2].record()
            dst.copy_(src)
            e[3].record()
            torch.cuda.synchronize()
            tk.append(e[0].elapsed_time(e[1]) * 1e3)
            tc.append(e[2].elapsed_time(e[3]) * 1e3)
        return spread(tk[1:]), spread(tc[1:])

    def clear():
        check(L.iamx_ortho_clear(0, comp.Ho, comp.Wo, p(metric), p(index), p(count), p(bgr), stream_ptr()), 'iamx_ortho_clear')

    for k in range(min(a.images, len(names))):
        plan = comp._mb_plan(k)
        if plan is None:
            say('image %d: an empty work box' % k)
            continue
        params, box, regions, _layers = plan
        areas = [ortho._area(r) for r in regions]
        stages = (
            ('owner', lambda: kernels.ortho_dsm_owner(comp.dsm, comp.ss, params, (h, w), k, box, metric, index, count),
             28 * areas[0], clear),
            ('layer', lambda: comp._mb_layer(k, frames[k], plan), 20 * areas[0], None),
            ('reduce', lambda: comp._mb_reduce(plan), 16 * sum(areas[:-1]) + 16 * sum(areas[1:]), None),
            ('accumulate', lambda: comp._mb_accumulate(plan), 48 * sum(areas) + 16 * sum(areas[1:]), None))
        say('image %d: box %d x %d = %d pixels, %d levels, %d pixels in all regions'
            % (k, box[2] - box[0] + 1, box[3] - box[1] + 1, areas[0], len(areas), sum(areas)))
        for what, fn, moved, before in stages:
            tk, tc = timed(fn, moved, before)
            say('  %-10s kernel us: %s; plain copy moving %.2f MB us: %s' % (what, tk, moved / 1e6, tc))
    s5.reset_switches(rp)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
