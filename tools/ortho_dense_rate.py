#!/usr/bin/env python3
"""The true orthophoto (ortho.render_dense, csrc/ortho_dsm.hip) on a stand-in project: the recorded
Step 5 scene step5_mid_default (30 images, poses, camera and sparse grids of tests/golden) with
synthetic frames of a quarter of the camera's size and a synthetic DSM over the sparse mosaic's frame
(the grids' mean height, rough ground and a few blocks that cast shadows):

  * iamx_ortho_dsm_image alone, per image, modes best and feather, by device events, into cleared
    accumulators: the median of --repeats launches beside a plain device copy of the same accumulator
    bytes of the image's work box (17 B per pixel in mode best, 37 in mode feather, read and written),
    the yardstick of profiles/r15_ortho_rate.txt;
  * the whole ortho.render_dense call (work boxes, uploads, launches) alternating with the whole
    ortho.render(mode='best') call on the same project and frames, --repeats times each.

No figure is a gate.  Every figure is given as median and spread (min .. max).  Real frames, the bias
default and DSMs larger than the Infinity Cache are NOT measured here.

    python tools/ortho_dense_rate.py [--out profiles/r27_ortho_dense_rate.txt]
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
    ap.add_argument('--gsd', type=float, default=0.5, help='DSM cell and sparse mosaic pixel, metres')
    ap.add_argument('--upsample', type=int, default=2)
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
    work = tempfile.mkdtemp(prefix='ortho_dense_rate_')
    proj = s5.project(g, work)
    with open(os.path.join(work, 'matches_grouped'), 'wb') as f:
        f.write(g['matches_in'])
    ref = getNode('/config/ned_reference', True)
    for k, v in (('lat_deg', 45.0), ('lon_deg', -93.0), ('alt_m', 280.0)):
        ref.setFloat(k, v)
    s5.set_switches(rp, g)
    names = list(g['groups'][0])
    h, w = g['height'] // 4, g['width'] // 4
    gen = torch.Generator(device='cuda').manual_seed(27)
    frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device='cuda', generator=gen) for _ in names]

    # the DSM over the sparse mosaic's frame
    _names, grids, _uv, _w, _h = oc.scene_input('step5_mid_default')
    rf = ortho.raster_frame(grids, a.gsd)
    rng = np.random.default_rng(27)
    dsm = np.full((rf.H, rf.W), float(np.nanmean(grids[:, :, 2])), np.float32) + rng.normal(0, 0.2, (rf.H, rf.W)).astype(np.float32)
    for _ in range(12):
        r, c = rng.integers(0, rf.H - 20), rng.integers(0, rf.W - 30)
        dsm[r:r + 20, c:c + 30] += np.float32(rng.uniform(4, 12))
    surface = dense.Surface(torch.from_numpy(dsm).cuda(), torch.ones((rf.H, rf.W), dtype=torch.int32, device='cuda'),
                            rf.x0, rf.y1, a.gsd)
    say('true orthophoto on %s: %d images, frames %d x %d, DSM %d x %d cells at %.3f m (%.1f MB), upsample %d: mosaic %d x %d'
        % (torch.cuda.get_device_name(0), len(names), w, h, rf.W, rf.H, a.gsd, dsm.nbytes / 1e6, a.upsample,
           rf.W * a.upsample, rf.H * a.upsample))

    # ---- the kernel alone ----
    camera = _deps.camera()
    K = np.asarray(camera.get_K(optimized=True), np.float64)
    dist = np.array(camera.get_dist_coeffs(optimized=True), np.float64).ravel()[:5]
    width, height = camera.get_image_params()
    L, p = lib(), kernels._ptr
    for mode in ortho.DENSE_MODES:
        comp = ortho._DenseComposer(surface, mode, a.upsample, None, names)
        per_pixel = 2 * ortho.BYTES_PER_PIXEL[mode]
        for k in range(min(a.images, len(names))):
            im = proj.findImageByName(names[k])
            R, C = dense.image_pose(im)
            Ks = dense.scaled_K(K, width, height, w, h)
            box = comp.box(Ks, dist, R, C, w, h)
            params = kernels.ortho_dsm_params(comp.x0, comp.y1, comp.gsd, comp.bias, comp.z_hi, Ks, dist, R, C)
            pixels = max(box[2] - box[0] + 1, 0) * max(box[3] - box[1] + 1, 0)
            src = torch.empty(max(pixels * per_pixel // 2, 1), dtype=torch.uint8, device='cuda')
            dst = torch.empty_like(src)
            tk, tc = [], []
            for _ in range(a.repeats + 1):
                check(L.iamx_ortho_clear(ortho.MODES[mode], comp.Ho, comp.Wo, p(comp.acc), p(comp.index), p(comp.count),
                                         p(comp.bgr), stream_ptr()), 'iamx_ortho_clear')
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record()
                kernels.ortho_dsm_image(ortho.MODES[mode], comp.dsm, comp.ss, params, frames[k], k, box, comp.acc,
                                        comp.index, comp.count, comp.bgr)
                e[1].record()
                e[2].record()
                dst.copy_(src)
                e[3].record()
                torch.cuda.synchronize()
                tk.append(e[0].elapsed_time(e[1]) * 1e3)
                tc.append(e[2].elapsed_time(e[3]) * 1e3)
            seen = int((comp.count.view(torch.int16) != 0).sum())
            say('%-7s image %d: box %d x %d = %d pixels, %d seen; kernel us: %s; plain copy of %.2f MB (read + written) us: %s'
                % (mode, k, box[2] - box[0] + 1, box[3] - box[1] + 1, pixels, seen, spread(tk[1:]),
                   pixels * per_pixel / 1e6, spread(tc[1:])))

    # ---- the whole calls, alternating ----
    quiet = io.StringIO()
    td, ts = [], []
    for rep in range(a.repeats + 1):
        torch.cuda.synchronize()
        t = clock()
        with contextlib.redirect_stdout(quiet):
            md = ortho.render_dense(proj, g['groups'], 0, surface, mode='best', upsample=a.upsample, frames=frames)
        torch.cuda.synchronize()
        td.append(clock() - t)
        t = clock()
        with contextlib.redirect_stdout(quiet):
            ms = ortho.render(proj, g['groups'], 0, a.gsd / a.upsample, mode='best', frames=frames)
        torch.cuda.synchronize()
        ts.append(clock() - t)
    say('render_dense(mode=best), whole call, %d x %d pixels, %d frames shrunk: first %.4g s, then s: %s'
        % (md.shape[1], md.shape[0], ortho.render_dense_stats['prefiltered'], td[0], spread(td[1:])))
    say('render(mode=best) over the sparse grids, whole call, %d x %d pixels, %d frames shrunk: first %.4g s, then s: %s'
        % (ms.shape[1], ms.shape[0], ortho.render_stats['prefiltered'], ts[0], spread(ts[1:])))
    say('covered share: dense %.3f, sparse %.3f' % (float((md.index >= 0).float().mean()), float((ms.index >= 0).float().mean())))
    s5.reset_switches(rp)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
