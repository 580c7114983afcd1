#!/usr/bin/env python3
"""Frames/s of imageanalysis_amd.ortho.render on a rendered survey (synth.make_rendered_survey: a
textured ground plane photographed from a lawn-mower grid, JPEG files on disk), as a stand-in
project: poses, camera, a matches_grouped of ground points, so the call runs everything a user's
call runs -- statistics, Delaunay, surface grids, JPEG decode on worker threads, prefilter,
rasteriser -- and ortho.save writes the tiles.

    python tools/ortho_rate.py [--rows R --cols C] [--full-frame] [--gsd G] [--repeats 3] [--out FILE]
                               [--mode M ...] [--bands B]

Per mode, `repeats` whole calls (frames/s by a host clock around the call, which ends in a device
synchronise).  Then the raster kernel alone, per image and by device events, beside a plain device
copy (iamx_hbm_copy16, one read per write) of the bytes that image's launch reads and writes in the
accumulators, alternating in the same process: best 27 bytes per covered pixel (metric read and
written, index, count read and written, bgr), feather 68 (four doubles and the count, read and
written).  The kernel's frame reads come on top and are not in the yardstick.

--mode (repeatable; default best and feather) names the modes that alternate.  With multiband among
them, per image the device-event times of its three stages -- the layer kernel, the reduce and
accumulate kernels of every level, and (once per mosaic, not per image) the collapse -- beside a
plain copy of the bytes they move: per pixel of the image's regions a 16-byte layer pixel written,
read by the reduce (below the top level) and read by the accumulate, and a 16-byte accumulator pixel
read and written; the collapse reads and writes 16 bytes per pixel of every level and writes bgr."""
import argparse
import contextlib
import io
import os
import pickle
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from imageanalysis_amd import _lib, kernels, ortho, synth  # noqa: E402
from imageanalysis_amd._deps import getNode  # noqa: E402
from imageanalysis_amd.hostlib import camera  # noqa: E402
from imageanalysis_amd.hostlib.image_pose import PoseProject  # noqa: E402

RMW_BYTES = {'best': 8 + 8 + 4 + 2 + 2 + 3, 'feather': 32 + 32 + 2 + 2}


def standin_project(tmp, rows, cols, full_frame, out):
    kw = dict(synth.FULL_FRAME) if full_frame else {}
    dev = torch.device('cuda', torch.cuda.current_device())
    t0 = time.time()
    names, truth, _logged, K = synth.make_rendered_survey(tmp, rows, cols, device=dev, **kw)
    w, h = (kw['w'], kw['h']) if full_frame else (1368, 912)
    print('%d rendered %d x %d JPEGs staged in %.1f s' % (len(names), w, h, time.time() - t0), file=out, flush=True)
    an = os.path.join(tmp, 'analysis')
    os.makedirs(an)
    proj = PoseProject(names, analysis_dir=an)
    for im, (ned, ypr) in zip(proj.image_list, truth):
        for opt in (False, True):
            im.set_camera_pose(ned.tolist(), ypr[0], ypr[1], ypr[2], opt=opt)
        im.image_file = os.path.join(tmp, 'images', im.name + '.JPG')
    node = getNode('/config/camera', True)
    node.__dict__.pop('K_opt', None)
    node.__dict__.pop('dist_coeffs_opt', None)
    for key in ('K', 'K_opt'):
        node.setLen(key, 9)
        for i, v in enumerate(K.reshape(-1).tolist()):
            node.setFloatEnum(key, i, v)
    camera.set_dist_coeffs([0.0] * 5)
    camera.set_dist_coeffs([0.0] * 5, optimized=True)
    camera.set_image_params(w, h)
    ref = getNode('/config/ned_reference', True)
    for k, v in (('lat_deg', 45.0), ('lon_deg', -93.0), ('alt_m', 280.0)):
        ref.setFloat(k, v)
    # ground points (NED z ~ 0) over the survey, each seen by two images: z_avg and the surface
    rng = np.random.default_rng(1)
    pos = np.array([t[0] for t in truth])
    lo, hi = pos[:, :2].min(axis=0) - 150.0, pos[:, :2].max(axis=0) + 150.0
    pts = lo + rng.random((4000, 2)) * (hi - lo)
    matches = [[[float(p[0]), float(p[1]), float(rng.normal(0, 0.05))], 0,
                [m % len(names), [0.0, 0.0]], [(m + 1) % len(names), [0.0, 0.0]]] for m, p in enumerate(pts)]
    with open(os.path.join(an, 'matches_grouped'), 'wb') as f:
        pickle.dump(matches, f)
    return proj, [names], (w, h)


def whole_call(proj, groups, gsd, mode, bands=5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        m = ortho.render(proj, groups, 0, gsd, mode=mode, bands=bands)
    torch.cuda.synchronize()
    return m, time.perf_counter() - t0


def _timed(launch, copy_bytes, ballast, reps):
    """-> (sorted ms of `launch`, sorted ms of a plain copy of copy_bytes), alternating"""
    L = _lib.lib()
    n16 = max(1, copy_bytes // 32)                       # half read, half written
    src = torch.empty(16 * n16, dtype=torch.uint8, device=ballast.device)
    dst = torch.empty_like(src)
    tk, tc = [], []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for _b in range(4):                              # (the host's enqueue gets ahead of the device)
            ballast.zero_()
        e[0].record()
        launch()
        e[1].record()
        e[2].record()
        _lib.check(L.iamx_hbm_copy16(kernels._ptr(src), kernels._ptr(dst), n16, 1, 2048, _lib.stream_ptr()))
        e[3].record()
        torch.cuda.synchronize()
        tk.append(e[0].elapsed_time(e[1]))
        tc.append(e[2].elapsed_time(e[3]))
    return sorted(tk), sorted(tc)


def multiband_times(proj, groups, gsd, bands, out, reps=7):
    """mode multiband's stages per image by device events, each beside a plain copy of its bytes"""
    images, grids, uv = ortho.group_grids(proj, groups, 0)
    width, height = camera.get_image_params()
    cells, _v = ortho.used_cells(grids)
    frames = []
    for im, g, c in list(zip(images, grids, cells))[:8]:
        f = kernels.jpeg_decode(im.image_file)
        frames.append(ortho.prepare_frame(f, im.name, g, c, gsd)[0])
    ballast = torch.empty(1 << 30, dtype=torch.uint8, device=frames[0].device)
    comp = ortho._Composer(grids, uv, width, height, gsd, 'multiband', bands=bands)
    line = ('multiband image %d (frame %d x %d, box %d x %d, %d levels): %-18s median %7.1f us (min %.1f, max %.1f), '
            '%.2f MB = %.2f TB/s; plain copy of the same bytes median %.1f us (min %.1f, max %.1f)')
    for k in range(len(frames)):
        plan = comp._mb_plan(k)
        if plan is None:
            continue
        _params, box, regions, _layers = plan
        areas = [ortho._area(r) for r in regions]
        stages = (('layer', lambda: comp._mb_layer(k, frames[k], plan), 16 * areas[0]),
                  ('reduce+accumulate', lambda: comp._mb_pyramid(plan), (16 + 32) * sum(areas) + 16 * sum(areas[:-1]) + 16 * sum(areas[1:])))
        comp._add_multiband(k, frames[k])                # warm-up
        for name, launch, nbytes in stages:
            tk, tc = _timed(launch, nbytes, ballast, reps)
            print(line % (k, frames[k].shape[1], frames[k].shape[0], box[2] - box[0] + 1, box[3] - box[1] + 1,
                          len(regions), name, 1e3 * tk[reps // 2], 1e3 * tk[0], 1e3 * tk[-1], nbytes / 1e6,
                          nbytes / (tk[reps // 2] * 1e-3) / 1e12, 1e3 * tc[reps // 2], 1e3 * tc[0], 1e3 * tc[-1]),
                  file=out, flush=True)
    nbytes = 32 * sum(h * w for h, w in comp.sizes) + (3 + 2 - 16) * comp.sizes[0][0] * comp.sizes[0][1]
    comp._mb_collapse()
    tk, tc = _timed(comp._mb_collapse, nbytes, ballast, reps)
    print('multiband collapse (mosaic %d x %d, %d levels, once per mosaic): median %7.1f us (min %.1f, max %.1f), %.2f MB '
          '= %.2f TB/s; plain copy of the same bytes median %.1f us (min %.1f, max %.1f)'
          % (comp.sizes[0][1], comp.sizes[0][0], len(comp.sizes), 1e3 * tk[reps // 2], 1e3 * tk[0], 1e3 * tk[-1],
             nbytes / 1e6, nbytes / (tk[reps // 2] * 1e-3) / 1e12, 1e3 * tc[reps // 2], 1e3 * tc[0], 1e3 * tc[-1]),
          file=out, flush=True)


def kernel_times(proj, groups, gsd, out, reps=7, modes=('best', 'feather')):
    """the raster kernel per image beside a plain copy of its accumulator bytes, alternating"""
    images, grids, uv = ortho.group_grids(proj, groups, 0)
    width, height = camera.get_image_params()
    cells, _v = ortho.used_cells(grids)
    frames = []
    for im, g, c in list(zip(images, grids, cells))[:8]:
        f = kernels.jpeg_decode(im.image_file)
        frames.append(ortho.prepare_frame(f, im.name, g, c, gsd)[0])
    L = _lib.lib()
    ballast = torch.empty(1 << 30, dtype=torch.uint8, device=frames[0].device)
    for mode in modes:
        comp = ortho._Composer(grids, uv, width, height, gsd, mode)
        rf = comp.rf

        def clear():
            _lib.check(L.iamx_ortho_clear(ortho.MODES[mode], rf.H, rf.W, kernels._ptr(comp.acc), kernels._ptr(comp.index),
                                          kernels._ptr(comp.count), kernels._ptr(comp.bgr), _lib.stream_ptr()))
        for k in range(len(frames)):                     # warm-up, and the covered pixels per image
            comp.add(k, frames[k])
        for k in range(len(frames)):
            clear()
            comp.add(k, frames[k])
            covered = int((comp.count.cpu().numpy() > 0).sum())
            nbytes = covered * RMW_BYTES[mode]
            n16 = max(1, nbytes // 32)                   # half read, half written
            src = torch.empty(16 * n16, dtype=torch.uint8, device=comp.dev)
            dst = torch.empty_like(src)
            tk, tc = [], []
            for _ in range(reps):
                clear()
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                for _b in range(4):                      # the device is given other work first, so that the
                    ballast.zero_()                      # host's enqueue is ahead of it (tools/texture_rate.py)
                e[0].record()
                comp.add(k, frames[k])
                e[1].record()
                e[2].record()
                _lib.check(L.iamx_hbm_copy16(kernels._ptr(src), kernels._ptr(dst), n16, 1, 2048, _lib.stream_ptr()))
                e[3].record()
                torch.cuda.synchronize()
                tk.append(e[0].elapsed_time(e[1]))
                tc.append(e[2].elapsed_time(e[3]))
            tk.sort()
            tc.sort()
            print('%-7s image %d (frame %d x %d): raster kernel median %7.1f us (min %.1f, max %.1f), %d covered pixels, '
                  '%.2f MB of accumulator traffic = %.2f TB/s; plain copy of the same bytes median %.1f us (min %.1f, '
                  'max %.1f)' % (mode, k, frames[k].shape[1], frames[k].shape[0], 1e3 * tk[reps // 2], 1e3 * tk[0],
                                 1e3 * tk[-1], covered, nbytes / 1e6, nbytes / (tk[reps // 2] * 1e-3) / 1e12,
                                 1e3 * tc[reps // 2], 1e3 * tc[0], 1e3 * tc[-1]), file=out, flush=True)


class Tee(object):
    def __init__(self, *files):
        self.files = files

    def write(self, s):
        for f in self.files:
            f.write(s)

    def flush(self):
        for f in self.files:
            f.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=3)
    ap.add_argument('--cols', type=int, default=8)
    ap.add_argument('--full-frame', action='store_true', help='5472 x 3648 frames (default: 1368 x 912)')
    ap.add_argument('--gsd', type=float, default=0.0, help='metres per pixel (default: 4 x the frames\' native gsd)')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', help='also write the lines to this file')
    ap.add_argument('--mode', action='append', choices=sorted(ortho.MODES),
                    help='a mode to run, repeatable: they alternate (default: best and feather)')
    ap.add_argument('--bands', type=int, default=5, help="multiband's pyramid levels")
    args = ap.parse_args()
    _lib.require_gpu()
    log = open(args.out, 'w') if args.out else None
    out = Tee(sys.stdout, log) if log else sys.stdout
    tmp = tempfile.mkdtemp(prefix='iamx_ortho_')
    try:
        proj, groups, (w, h) = standin_project(tmp, args.rows, args.cols, args.full_frame, out)
        native = (synth.FULL_FRAME['gsd'] if args.full_frame else 0.11)
        gsd = args.gsd or 4 * native
        n = len(groups[0])
        whole_call(proj, groups, gsd, 'best')                 # first-touch costs: worker threads, code objects
        modes = args.mode or ['best', 'feather']
        for rep in range(args.repeats):
            for mode in modes:
                m, dt = whole_call(proj, groups, gsd, mode, args.bands)
                H, W = m.shape
                print('run%d  %-9s: %6.1f frames/s whole call (%d frames of %d x %d in %.2f s, %d shrunk first; '
                      'mosaic %d x %d at %.3f m)' % (rep, mode, n / dt, n, w, h, dt, ortho.render_stats['prefiltered'],
                                                    W, H, gsd), file=out, flush=True)
        t0 = time.perf_counter()
        info = ortho.save(m, proj.analysis_dir, tile=2048, fmt='jpg')
        print('save: %d tiles and ortho.json in %.2f s (%s)' % (len(info['tiles']), time.perf_counter() - t0,
                                                                ', '.join(sorted(os.listdir(os.path.join(
                                                                    proj.analysis_dir, 'ortho')))[:4]) + ' ...'),
              file=out, flush=True)
        covered = float((m.count.cpu().numpy() > 0).mean())
        print('covered share of the mosaic %.2f, up to %d images over a pixel' % (covered, int(m.count.cpu().numpy().max())),
              file=out, flush=True)
        with contextlib.redirect_stdout(io.StringIO()):
            kernel_times(proj, groups, gsd, out, modes=[mode for mode in modes if mode != 'multiband'])
            if 'multiband' in modes:
                multiband_times(proj, groups, gsd, args.bands, out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        if log:
            log.close()


if __name__ == '__main__':
    main()
