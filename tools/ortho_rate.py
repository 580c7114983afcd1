#!/usr/bin/env python3
"""Frames/s of imageanalysis_amd.ortho.render on a rendered survey (synth.make_rendered_survey: a
textured ground plane photographed from a lawn-mower grid, JPEG files on disk), as a stand-in
project: poses, camera, a matches_grouped of ground points, so the call runs everything a user's
call runs -- statistics, Delaunay, surface grids, JPEG decode on worker threads, prefilter,
rasteriser -- and ortho.save writes the tiles.

    python tools/ortho_rate.py [--rows R --cols C] [--full-frame] [--gsd G] [--repeats 3] [--out FILE]

Per mode, `repeats` whole calls (frames/s by a host clock around the call, which ends in a device
synchronise).  Then the raster kernel alone, per image and by device events, beside a plain device
copy (iamx_hbm_copy16, one read per write) of the bytes that image's launch reads and writes in the
accumulators, alternating in the same process: best 27 bytes per covered pixel (metric read and
written, index, count read and written, bgr), feather 68 (four doubles and the count, read and
written).  The kernel's frame reads come on top and are not in the yardstick."""
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


def whole_call(proj, groups, gsd, mode):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        m = ortho.render(proj, groups, 0, gsd, mode=mode)
    torch.cuda.synchronize()
    return m, time.perf_counter() - t0


def kernel_times(proj, groups, gsd, out, reps=7):
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
    for mode in ('best', 'feather'):
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
        for rep in range(args.repeats):
            for mode in ('best', 'feather'):
                m, dt = whole_call(proj, groups, gsd, mode)
                H, W = m.shape
                print('run%d  %-7s: %6.1f frames/s whole call (%d frames of %d x %d in %.2f s, %d shrunk first; '
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
            kernel_times(proj, groups, gsd, out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        if log:
            log.close()


if __name__ == '__main__':
    main()
