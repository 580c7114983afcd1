#!/usr/bin/env python3
"""Frames/s of imageanalysis_amd.panda3d.make_textures_opencv on 20 MP JPEGs (Step 5's textures):
N synth.make_survey_image frames (5472 x 3648, quality 92, rendered as tools/detect_rate.py renders
them) -> 512 x 512 textures in a fresh directory, with the worker seconds per stage (read, decode,
resize kernel, download, encode, write), the entropy decode on the host and on the device
ALTERNATING in one process, and a labelled single-thread host stand-in for the reference's loop.

    python tools/texture_rate.py N [--entropy host|device] [--repeats R] [--no-standin]

Without --entropy every repeat runs host then device.  The last lines time the resize kernel alone
(device events) beside a plain device read of the same 60 MB (iamx_hbm_copy16, four 16-byte reads
per 16-byte write) in the same process; under `rocprofv3 --kernel-trace --stats -- python
tools/texture_rate.py ...` the same kernels appear by name (area_kernel, hbm_copy16)."""
import argparse
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from imageanalysis_amd import _lib, kernels, panda3d, synth  # noqa: E402


class Img(object):
    def __init__(self, path):
        self.image_file = path
        self.name = os.path.splitext(os.path.basename(path))[0]


def stage(tmp, n):
    """n JPEG files from twelve rendered frames (the frames repeat; every file is its own decode)"""
    from PIL import Image as PILImage
    os.makedirs(os.path.join(tmp, 'images'))
    t0 = time.time()
    base = min(n, 12)
    with ThreadPoolExecutor(max_workers=12) as pool:           # (the encoder releases the interpreter)
        futs = []
        for k in range(base):
            bgr = synth.make_survey_image(seed=k).cpu().numpy()
            futs.append(pool.submit(PILImage.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save,
                                    os.path.join(tmp, 'images', 'D%04d.JPG' % k), quality=92))
        for f in futs:
            f.result()
    for k in range(base, n):
        shutil.copyfile(os.path.join(tmp, 'images', 'D%04d.JPG' % (k % base)),
                        os.path.join(tmp, 'images', 'D%04d.JPG' % k))
    print('%d synthetic 5472x3648 JPEGs (%d rendered) staged in %.1f s' % (n, base, time.time() - t0), flush=True)
    return [Img(os.path.join(tmp, 'images', 'D%04d.JPG' % k)) for k in range(n)]


def one_run(tmp, images, entropy, tag):
    an = os.path.join(tmp, 'analysis_' + tag)
    os.makedirs(an)
    panda3d.TEXTURE_ENTROPY = entropy
    before = {k: (dict(v) if isinstance(v, dict) else v) for k, v in panda3d.texture_stats.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    panda3d.make_textures_opencv(os.path.join(tmp, 'images'), an, images, resolution=512)
    dt = time.perf_counter() - t0
    st = panda3d.texture_stats
    made = st['made'] - before['made']
    split = {k: 1e3 * (st['stage_s'][k] - before['stage_s'][k]) / max(made, 1) for k in st['stage_s']}
    print('%-7s %-6s: %6.1f frames/s (%d textures in %.2f s, %d workers, %d decoded the host way); '
          'worker ms per frame: ' % (tag, entropy, made / dt, made, dt, panda3d.TEXTURE_WORKERS,
                                     st['host_decoded'] - before['host_decoded'])
          + ', '.join('%s %.2f' % (k, split[k]) for k in ('read', 'decode', 'resize', 'download', 'encode', 'write')),
          flush=True)
    shutil.rmtree(an)
    return made / dt


def host_standin(images, n):
    """single thread, host only: Pillow decode + BOX reduce, cv2 unavailable"""
    from PIL import Image as PILImage
    out = tempfile.mkdtemp(prefix='iamx_tex_host_')
    t0 = time.perf_counter()
    for im in images[:n]:
        with PILImage.open(im.image_file) as p:
            p.load()
            small = p.resize((512, 512), PILImage.BOX)
            small.save(os.path.join(out, im.name + '.JPG'), format='JPEG', quality=95, subsampling='4:2:0')
    dt = time.perf_counter() - t0
    shutil.rmtree(out)
    print('host stand-in (Pillow decode + BOX reduce, cv2 unavailable), one thread, %d frames: '
          '%.2f frames/s = %.0f ms per frame' % (n, n / dt, 1e3 * dt / n), flush=True)


def kernel_beside_read(images):
    """the resize kernel alone beside a plain device read of the frame's 60 MB, device events"""
    frame = kernels.jpeg_decode(images[0].image_file)
    h, w = int(frame.shape[0]), int(frame.shape[1])
    nbytes = frame.numel()
    n16 = nbytes // 64
    dst = torch.empty(n16 * 16, dtype=torch.uint8, device=frame.device)
    L = _lib.lib()

    # A launch returns before its kernel ends, and this kernel (tens of microseconds) is shorter than
    # the host's time to enqueue the next one: events around single launches would time the host's
    # enqueue gaps.  So the device is first given ~3 ms of other work (eight fills of 1 GiB); while it
    # works that off the host enqueues the whole series, and the events then lie between kernels that
    # run back to back.  The kernel trace of a rocprofv3 run is the check on these figures.
    ballast = torch.empty(1 << 30, dtype=torch.uint8, device=frame.device)

    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        for _ in range(8):
            ballast.zero_()
        ev[0].record()
        for k in range(reps):
            fn()
            ev[k + 1].record()
        torch.cuda.synchronize()
        ts = sorted(ev[k].elapsed_time(ev[k + 1]) for k in range(reps))
        return ts[len(ts) // 2], ts[0], ts[-1]

    def read():
        _lib.check(L.iamx_hbm_copy16(kernels._ptr(frame), kernels._ptr(dst), n16, 4, 2048, _lib.stream_ptr()),
                   'iamx_hbm_copy16')
    for res in (512, 64):
        out = torch.empty((res, res, 3), dtype=torch.uint8, device=frame.device)

        def resize():
            _lib.check(L.iamx_image_resize_area(kernels._ptr(frame), h, w, 3, res / float(w), res / float(h),
                                                kernels._ptr(out), _lib.stream_ptr()), 'iamx_image_resize_area')
        med, lo, hi = timed(resize)
        print('resize_area %dx%d -> %d: median %.1f us (min %.1f, max %.1f) = %.2f TB/s of source bytes'
              % (w, h, res, 1e3 * med, 1e3 * lo, 1e3 * hi, nbytes / (med * 1e-3) / 1e12), flush=True)
    med, lo, hi = timed(read)
    print('plain device read of the same %.1f MB (iamx_hbm_copy16, 4 reads per write, 2048 workgroups): '
          'median %.1f us (min %.1f, max %.1f) = %.2f TB/s read'
          % (nbytes / 1e6, 1e3 * med, 1e3 * lo, 1e3 * hi, n16 * 64 / (med * 1e-3) / 1e12), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('n', type=int, nargs='?', default=12)
    ap.add_argument('--entropy', choices=('host', 'device'))
    ap.add_argument('--repeats', type=int, default=1)
    ap.add_argument('--no-standin', action='store_true')
    ap.add_argument('--standin-frames', type=int, default=8)
    args = ap.parse_args()
    _lib.require_gpu()
    from imageanalysis_amd.hostlib import logger
    logger.log = lambda *a, **k: None                          # (two lines per file are not the measurement)
    tmp = tempfile.mkdtemp(prefix='iamx_tex_')
    try:
        images = stage(tmp, args.n)
        routes = (args.entropy,) if args.entropy else ('host', 'device')
        panda3d.TIME_STAGES = True
        for route in routes:                                   # first-touch costs of every worker thread
            one_run(tmp, images[:2 * panda3d.TEXTURE_WORKERS], route, 'warm')
        rates = {r: [] for r in routes}
        for rep in range(args.repeats):
            for route in routes:
                rates[route].append(one_run(tmp, images, route, 'run%d' % rep))
        for route in routes:
            r = sorted(rates[route])
            print('entropy %-6s: median %.1f frames/s, min %.1f, max %.1f over %d runs of %d frames'
                  % (route, r[len(r) // 2], r[0], r[-1], len(r), args.n), flush=True)
        print('device entropy decoder:', kernels.jpeg_device_stats, flush=True)
        if not args.no_standin:
            host_standin(images, min(args.standin_frames, args.n))
        kernel_beside_read(images)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
