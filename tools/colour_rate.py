#!/usr/bin/env python3
"""Frames/s of the pass over a survey's frames that makes the explorer's colour tables
(imageanalysis_amd.histogram / vignette) on 20 MP JPEGs: N synth.make_survey_image frames
(5472 x 3648, quality 92, staged as tools/texture_rate.py stages them), R repeats of

    histograms only      histogram.make_histograms          (decode, quarter image, histogram, 3 KB back)
    average only         vignette.average                   (decode, sum of 8 frames per launch, mean)
    both in one pass     vignette.average(histograms=True)  (one decode feeds both)

in one process, alternating, beside ONE host thread doing the reference's work with what is
installed: Pillow decode + oracle.image_oracle.resize_linear_u8 + three bincounts + a float32 add
(cv2 is unavailable).  The last lines time the kernels alone by device events, each on a decoded
20 MP frame: histogram (the frame and its quarter image), accumulate (1 and 8 frames per launch),
mean, radial moments, fitted mask, mask finish, look-up (with and without the mask).

    python tools/colour_rate.py [N] [--repeats R] [--standin-frames K]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from imageanalysis_amd import _lib, histogram, kernels, vignette  # noqa: E402
import texture_rate  # noqa: E402  (stage)


def host_standin(images, n):
    """one thread, host only: what the reference does per frame for BOTH tables, cv2 unavailable"""
    from oracle.image_oracle import resize_linear_u8
    from imageanalysis_amd import image
    total = None
    split = dict(decode=0.0, resize=0.0, bincount=0.0, add=0.0)
    clock = time.perf_counter
    t0 = clock()
    for im in images[:n]:
        t = clock()
        bgr = image._decode_bgr(im.image_file, writable=False)
        split['decode'] += clock() - t
        t = clock()
        small = resize_linear_u8(bgr, 0.25)
        split['resize'] += clock() - t
        t = clock()
        for c in range(3):
            np.bincount(small[:, :, c].ravel(), minlength=256).astype('float32')
        split['bincount'] += clock() - t
        t = clock()
        if total is None:
            total = np.zeros(bgr.shape, np.float32)
        total += bgr
        split['add'] += clock() - t
    dt = clock() - t0
    print('host stand-in (Pillow decode + resize_linear_u8 + bincount + float32 add, cv2 unavailable), one thread, '
          '%d frames: %.2f frames/s = %.0f ms per frame (' % (n, n / dt, 1e3 * dt / n)
          + ', '.join('%s %.0f' % (k, 1e3 * v / n) for k, v in split.items()) + ')', flush=True)


def kernel_times(images):
    """each kernel alone, device events between back-to-back launches (the scheme of
    tools/texture_rate.py: the device is given other work first, so the host's enqueue is ahead)"""
    frame = kernels.jpeg_decode(images[0].image_file)
    h, w = int(frame.shape[0]), int(frame.shape[1])
    dev = frame.device
    nbytes = frame.numel()
    ballast = torch.empty(1 << 30, dtype=torch.uint8, device=dev)

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

    def report(name, fn, moved):
        med, lo, hi = timed(fn)
        print('%-34s median %8.1f us (min %.1f, max %.1f) = %.2f TB/s of %.0f MB moved'
              % (name, 1e3 * med, 1e3 * lo, 1e3 * hi, moved / (med * 1e-3) / 1e12, moved / 1e6), flush=True)

    L = _lib.lib()
    P, S = kernels._ptr, _lib.stream_ptr
    ck = _lib.check
    small = kernels.equalize_resize(frame, 0.25, equalize=False)
    hist = torch.zeros((3, 256), dtype=torch.int32, device=dev)
    flat = torch.full_like(frame, 131)
    report('histogram, 20 MP frame', lambda: ck(L.iamx_colour_histogram(P(frame), h * w, P(hist), S())), nbytes)
    report('histogram, flat 20 MP frame', lambda: ck(L.iamx_colour_histogram(P(flat), h * w, P(hist), S())), nbytes)
    report('histogram, quarter image', lambda: ck(L.iamx_colour_histogram(
        P(small), small.shape[0] * small.shape[1], P(hist), S())), small.numel())
    total = torch.zeros((h, w, 3), dtype=torch.int32, device=dev)
    frames = [frame] + [torch.roll(frame, k, 1) for k in range(1, 8)]
    report('accumulate, 1 frame per launch', lambda: kernels.colour_accumulate(total, frames[:1]), 9 * nbytes)
    total.zero_()
    report('accumulate, 8 frames per launch', lambda: kernels.colour_accumulate(total, frames), 16 * nbytes)
    del frames
    avg = torch.empty_like(frame)
    report('mean', lambda: ck(L.iamx_colour_mean(P(total), total.numel(), 200, P(avg), S())), 5 * nbytes)
    import ctypes
    ws = torch.empty(int(L.iamx_colour_moments_workspace_doubles()), dtype=torch.float64, device=dev)
    out = torch.empty((3, 8), dtype=torch.float64, device=dev)
    R = ctypes.c_double(0.0)
    report('radial moments', lambda: ck(L.iamx_colour_moments(P(frame), h, w, w / 2.0 - 7.5, h / 2.0 + 4.25,
                                                              ctypes.byref(R), P(ws), P(out), S())), nbytes)
    coef = np.array([[-1.2e-14, -6.0e-6, 201.3], [-2.0e-14, -4.0e-6, 179.6], [0.5e-14, -8.0e-6, 150.2]])
    mask = torch.empty_like(frame)
    report('fitted mask', lambda: ck(L.iamx_colour_fit_mask(h, w, w / 2.0 - 7.5, h / 2.0 + 4.25,
                                                            coef.ctypes.data_as(ctypes.c_void_p), 1, P(mask), S())),
           nbytes)
    scratch = torch.empty(3, dtype=torch.int32, device=dev)
    fin = torch.empty_like(frame)
    report('mask finish (max + subtract)', lambda: ck(L.iamx_colour_mask_finish(P(mask), h * w, P(scratch), P(fin),
                                                                               S())), 3 * nbytes)
    lut = torch.from_numpy(np.tile(np.arange(255, -1, -1, dtype=np.uint8), (3, 1))).to(dev)
    report('look-up', lambda: ck(L.iamx_colour_lut(P(frame), h * w, P(lut), None, P(avg), S())), 2 * nbytes)
    report('look-up + mask', lambda: ck(L.iamx_colour_lut(P(frame), h * w, P(lut), P(fin), P(avg), S())), 3 * nbytes)


def one_run(images, mode):
    """seconds of one pass (the functions' own lines -- a name per frame -- are not the measurement)"""
    import contextlib
    import io
    histogram.histograms.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        if mode == 'histograms':
            histogram.make_histograms(images)
        else:
            vignette.average(images, histograms=(mode == 'both'))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('n', type=int, nargs='?', default=24)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--standin-frames', type=int, default=6)
    args = ap.parse_args()
    _lib.require_gpu()
    import shutil
    import tempfile
    tmp = tempfile.mkdtemp(prefix='iamx_colour_')
    try:
        images = texture_rate.stage(tmp, args.n)
        modes = ('histograms', 'average', 'both')
        rates = {m: [] for m in modes}
        workers = min(histogram.HISTOGRAM_WORKERS, len(images))
        for m in modes:                                        # first-touch costs of every worker thread
            one_run(images[:16], m)
        for rep in range(args.repeats):
            for m in modes:
                dt = one_run(images, m)
                rates[m].append(len(images) / dt)
                print('run%d  %-10s: %6.1f frames/s (%d frames in %.2f s, %d workers)'
                      % (rep, m, len(images) / dt, len(images), dt, workers), flush=True)
        for m in modes:
            r = sorted(rates[m])
            print('%-10s: median %.1f frames/s, min %.1f, max %.1f over %d runs of %d frames'
                  % (m, r[len(r) // 2], r[0], r[-1], len(r), args.n), flush=True)
        host_standin(images, min(args.standin_frames, args.n))
        kernel_times(images)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
