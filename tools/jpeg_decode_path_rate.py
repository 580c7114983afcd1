#!/usr/bin/env python3
"""Frames/s of the JPEG decode path alone (file bytes -> BGR frame in HBM through the package's
python calls, no detection): kernels.jpeg_host_decode + jpeg_reconstruct against
kernels.jpeg_device_decode + jpeg_reconstruct on 1, 4 and 24 worker threads, each on its own
high-priority stream as image.prefetch's workers are, alternating on the same 96 frames
(twelve synth.make_survey_image frames, 5472 x 3648, quality 92, eight times over).

    python tools/jpeg_decode_path_rate.py"""
import io
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from imageanalysis_amd import kernels, synth  # noqa: E402

tls = threading.local()


def job(args):
    mode, data = args
    st = getattr(tls, 'stream', None)
    if st is None:
        st = tls.stream = torch.cuda.Stream(priority=-1)
    t0 = time.perf_counter()
    with torch.cuda.stream(st), kernels.polite_waits():
        jc = kernels.jpeg_device_decode(data) if mode == 'device' else kernels.jpeg_host_decode(data)
        t1 = time.perf_counter()
        kernels.jpeg_reconstruct(jc)
    return t1 - t0, time.perf_counter() - t1


def main():
    from PIL import Image

    def enc(img):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=92)
        return buf.getvalue()
    imgs = [np.ascontiguousarray(synth.make_survey_image(seed=k).cpu().numpy()[:, :, ::-1]) for k in range(12)]
    with ThreadPoolExecutor(12) as pool:
        datas = list(pool.map(enc, imgs)) * 8
    for nthr in (1, 4, 24):
        with ThreadPoolExecutor(nthr) as pool:
            for mode in ('device', 'host'):                          # first-touch costs of every thread
                list(pool.map(job, [(mode, d) for d in datas[:nthr * 2]]))
            for mode in ('host', 'device', 'host', 'device'):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = list(pool.map(job, [(mode, d) for d in datas]))
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print('%2d threads, entropy decode on the %-6s: %6.1f frames/s; in the worker per frame: '
                      'coefficients %.2f ms, reconstruction %.2f ms'
                      % (nthr, mode, len(datas) / dt, 1e3 * np.mean([a for a, b in r]),
                         1e3 * np.mean([b for a, b in r])), flush=True)


if __name__ == '__main__':
    main()
