#!/usr/bin/env python3
"""Rate of the JPEG entropy decode on the device (iamx_jpeg_entropy_decode) against the host half
it replaces (iamx_jpeg_decode_coefficients on 1 and on 16 threads, plus the upload of the
coefficients it implies), alternating in one call on the same files: twelve
synth.make_survey_image frames (5472 x 3648) at quality 92, 4:2:0 and 4:2:2.

    python tools/jpeg_entropy_rate.py [--frames 12] [--rounds 3] [--repeat 3]

Device figures are device events around the launches (files, headers and buffers resident before
the clock starts); each timed window holds all frames `rounds` times.  For kernel times run the
same command with --device-only under `rocprofv3 --kernel-trace --stats`."""
import argparse
import ctypes
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from imageanalysis_amd import _lib, synth  # noqa: E402
from imageanalysis_amd.kernels import _ptr  # noqa: E402


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Frame(object):
    def __init__(self, L, dev, data):
        n = len(data)
        self.n = n
        self.raw = np.zeros((n + 15) // 16 * 16, np.uint8)
        self.raw[:n] = np.frombuffer(data, np.uint8)
        self.info = np.zeros(16, np.int32)
        self.quant = np.zeros((3, 64), np.uint16)
        self.header = np.zeros(int(L.iamx_jpeg_entropy_header_bytes()), np.uint8)
        _lib.check(L.iamx_jpeg_entropy_prepare(p(self.raw), n, p(self.info), p(self.quant), p(self.header),
                                               len(self.header)), 'iamx_jpeg_entropy_prepare')
        self.blocks = int(self.info[11])
        self.ws_bytes = int(L.iamx_jpeg_entropy_workspace_bytes(p(self.header)))
        self.scan_len = int(self.header[40:44].view(np.uint32)[0])
        self.subseq = int(self.header[52:56].view(np.int32)[0])
        self.n_subseq = int(self.header[44:48].view(np.int32)[0])
        self.d_raw = torch.from_numpy(self.raw).to(dev)
        self.d_header = torch.from_numpy(self.header).to(dev)


class Slot(object):
    """buffers of one frame in flight"""

    def __init__(self, dev, frames):
        self.stream = torch.cuda.Stream()
        self.ws = torch.empty(max(f.ws_bytes for f in frames), dtype=torch.uint8, device=dev)
        self.coef = torch.empty((max(f.blocks for f in frames), 64), dtype=torch.int16, device=dev)
        self.status = torch.zeros(4, dtype=torch.int32, device=dev)


def device_window(L, frames, slots, rounds, check=None):
    """all frames `rounds` times, round-robin over the slots' streams -> seconds per frame"""
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for s in slots:
        s.stream.wait_event(start)
    k = 0
    for _ in range(rounds):
        for f in frames:
            s = slots[k % len(slots)]
            k += 1
            _lib.check(L.iamx_jpeg_entropy_decode(_ptr(f.d_raw), f.raw.size, p(f.header), _ptr(f.d_header),
                                                  _ptr(s.ws), f.ws_bytes, _ptr(s.coef), f.blocks,
                                                  _ptr(s.status), ctypes.c_void_p(s.stream.cuda_stream)),
                       'iamx_jpeg_entropy_decode')
            if check is not None:
                s.stream.synchronize()
                check(f, s)
    for s in slots:
        torch.cuda.current_stream().wait_stream(s.stream)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e-3 / (rounds * len(frames))


def host_window(L, frames, bufs, threads, rounds):
    def one(args):
        f, buf = args
        quant = np.zeros((3, 64), np.uint16)
        rc = L.iamx_jpeg_decode_coefficients(p(f.raw), f.n, ctypes.c_void_p(buf.data_ptr()), f.blocks, p(quant))
        assert rc == 0
    t0 = time.perf_counter()
    if threads == 1:
        for _ in range(rounds):
            for f in frames:
                one((f, bufs[0]))
    else:
        with ThreadPoolExecutor(max_workers=threads) as pool:
            for _ in range(rounds):
                list(pool.map(one, [(f, bufs[k % len(bufs)]) for k, f in enumerate(frames)]))
    return (time.perf_counter() - t0) / (rounds * len(frames))


def upload_window(frames, buf, dev, rounds):
    d = torch.empty_like(buf, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        for f in frames:
            d[:f.blocks * 64].copy_(buf[:f.blocks * 64], non_blocking=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (rounds * len(frames))


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=12)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--device-only', action='store_true')
    a = ap.parse_args()
    dev = _lib.require_gpu()
    L = _lib.lib()
    images = [np.ascontiguousarray(synth.make_survey_image(seed=k).cpu().numpy()[:, :, ::-1]) for k in range(a.frames)]
    for sub, name in ((2, '4:2:0'), (1, '4:2:2')):
        def enc(img):
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, 'JPEG', quality=92, subsampling=sub)
            return buf.getvalue()
        with ThreadPoolExecutor(max_workers=12) as pool:
            datas = list(pool.map(enc, images))
        frames = [Frame(L, dev, d) for d in datas]
        f0 = frames[0]
        print('== %s: %d frames, file %.2f MB, scan %.2f MB, %d blocks (%.1f MB of coefficients), '
              'sub-sequences of %d bytes: %d lanes' % (name, len(frames), np.mean([f.n for f in frames]) / 1e6,
                                                      np.mean([f.scan_len for f in frames]) / 1e6, f0.blocks,
                                                      f0.blocks * 128 / 1e6, f0.subseq, f0.n_subseq))
        slots = [Slot(dev, frames) for _ in range(4)]
        stats = {'passes': [], 'status': [], 'decoded': []}

        def check(f, s):
            st = s.status.cpu().numpy()
            stats['status'].append(int(st[0]))
            stats['passes'].append(int(st[1]))
            stats['decoded'].append(int(st[2]) / float(f.n_subseq))
        device_window(L, frames, slots[:1], 1, check)                 # warm-up, and what became of each file
        refused = sum(1 for s in stats['status'] if s != 1)
        print('passes needed: max %d, mean %.1f; files not decoded on the device: %d of %d'
              % (max(stats['passes']), np.mean(stats['passes']), refused, len(frames)))
        # status[2] counts the sub-sequences the sync passes decoded; the write pass decodes each once more
        reads = np.mean(stats['decoded']) + 1.0
        print('bytes per frame: file in %.2f MB, coefficients out %.1f MB (+ %.1f MB cleared first), scan read '
              '%.2f times (sync passes %.2f, counted on the device, + the write pass): %.1f MB'
              % (f0.n / 1e6, f0.blocks * 128 / 1e6, f0.blocks * 128 / 1e6, reads, reads - 1.0,
                 reads * np.mean([f.scan_len for f in frames]) / 1e6))
        if a.device_only:
            for _ in range(a.repeat):
                print('device, 1 stream : %.3f ms/frame' % (1e3 * device_window(L, frames, slots[:1], a.rounds)))
                print('device, 4 streams: %.3f ms/frame' % (1e3 * device_window(L, frames, slots, a.rounds)))
            continue
        nval = max(f.blocks for f in frames) * 64
        bufs = [torch.empty(nval, dtype=torch.int16).pin_memory() for _ in range(16)]
        host_window(L, frames[:2], bufs, 1, 1)
        for r in range(a.repeat):
            d1 = device_window(L, frames, slots[:1], a.rounds)
            h1 = host_window(L, frames, bufs, 1, 1)
            d4 = device_window(L, frames, slots, a.rounds)
            h16 = host_window(L, frames, bufs, 16, a.rounds)
            up = upload_window(frames, bufs[0], dev, a.rounds)
            print('repeat %d: device 1 stream %.3f ms/frame (%.0f frames/s), 4 streams %.3f ms/frame (%.0f frames/s) | '
                  'host half 1 thread %.1f ms/frame (%.0f frames/s), 16 threads %.2f ms/frame (%.0f frames/s), '
                  'coefficient upload %.2f ms/frame'
                  % (r, d1 * 1e3, 1 / d1, d4 * 1e3, 1 / d4, h1 * 1e3, 1 / h1, h16 * 1e3, 1 / h16, up * 1e3))
        del slots, bufs, frames


if __name__ == '__main__':
    main()
