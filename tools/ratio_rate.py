#!/usr/bin/env python3
"""What the 'bestratio' strategy (csrc/match_ratio.hip, kernels.ratio_pairs) costs.

  stages   4096 ordered pairs of 4096-row images out of one store of 64 images, each sharing 1500
           rows with the next one (descriptor noise +-6, a pixel shift, 0.6 px noise).  Two pair
           lists: `strip` (every pair is an image and its successor: all pairs overlap) and
           `all-pairs` (every ordered pair of the 64 images: one in 64 overlaps, the shape of an
           all-pairs schedule).  Per list the stages of kernels.ratio_pairs one by one through the
           C ABI, device events, one warm-up + three timed launches, mean and spread: the k = 2
           search (iamx_knn2_l2_pairs), the bins (iamx_ratio_bins), the consensus
           (iamx_verify_pairs, homography) at 256 and at 2048 hypotheses, the select stage
           (iamx_ratio_select, behind the 2048-hypothesis masks), and how many pairs end with another
           list behind the 256-hypothesis masks.
  --e2e N  bench.e2e_bench(N)'s rendered survey: seconds of matcher.find_matches with
           strategy='traditional' and with 'bestratio', three calls each on emptied match lists.

The clock state is what `rocm-smi --showclocks` prints before and after (read only).

    python tools/ratio_rate.py [--pairs 4096] [--rows 4096] [--e2e 512] [--out FILE]"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from imageanalysis_amd import _lib, kernels, matcher  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=4096)
ap.add_argument('--rows', type=int, default=4096)
ap.add_argument('--images', type=int, default=64)
ap.add_argument('--e2e', type=int, default=0)
ap.add_argument('--out', default=None)
args = ap.parse_args()
lines = []
W_PX, H_PX, TOL, MIN_PAIRS = 5472, 3648, 33, 25.0


def say(s):
    print(s, flush=True)
    lines.append(s)


def clocks(tag):
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30).stdout
        rows = [ln.strip() for ln in out.splitlines() if 'sclk' in ln or 'mclk' in ln]
        say('clock state %s: %s' % (tag, '; '.join(rows[:4]) if rows else 'rocm-smi printed no sclk / mclk line'))
    except Exception as exc:                      # noqa: BLE001
        say('clock state %s: not read (%s)' % (tag, exc))


def sift_like(rng, n):
    g = rng.gamma(0.6, 1.0, size=(n, 128))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g = np.minimum(g, 0.2)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return np.clip(np.rint(g * 512.0), 0, 255).astype(np.uint8)


def survey(n_img, n, k):
    rng = np.random.default_rng(61)
    des, xy = [], []
    for i in range(n_img):
        d = sift_like(rng, n)
        p = np.stack([rng.uniform(600, W_PX - 600, n), rng.uniform(400, H_PX - 400, n)], 1)
        if i:
            d[:k] = np.clip(des[i - 1][k:2 * k].astype(int) + rng.integers(-6, 7, (k, 128)), 0, 255)
            p[:k] = xy[i - 1][k:2 * k] + [250.0, -120.0] + rng.normal(0, 0.6, (k, 2))
        des.append(d)
        xy.append(np.clip(p, 0, [W_PX - 1, H_PX - 1]).astype(np.float32))
    return des, xy


def timed(fn, repeats=3):
    fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return np.array(ts), out


def stages():
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    n_img, n = args.images, args.rows
    des, xy = survey(n_img, n, min(1500, n // 2 - 1))
    store = kernels.DescriptorStore.from_arrays(des)
    allxy = np.ascontiguousarray(np.concatenate(xy), np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kp_off, d_xy, d_key = up(np.arange(n_img, dtype=np.int64) * n), up(allxy), up(matcher.kp_key2(allxy))
    strip = [(i % (n_img - 1), i % (n_img - 1) + 1) for i in range(args.pairs)]
    every = [(i, j) for i in range(n_img) for j in range(n_img) if i != j]
    every = [every[k % len(every)] for k in range(args.pairs)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = len(kernels.RATIO_CUTOFFS)
    cut = np.asarray(kernels.RATIO_CUTOFFS, np.float64)
    for tag, pairs in (('strip', strip), ('all-pairs', every)):
        pairs = np.asarray(pairs, np.int32)
        n_p = len(pairs)
        t_knn, (idx, d2, out_off) = timed(lambda: kernels.knn2_pairs(store, pairs))
        total = int(out_off[-1])
        cap = nb * total
        d_pairs, row_off = up(pairs), up(out_off)
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        bin_cnt, seg_cnt, flag = z32(n_p, nb), z32(n_p, nb), z32(2)
        seg_off = torch.zeros(n_p * nb + 1, dtype=torch.int64, device=dev)
        pts = torch.empty((cap, 4), dtype=torch.float32, device=dev)
        rows = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        t_bins, _ = timed(lambda: _lib.check(L.iamx_ratio_bins(
            P(idx), P(d2), P(row_off), P(d_pairs), P(kp_off), P(d_xy), n_p, nb, ctypes.c_void_p(cut.ctypes.data),
            MIN_PAIRS, cap, P(bin_cnt), P(seg_cnt), P(seg_off), P(pts), P(rows), P(flag), st()), 'iamx_ratio_bins'))
        t_ver, masks = {}, {}
        for hyp in (256, 2048):
            t_ver[hyp], (mask, _m, _b, vstatus) = timed(
                lambda: kernels.verify_pairs(pts, seg_off, 'homography', float(TOL), hypotheses=hyp, seed=0))
            masks[hyp] = (mask, vstatus)
        stride, tab = n, kernels._tab_size(n)
        work = torch.empty(n_p * (6 * stride + 2 * tab), dtype=torch.int32, device=dev)
        slots = torch.empty((n_p, stride, 2), dtype=torch.int32, device=dev)
        cnt, chosen, stats = z32(n_p), z32(n_p), z32(n_p, nb, 3)
        off = torch.zeros(n_p + 1, dtype=torch.int64, device=dev)
        out_rows = torch.empty((total, 2), dtype=torch.int32, device=dev)
        select = lambda mask, vstatus: _lib.check(L.iamx_ratio_select(
            P(d_pairs), P(kp_off), P(d_key), n_p, nb, MIN_PAIRS, kernels.RATIO_MIN_UNIQUE, P(bin_cnt), P(seg_cnt),
            P(seg_off), P(rows), P(mask), P(vstatus), cap, stride, tab, P(work), P(slots), P(cnt), P(off),
            P(out_rows), total, P(chosen), P(stats), P(flag), st()), 'iamx_ratio_select')
        select(*masks[256])
        few = (cnt.cpu().numpy().copy(), chosen.cpu().numpy().copy())
        t_sel, _ = timed(lambda: select(*masks[2048]))
        assert flag.cpu().tolist() == [0, 0]
        segs = int((seg_cnt > 0).sum())
        say('%s: %d ordered pairs of %d-row images; %d of %d bins looked at, %d bin entries materialised; '
            '%d pairs with a result, %d matches' % (tag, n_p, n, segs, n_p * nb, int(seg_off[-1]),
                                                     int((cnt > 0).sum()), int(off[-1])))
        fmt = lambda t: '%8.2f ms (%.2f .. %.2f)' % (t.mean(), t.min(), t.max())
        say('  k = 2 search (knn2_pairs, tables and its sync included)  ' + fmt(t_knn))
        say('  bins (count, scan, fill)                                 ' + fmt(t_bins))
        say('  consensus,  256 hypotheses                               ' + fmt(t_ver[256]))
        say('  consensus, 2048 hypotheses                               ' + fmt(t_ver[2048]))
        say('  select (inliers, unique counts, result, packing)         ' + fmt(t_sel))
        whole = t_knn.mean() + t_bins.mean() + t_ver[2048].mean() + t_sel.mean()
        say('  sum at 2048 hypotheses %.2f ms = %.2f us per pair; the consensus is %.0f %% of it'
            % (whole, whole * 1e3 / n_p, 100 * t_ver[2048].mean() / whole))
        many = (cnt.cpu().numpy(), chosen.cpu().numpy())
        say('  256 against 2048 hypotheses: %d of %d pairs end with another list length (largest difference %d '
            'matches), %d with another bin; %d against %d matches in all'
            % (int((few[0] != many[0]).sum()), n_p, int(np.abs(few[0] - many[0]).max()),
               int((few[1] != many[1]).sum()), int(few[0].sum()), int(many[0].sum())))


class _Done(Exception):
    pass


def e2e(n_images):
    import bench
    got = {'traditional': [], 'bestratio': []}
    orig = matcher.find_matches

    def both(proj, K, **kw):
        for strategy in ('traditional', 'bestratio'):
            for _ in range(3):
                for im in proj.image_list:
                    im.match_list = {}
                torch.cuda.synchronize()
                t = time.perf_counter()
                orig(proj, K, **dict(kw, strategy=strategy))
                torch.cuda.synchronize()
                sec = time.perf_counter() - t
                hit = sum(len(v) > 0 for im in proj.image_list for v in im.match_list.values()) // 2
                tot = sum(len(v) for im in proj.image_list for v in im.match_list.values()) // 2
                tried = sum(len(im.match_list) for im in proj.image_list) // 2
                got[strategy].append((sec, tried, hit, tot))
        raise _Done()

    matcher.find_matches = both
    try:
        bench.e2e_bench(n_images)
    except _Done:
        pass
    finally:
        matcher.find_matches = orig
    say('rendered survey of bench.e2e_bench(%d), matcher.find_matches, three calls each on emptied lists:' % n_images)
    for strategy in ('traditional', 'bestratio'):
        secs = np.array([g[0] for g in got[strategy]])
        _s, tried, hit, tot = got[strategy][-1]
        say('  %-12s %8.3f s (%.3f .. %.3f)   %d pairs tried, %d with matches, %d matches'
            % (strategy, secs.mean(), secs.min(), secs.max(), tried, hit, tot))


say('device: %s' % torch.cuda.get_device_name(0))
clocks('before')
stages()
if args.e2e:
    e2e(args.e2e)
clocks('after')
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
