#!/usr/bin/env python3
"""What the 'bruteforce' strategy (csrc/match_brute.hip, kernels.brute_pairs) costs.

  stages   4096 ordered pairs of 4096-row images out of one store of 64 images, each sharing 1500
           rows with the next one (descriptor noise +-6, a pixel shift, 0.6 px noise, kp.size within
           the size test).  Two pair lists: `strip` (every pair is an image and its successor: all
           pairs overlap) and `all-pairs` (every ordered pair of the 64 images: one in 64 overlaps,
           the shape of an all-pairs schedule).  Per list the stages of kernels.brute_pairs one by one
           through the C ABI, device events, one warm-up + three timed launches, mean and spread: the
           k = 3 search (iamx_knn3_l2_pairs), the cells (iamx_brute_bins), the consensus
           (iamx_verify_pairs, homography, over all n_pairs * 861 segments) at 256 and at 2048
           hypotheses, the walk (iamx_brute_select, behind the 2048-hypothesis masks); the share of
           the looked-at segments that lie in distance bins the early exit never reaches -- what a
           wave form of the consensus would not have to compute --; and how many pairs end with
           another list behind the 256-hypothesis masks.
  --e2e N  bench.e2e_bench(N)'s rendered survey: seconds of matcher.find_matches with
           strategy='traditional' and 'bestratio' and of matcher.bruteforce_matches, three calls each
           on emptied match lists.

The clock state is what `rocm-smi --showclocks` prints before and after (read only).

    python tools/brute_rate.py [--pairs 4096] [--rows 4096] [--e2e 512] [--out FILE]"""
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
ap.add_argument('--no-stages', action='store_true')
ap.add_argument('--out', default=None)
args = ap.parse_args()
lines = []
W_PX, H_PX, MIN_PAIRS, MATCH_RATIO = 5472, 3648, 25.0, 0.75
DIAG = int(np.sqrt(float(H_PX * H_PX + W_PX * W_PX)))
TOL, STEP_D = max(int(DIAG * 0.005), 5), int(DIAG * 0.55) / 40
NC = kernels.BRUTE_CELLS


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
    des, xy, size = [], [], []
    for i in range(n_img):
        d = sift_like(rng, n)
        p = np.stack([rng.uniform(600, W_PX - 600, n), rng.uniform(400, H_PX - 400, n)], 1)
        s = rng.uniform(2.0, 6.0, n)
        if i:
            d[:k] = np.clip(des[i - 1][k:2 * k].astype(int) + rng.integers(-6, 7, (k, 128)), 0, 255)
            p[:k] = xy[i - 1][k:2 * k] + [250.0, -120.0] + rng.normal(0, 0.6, (k, 2))
            s[:k] = size[i - 1][k:2 * k] * rng.uniform(0.9, 1.1, k)
        des.append(d)
        xy.append(np.clip(p, 0, [W_PX - 1, H_PX - 1]).astype(np.float32))
        size.append(s.astype(np.float32))
    return des, xy, size


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
    des, xy, size = survey(n_img, n, min(1500, n // 2 - 1))
    store = kernels.DescriptorStore.from_arrays(des)
    allxy = np.ascontiguousarray(np.concatenate(xy), np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kp_off, d_xy, d_key = up(np.arange(n_img, dtype=np.int64) * n), up(allxy), up(matcher.kp_key2(allxy))
    d_size = up(np.concatenate(size).astype(np.float32))
    strip = [(i % (n_img - 1), i % (n_img - 1) + 1) for i in range(args.pairs)]
    every = [(i, j) for i in range(n_img) for j in range(n_img) if i != j]
    every = [every[k % len(every)] for k in range(args.pairs)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for tag, pairs in (('strip', strip), ('all-pairs', every)):
        pairs = np.asarray(pairs, np.int32)
        n_p = len(pairs)
        t_knn, (idx, d2, out_off) = timed(lambda: kernels.knn3_pairs(store, pairs))
        total = int(out_off[-1])
        cap = 9 * total
        d_pairs, row_off = up(pairs), up(out_off)
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        bin_cnt, seg_cnt, flag = z32(n_p, NC), z32(n_p, NC), z32(2)
        seg_off = torch.zeros(n_p * NC + 1, dtype=torch.int64, device=dev)
        pts = torch.empty((cap, 4), dtype=torch.float32, device=dev)
        rows = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        t_bins, _ = timed(lambda: _lib.check(L.iamx_brute_bins(
            P(idx), P(d2), P(row_off), P(d_pairs), P(kp_off), P(d_xy), P(d_size), n_p, MATCH_RATIO, MIN_PAIRS,
            STEP_D, kernels.BRUTE_STEP_A, cap, P(bin_cnt), P(seg_cnt), P(seg_off), P(pts), P(rows), P(flag), st()),
            'iamx_brute_bins'))
        t_ver, masks = {}, {}
        for hyp in (256, 2048):
            t_ver[hyp], (mask, _m, _b, vstatus) = timed(
                lambda: kernels.verify_pairs(pts, seg_off, 'homography', float(TOL), hypotheses=hyp, seed=0))
            masks[hyp] = (mask, vstatus)
        stride, tab = n, kernels._tab_size(n)
        work = torch.empty(n_p * (6 * stride + 2 * tab), dtype=torch.int32, device=dev)
        slots = torch.empty((n_p, stride, 2), dtype=torch.int32, device=dev)
        cnt, chosen, stats, fit_cnt = z32(n_p), z32(n_p), z32(n_p, 4), z32(n_p, NC)
        off = torch.zeros(n_p + 1, dtype=torch.int64, device=dev)
        out_rows = torch.empty((total, 2), dtype=torch.int32, device=dev)
        select = lambda mask, vstatus: _lib.check(L.iamx_brute_select(
            P(d_pairs), P(kp_off), P(d_key), n_p, MIN_PAIRS, P(seg_cnt), P(seg_off), P(rows), P(mask), P(vstatus), cap,
            stride, tab, P(work), P(slots), P(cnt), P(off), P(out_rows), total, P(chosen), P(stats), P(fit_cnt),
            P(flag), st()), 'iamx_brute_select')
        select(*masks[256])
        few = (cnt.cpu().numpy().copy(), chosen.cpu().numpy().copy())
        t_sel, _ = timed(lambda: select(*masks[2048]))
        assert flag.cpu().tolist() == [0, 0]
        looked = seg_cnt > 0
        segs, reached = int(looked.sum()), int(stats[:, 3].sum())
        live_entries = int(seg_off[-1])
        # the entries of the segments in the distance bins the walk reached
        walked = stats[:, 2].cpu().numpy()
        sc = seg_cnt.cpu().numpy().reshape(n_p, kernels.BRUTE_DIST_BINS, kernels.BRUTE_ANGLE_BINS)
        in_walk = np.arange(kernels.BRUTE_DIST_BINS)[None, :] < walked[:, None]
        reached_entries = int((sc.sum(2) * in_walk).sum())
        say('%s: %d ordered pairs of %d-row images; %d of %d cells looked at, %d cell entries materialised; '
            '%d pairs with a result, %d matches' % (tag, n_p, n, segs, n_p * NC, live_entries,
                                                     int((cnt > 0).sum()), int(off[-1])))
        fmt = lambda t: '%9.2f ms (%.2f .. %.2f)' % (t.mean(), t.min(), t.max())
        say('  k = 3 search (knn3_pairs, tables and its sync included)  ' + fmt(t_knn))
        say('  cells (count, scan, fill in query-row order)             ' + fmt(t_bins))
        say('  consensus,  256 hypotheses, all looked-at cells          ' + fmt(t_ver[256]))
        say('  consensus, 2048 hypotheses, all looked-at cells          ' + fmt(t_ver[2048]))
        say('  walk (fitted counts, early exit, de-duplication, packing)' + fmt(t_sel))
        for hyp in (256, 2048):
            whole = t_knn.mean() + t_bins.mean() + t_ver[hyp].mean() + t_sel.mean()
            say('  sum at %4d hypotheses %.2f ms = %.2f us per pair; the consensus is %.0f %% of it, %.2f us per '
                'looked-at cell' % (hyp, whole, whole * 1e3 / n_p, 100 * t_ver[hyp].mean() / whole,
                                    t_ver[hyp].mean() * 1e3 / max(segs, 1)))
        say('  early exit: the walk reaches %d of the %d looked-at cells (%d of %d entries); %.1f %% of the cells and '
            '%.1f %% of the entries are consensus work it made unnecessary; distance bins walked per pair: mean %.1f'
            % (reached, segs, reached_entries, live_entries, 100.0 * (segs - reached) / max(segs, 1),
               100.0 * (live_entries - reached_entries) / max(live_entries, 1), float(walked.mean())))
        many = (cnt.cpu().numpy(), chosen.cpu().numpy())
        say('  256 against 2048 hypotheses: %d of %d pairs end with another list length (largest difference %d '
            'matches), %d with another cell; %d against %d matches in all'
            % (int((few[0] != many[0]).sum()), n_p, int(np.abs(few[0] - many[0]).max()),
               int((few[1] != many[1]).sum()), int(few[0].sum()), int(many[0].sum())))


class _Done(Exception):
    pass


def e2e(n_images):
    import bench
    names = ('traditional', 'bestratio', 'bruteforce')
    got = {k: [] for k in names}
    orig = matcher.find_matches

    def every(proj, K, **kw):
        for strategy in names:
            for _ in range(3):
                for im in proj.image_list:
                    im.match_list = {}
                torch.cuda.synchronize()
                t = time.perf_counter()
                if strategy == 'bruteforce':
                    matcher.bruteforce_matches(proj, K, sort=kw.get('sort', False))
                else:
                    orig(proj, K, **dict(kw, strategy=strategy))
                torch.cuda.synchronize()
                sec = time.perf_counter() - t
                hit = sum(len(v) > 0 for im in proj.image_list for v in im.match_list.values()) // 2
                tot = sum(len(v) for im in proj.image_list for v in im.match_list.values()) // 2
                tried = sum(len(im.match_list) for im in proj.image_list) // 2
                got[strategy].append((sec, tried, hit, tot))
        raise _Done()

    matcher.find_matches = every
    try:
        bench.e2e_bench(n_images)
    except _Done:
        pass
    finally:
        matcher.find_matches = orig
    say('rendered survey of bench.e2e_bench(%d), three calls each on emptied lists (find_matches; '
        'bruteforce_matches at %d hypotheses):' % (n_images, matcher.BRUTE_HYPOTHESES))
    for strategy in names:
        secs = np.array([g[0] for g in got[strategy]])
        _s, tried, hit, tot = got[strategy][-1]
        say('  %-12s %8.3f s (%.3f .. %.3f)   %d pairs tried, %d with matches, %d matches'
            % (strategy, secs.mean(), secs.min(), secs.max(), tried, hit, tot))


say('device: %s' % torch.cuda.get_device_name(0))
clocks('before')
if not args.no_stages:
    stages()
if args.e2e:
    e2e(args.e2e)
clocks('after')
if args.out:
    with open(args.out, 'a' if args.no_stages else 'w') as f:
        f.write('\n'.join(lines) + '\n')
