#!/usr/bin/env python3
"""What the 'smart' strategy (csrc/match_knn3.hip, csrc/match_smart.hip, kernels.smart_pairs,
matcher.smart_matches) costs.

  search   4096 ordered pairs of 4096-row images out of one store of 64 images, each sharing 1500
           rows with the next one (descriptor noise +-6, a pixel shift, 0.6 px noise): the k = 3 kernel
           (iamx_knn3_l2_pairs) beside the k = 2 kernel (iamx_knn2_l2_pairs) on the SAME launch
           tables, kernels alone (device events, one warm-up + five timed launches).
  passes   the same pairs through the pass loop of kernels.smart_pairs stage by stage through the C
           ABI, from a prediction that is the true shift turned by 3 degrees: per pass the pairs that
           take part and the time of iamx_smart_stats, of the consensus (iamx_verify_pairs, 2048
           hypotheses) and of iamx_smart_select (walk, de-duplication, the refit of the taken bin);
           the refit alone (iamx_homography_fit over every bin's inliers); passes per pair.
  fit      iamx_homography_fit against the float64 restatement, and that against its longdouble form,
           as transfer errors over the segment's points (4, 5, 81, 2049 points).
  strip    seconds of matcher.smart_matches on the 14-image strip of tests/golden (46 pairs, one after
           another), three calls on emptied match lists.

The clock state is what `rocm-smi --showclocks` prints before and after (read only).

    python tools/smart_rate.py [--pairs 4096] [--rows 4096] [--out FILE]"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
import torch  # noqa: E402

from imageanalysis_amd import _lib, kernels, matcher  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=4096)
ap.add_argument('--rows', type=int, default=4096)
ap.add_argument('--images', type=int, default=64)
ap.add_argument('--out', default=None)
args = ap.parse_args()
lines = []
W_PX, H_PX, TOL, MIN_PAIRS, MATCH_RATIO = 5472, 3648, 32, 25.0, 0.75
NB = len(kernels.SMART_CUTOFFS)


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
        s = rng.uniform(2.0, 3.2, n)
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


fmt = lambda t: '%8.2f ms (%.2f .. %.2f)' % (t.mean(), t.min(), t.max())
P = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


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
    pairs = np.asarray([(i % (n_img - 1), i % (n_img - 1) + 1) for i in range(args.pairs)], np.int32)
    n_p = len(pairs)
    # ---- the two searches on the same tables
    out_off = np.arange(n_p + 1, dtype=np.int64) * n
    wg = np.arange(n_p + 1, dtype=np.int32) * int(L.iamx_knn2_wg_per_pair(n))
    total = int(out_off[-1])
    d_pairs, d_wg, d_out, row_off = up(pairs), up(wg), up(out_off[:-1]), up(out_off)
    res = {}
    for k, fn in ((2, L.iamx_knn2_l2_pairs), (3, L.iamx_knn3_l2_pairs)):
        idx = torch.empty((total, k), dtype=torch.int32, device=dev)
        d2 = torch.empty((total, k), dtype=torch.int32, device=dev)
        t, _ = timed(lambda: _lib.check(fn(P(store.desc), P(store.norm_q), P(store.norm_t), P(store.img_off),
                                           P(store.img_n), P(d_pairs), P(d_wg), P(d_out), n_p, int(wg[-1]), P(idx),
                                           P(d2), st()), 'knn'), repeats=5)
        res[k] = (t, idx, d2)
    assert torch.equal(res[2][1], res[3][1][:, :2]) and torch.equal(res[2][2], res[3][2][:, :2])
    dist = 1e-9 * n_p * float(n) * n
    say('search: %d ordered pairs of %d-row images, one launch, kernels alone (columns 0-1 of k = 3 equal k = 2)' % (n_p, n))
    for k in (2, 3):
        say('  k = %d  %s   %.1f G distances / s' % (k, fmt(res[k][0]), dist / (res[k][0].mean() * 1e-3)))
    say('  k = 3 takes %.2f x the time of k = 2' % (res[3][0].mean() / res[2][0].mean()))
    # ---- the pass loop, stage by stage
    _t, idx, d2 = res[3]
    cap, stride = NB * total, n
    tab = kernels._tab_size(stride)
    a = np.radians(3.0)
    c, s, cx, cy = np.cos(a), np.sin(a), W_PX / 2.0, H_PX / 2.0
    turn = np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1.0]])
    H0 = np.array([[1, 0, 250.0], [0, 1, -120.0], [0, 0, 1.0]]).dot(turn)
    H = up(np.tile(H0.ravel(), (n_p, 1)))
    z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    bin_cnt, seg_cnt, flag = z32(n_p, NB), z32(n_p, NB), z32(2)
    seg_off = torch.zeros(n_p * NB + 1, dtype=torch.int64, device=dev)
    pts = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    rows = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    work = torch.empty(n_p * (6 * stride + 2 * tab), dtype=torch.int32, device=dev)
    slots = torch.empty((n_p, stride, 2), dtype=torch.int32, device=dev)
    best = up(np.tile(np.array([kernels.SMART_MIN_UNIQUE, 0], np.int32), (n_p, 1)))
    improved, cnt, fit_status, stats = z32(n_p), z32(n_p), z32(n_p), z32(n_p, NB, 3)
    off = torch.zeros(n_p + 1, dtype=torch.int64, device=dev)
    out_rows = torch.empty((total, 2), dtype=torch.int32, device=dev)
    active = torch.ones(n_p, dtype=torch.int32, device=dev)
    passes = np.zeros(n_p, np.int64)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    say('passes: the same pairs from a prediction 3 degrees off, consensus at 2048 hypotheses')
    tot = np.zeros(4)
    k = 0
    while True:
        e = [ev() for _ in range(5)]
        e[0].record()
        _lib.check(L.iamx_smart_stats(P(idx), P(d2), P(row_off), P(d_pairs), P(kp_off), P(d_xy), P(d_size), P(H),
                                      P(active), n_p, MATCH_RATIO, MIN_PAIRS, cap, P(bin_cnt), P(seg_cnt), P(seg_off),
                                      P(pts), P(rows), P(flag), st()), 'iamx_smart_stats')
        e[1].record()
        mask, model, _b, vstatus = kernels.verify_pairs(pts, seg_off, 'homography', float(TOL), hypotheses=2048, seed=0)
        e[2].record()
        _lib.check(L.iamx_smart_select(P(d_pairs), P(kp_off), P(d_key), P(active), n_p, MIN_PAIRS, P(bin_cnt),
                                       P(seg_cnt), P(seg_off), P(pts), P(rows), P(mask), P(vstatus), P(model), cap,
                                       stride, tab, P(work), P(best), P(improved), P(slots), P(cnt), P(off),
                                       P(out_rows), total, P(stats), P(H), P(fit_status), P(flag), st()),
                   'iamx_smart_select')
        e[3].record()
        Hall, _s = kernels.homography_fit(pts, seg_off, mask)
        e[4].record()
        e[4].synchronize()
        ms = np.array([e[i].elapsed_time(e[i + 1]) for i in range(4)])
        act = active.cpu().numpy() > 0
        passes[act] += 1
        took = improved.cpu().numpy() > 0
        k += 1
        say('  pass %d: %4d pairs, %4d bins looked at, %8d bin entries; stats %7.2f ms, consensus %8.2f ms, '
            'select + refit %6.2f ms (%4d pairs gained); the refit of EVERY bin alone %6.2f ms'
            % (k, int(act.sum()), int((seg_cnt > 0).sum()), int(seg_off[-1]), ms[0], ms[1], ms[2], int(took.sum()), ms[3]))
        tot += ms
        if not took.any() or k > 16:
            break
        active.copy_(torch.from_numpy(took.astype(np.int32)))
    assert flag.cpu().tolist() == [0, 0]
    whole = tot[:3].sum()
    say('  all passes: stats %.2f ms (%.0f %%), consensus %.2f ms (%.0f %%), select + refit %.2f ms (%.0f %%); '
        '%.2f us per pair beside %.2f us of the k = 3 search'
        % (tot[0], 100 * tot[0] / whole, tot[1], 100 * tot[1] / whole, tot[2], 100 * tot[2] / whole,
           whole * 1e3 / n_p, res[3][0].mean() * 1e3 / n_p))
    say('  passes per pair: mean %.2f, largest %d; %d pairs with a result, %d matches'
        % (passes.mean(), passes.max(), int((cnt > 0).sum()), int(off[-1])))


def fit_figures():
    import smart_reference as sr
    say('fit: iamx_homography_fit against the float64 restatement, that against its longdouble form (transfer error, px)')
    for n, seed in ((4, 41), (5, 42), (81, 45), (2049, 43)):
        pts = sr.vr.scene(n, 1.0, 0.0, seed)[0]
        H, status = kernels.homography_fit(pts, [0, n])
        H64, _a = sr.fit(pts)
        Hld, _b = sr.fit(pts, dtype=np.longdouble)
        say('  n = %4d: device vs float64 %.3g, float64 vs longdouble %.3g (allowed: 64 x that, floor 1e-9)'
            % (n, sr.transfer_error(H.cpu().numpy()[0], H64, pts), sr.transfer_error(H64, Hld, pts)))


def strip():
    from test_match_smart import strip_project
    g, s, proj, _loop = strip_project(device=True)
    secs = []
    for _ in range(3):
        for im in proj.image_list:
            im.match_list = {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        matcher.smart_matches(proj, None, sort=False)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t)
    hit = sum(len(v) > 0 for im in proj.image_list for v in im.match_list.values()) // 2
    tried = sum(len(im.match_list) for im in proj.image_list) // 2
    say('strip: matcher.smart_matches on the 14-image strip, three calls on emptied lists: the first (uploads, '
        'first launches) %.3f s, then %.3f s and %.3f s; %d pairs one after another, %d with matches = %.1f ms per pair'
        % (secs[0], secs[1], secs[2], tried, hit, 1e3 * min(secs[1:]) / max(tried, 1)))


say('device: %s' % torch.cuda.get_device_name(0))
clocks('before')
stages()
fit_figures()
strip()
clocks('after')
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
