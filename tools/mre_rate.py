#!/usr/bin/env python3
"""Rate of the cull step (scripts/4b-mre-by-image.py) at BASELINE configs[3] / configs[4]
observation counts on synthetic scenes (imageanalysis_amd.synth, 2 % of the observations displaced
by 20-200 px):

  device   iamx_ba_residual (the yardstick), iamx_ba_reproj_stats (pass 1, e written) and
           iamx_ba_mark_outliers (pass 2), hipEvent medians; bytes per observation and the
           fraction of 8 TB/s they correspond to
  host     the (match, feature) mapping + ordering of the flagged observations, the Chains
           deletion (mask + numpy rebuild), and the in-process twin sequence on plain lists
           (Optimizer.setup, mre_by_image, mark_outliers, delete_marked_features)
  ref-form the reference's per-observation tabulation loop (4b-mre-by-image.py:72-102) on a
           subset of the cameras, extrapolated by observation count

    python tools/mre_rate.py [--configs 3,4] [--reps 20] [--out mre_rate.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from imageanalysis_amd import kernels, match_culling as cull, optimizer, synth  # noqa: E402
from imageanalysis_amd.hostlib import camera  # noqa: E402
from imageanalysis_amd.hostlib import transforms as tf  # noqa: E402
from imageanalysis_amd.hostlib.image_pose import PoseProject  # noqa: E402
from imageanalysis_amd.match_cleanup import Chains  # noqa: E402

CONFIGS = {3: dict(rows=38, cols=74, n_points=300000, n_obs=1960000),
           4: dict(rows=71, cols=141, n_points=780000, n_obs=5120000)}
HBM = 8.0e12


def ev_median(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def scene(cfg):
    prob = synth.make_ba_problem(**CONFIGS[cfg])
    rng = np.random.default_rng(9)
    uv = prob['uv'].copy()
    k = rng.choice(len(uv), len(uv) // 50, replace=False)
    ang, r = rng.uniform(0, 2 * np.pi, len(k)), rng.uniform(20, 200, len(k))
    uv[k, 0] += r * np.cos(ang)
    uv[k, 1] += r * np.sin(ang)
    prob['uv'] = uv
    return prob


def chains_of(prob):
    """point-major chains (chain p = point p) as Chains and as the list of lists"""
    P = len(prob['pts0'])
    order = np.argsort(prob['pt_idx'], kind='stable')
    pi = prob['pt_idx'][order]
    ptr = np.searchsorted(pi, np.arange(P + 1)).astype(np.int64)
    ch = Chains(prob['cam_idx'][order], prob['uv'][order], ptr)
    ch.ned[:] = prob['pts0']
    ch.has_ned[:] = True
    ch.group[:] = 0
    return ch


def project(prob):
    C = len(prob['cams0'])
    proj = PoseProject(['I%05d' % i for i in range(C)])
    K = np.asarray(prob['K'], float)
    camera.set_K(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    camera.set_dist_coeffs([0.0] * 5)
    camera.set_image_params(5472, 3648)
    for im, c in zip(proj.image_list, prob['cams0']):
        e = tf.euler_from_quaternion(c[3:7], 'rzyx')
        im.set_camera_pose(c[:3].tolist(), *[float(np.degrees(a)) for a in e])
    return proj, [[im.name for im in proj.image_list]]


def run(cfg, reps):
    out = dict(config=cfg)
    prob = scene(cfg)
    C, O = len(prob['cams0']), len(prob['cam_idx'])
    out.update(n_cameras=C, n_obs=O)
    dev = torch.device('cuda:0')
    K = np.asarray(prob['K'], float)
    calib = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0], np.float64)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
         for a in (prob['cams0'], prob['pts0'], prob['cam_idx'], prob['pt_idx'], prob['uv'], calib)]
    ptr = np.zeros(C + 1, np.int64)
    np.cumsum(np.bincount(prob['cam_idx'], minlength=C), out=ptr[1:])
    cam_ptr = torch.from_numpy(ptr).to(dev)
    st = {}

    def p1():
        st['r'] = kernels.ba_reproj_stats(*t, cam_ptr)

    def p2():
        kernels.ba_mark_outliers(st['r'][2], st['r'][1], 5.0)
    r_buf = torch.empty(2 * O, dtype=torch.float64, device=dev)
    for f in (p1, p2):
        f()
    torch.cuda.synchronize()
    t_res = ev_median(lambda: kernels.ba_residual(*t, out=r_buf), reps)
    t1 = ev_median(p1, reps)
    t2 = ev_median(p2, reps)
    b_res = 4 + 4 + 16 + 24 + 16          # idx, uv, gathered point, r written
    b1 = 4 + 4 + 16 + 24 + 8              # idx, uv, gathered point, e written
    b2 = 3 * 8                            # e read by the sq, count and scatter passes
    out['device'] = dict(
        residual_s=t_res, stats_s=t1, mark_s=t2,
        residual_bytes_per_obs=b_res, stats_bytes_per_obs=b1, mark_bytes_per_obs=b2,
        residual_frac_8TBps=b_res * O / t_res / HBM, stats_frac_8TBps=b1 * O / t1 / HBM,
        mark_frac_8TBps=b2 * O / t2 / HBM)

    # host: mapping + ordering of the flagged observations, Chains deletion
    ch = chains_of(prob)

    class _Rep(object):
        pass
    rep = _Rep()
    rep.e, rep.summary = st['r'][2], st['r'][1]
    rep.pt_idx, rep.cam_idx = prob['pt_idx'], prob['cam_idx']
    rep.camera_map_fwd = np.arange(C)
    rep.feat_map_rev = {i: i for i in range(len(prob['pts0']))}
    h0 = time.perf_counter()
    obs, err, _, _ = cull.flagged(rep, 5.0)
    h1 = time.perf_counter()
    fi = cull.observation_features(ch, rep.pt_idx[obs], rep.cam_idx[obs])
    h2 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        for m, f in zip(rep.pt_idx[obs].tolist(), fi.tolist()):
            cull.mark_feature(ch, m, f, 0.0)
        h3 = time.perf_counter()
        cull.delete_marked_features(ch, 3)
    h4 = time.perf_counter()
    out['host'] = dict(n_flagged=len(obs), flagged_fetch_sort_s=h1 - h0, mapping_s=h2 - h1,
                       mark_s=h3 - h2, chains_delete_s=h4 - h3)

    # the twin's sequence in process on plain lists (pickle load / dump not included)
    ch = chains_of(prob)
    rows = ch.rows()
    proj, groups = project(prob)
    with contextlib.redirect_stdout(io.StringIO()):
        e0 = time.perf_counter()
        opt = optimizer.Optimizer('/nonexistent')
        opt.setup(proj, groups, 0, rows, optimized=False)
        e1 = time.perf_counter()
        rep = cull.mre_by_image(opt, rows, proj=proj)
        e2 = time.perf_counter()
    # reference-form tabulation (before the marks: it reads the same rows) (4b-mre-by-image.py:72-102) on the
    # first cameras, extrapolated
    r = kernels.ba_residual(*t).cpu().numpy()
    sub = int(np.searchsorted(ptr, 50000))
    fmap = opt.feat_map_rev
    q0 = time.perf_counter()
    results, count = [], 0
    for i in range(sub):
        orig = opt.camera_map_fwd[i]
        for j in opt.by_camera_point_indices[i]:
            match = rows[fmap[j]]
            mi = 0
            for k, p in enumerate(match[2:]):
                if p[0] == orig:
                    mi = k
            e = r[count * 2:count * 2 + 2]
            results.append([np.linalg.norm(e), fmap[j], mi])
            count += 1
    q1 = time.perf_counter()
    sorted(results, key=lambda fields: fields[0], reverse=True)
    q2 = time.perf_counter()
    out['reference_form'] = dict(subset_obs=count, loop_s=q1 - q0, sort_s=q2 - q1,
                                 extrapolated_loop_s=(q1 - q0) * O / max(count, 1))
    with contextlib.redirect_stdout(io.StringIO()):
        e2b = time.perf_counter()
        n = cull.mark_outliers(rows, rep, 5.0)
        e3 = time.perf_counter()
        cull.delete_marked_features(rows, 3)
        e4 = time.perf_counter()
    out['twin_in_process'] = dict(setup_s=e1 - e0, mre_by_image_s=e2 - e1, mark_outliers_s=e3 - e2b,
                                  delete_s=e4 - e3, total_s=(e2 - e0) + (e4 - e2b), marked=n)

    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='3,4')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    kernels.require_gpu()
    res = [run(int(c), a.reps) for c in a.configs.split(',')]
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
