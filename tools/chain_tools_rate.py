#!/usr/bin/env python3
"""The two chain tools run between optimiser passes (3c-match-triangulation --method triangulate,
4b-colocated-feats) and the keypoint undistortion on one synthetic survey of BASELINE config 4's
shape (synth.make_ba_problem: 10 000 nadir images on a lawn-mower grid, 300 k chains, about 5 M
members, a lens with distortion):

  * each of the three kernels of csrc/chain_geom.hip alone, device-resident arguments, by device
    events between back-to-back launches;
  * the whole Python call (match_cleanup.triangulate_rays, match_culling.colocated_features on the
    array-backed Chains, undistort.undistort_points on every member): per-image matrices on the
    host, upload, kernel, download, write-back;
  * the numpy loop restatements of tests/chain_tools_common.py and tests/undistort_restatement.py on
    the same host, on --loop-chains chains, EXTRAPOLATED to the survey by members (triangulate,
    undistort) or by member pairs (colocated) and labelled so.  The restatements loop per member and
    per pair as the reference's scripts do, but they are NOT the reference: its loop also makes a
    cv2 call and two property-tree pose reads per member, and it is not what is timed here.

Every figure is taken --repeats times; the text gives the median and the spread (min .. max).

    python tools/chain_tools_rate.py [--out profiles/r13_chain_tools_rate.txt]
"""
import argparse
import os
import sys
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

DIST = (-0.12, 0.083, -0.0016, -0.00096, -0.012)


def spread(xs):
    xs = sorted(xs)
    return '%.4g (min %.4g .. max %.4g, n=%d)' % (xs[len(xs) // 2], xs[0], xs[-1], len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=100)
    ap.add_argument('--cols', type=int, default=100)
    ap.add_argument('--points', type=int, default=300000)
    ap.add_argument('--obs', type=int, default=5120000)
    ap.add_argument('--loop-chains', type=int, default=300)
    ap.add_argument('--min-angle', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import chain_tools_common as ct
    import undistort_restatement as ur
    from imageanalysis_amd import _lib, match_cleanup, synth, undistort
    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd.hostlib import camera
    from imageanalysis_amd.hostlib.image_pose import PoseProject

    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    clock = time.perf_counter
    t = clock()
    prob = synth.make_ba_problem(rows=a.rows, cols=a.cols, n_points=a.points, n_obs=a.obs, dist=DIST)
    order = np.argsort(prob['pt_idx'], kind='stable')
    img = prob['cam_idx'][order].astype(np.int32)
    uv = prob['uv'][order]
    counts = np.bincount(prob['pt_idx'], minlength=len(prob['pts_true']))
    ptr = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=ptr[1:])
    n, total, C = len(counts), len(img), len(prob['cams_true'])
    pairs = int((counts * (counts - 1) // 2).sum())
    K = prob['K']
    camera.set_K(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    camera.set_K(K[0, 0], K[1, 1], K[0, 2], K[1, 2], optimized=True)
    camera.set_dist_coeffs(list(DIST))
    camera.set_dist_coeffs(list(DIST), optimized=True)
    names = ['IMG_%05d' % i for i in range(C)]
    proj = PoseProject(names)
    for im, cam in zip(proj.image_list, prob['cams_true']):
        for opt in (False, True):
            im.set_camera_pose(cam[:3].tolist(), 0.0, 0.0, 0.0, opt=opt)
            node = im.node.getChild('camera_pose_opt' if opt else 'camera_pose', True)
            for k in range(4):
                node.setFloatEnum('quat', k, float(cam[3 + k]))
    group_list = [names]
    chains = match_cleanup.Chains(img, uv, ptr)
    chains.group[:] = 0
    chains.ned[:] = prob['pts0']
    chains.has_ned[:] = True
    say('chain tools on a synthetic survey: %d images, %d chains, %d members (%.1f per chain, longest %d), '
        '%d member pairs (%s; built in %.1f s)' % (C, n, total, total / n, counts.max(), pairs,
                                                    torch.cuda.get_device_name(0), clock() - t))

    # the whole Python calls
    t_tri, t_colo, t_und = [], [], []
    for rep in range(a.repeats + 1):
        t = clock()
        res = match_cleanup.triangulate_rays(proj, chains, group_list, 0, attitude='optimized')
        t_tri.append(clock() - t)
        t = clock()
        marks = cull.colocated_features(proj, chains, group_list, 0, a.min_angle)
        t_colo.append(clock() - t)
        t = clock()
        und = undistort.undistort_points(uv, K, DIST)
        t_und.append(clock() - t)
    assert chains.untouched()
    err = np.linalg.norm(chains.ned - prob['pts_true'], axis=1)
    say('whole Python call (first call apart: library load, allocator):')
    say('    triangulate_rays        first %.4g s, then s: %s' % (t_tri[0], spread(t_tri[1:])))
    say('        %d chains written, %d below the ground plane; against the true points: median %.3g m, max %.3g m'
        % (len(res.written), len(res.below), np.median(err), err.max()))
    say('    colocated_features      first %.4g s, then s: %s   (%d marks at %.3g degrees)'
        % (t_colo[0], spread(t_colo[1:]), len(marks), a.min_angle))
    say('    undistort_points        first %.4g s, then s: %s   (%d points)' % (t_und[0], spread(t_und[1:]), total))

    # the kernels alone
    sc_arrays = match_cleanup.chain_arrays(chains)
    IK = np.linalg.inv(K)
    M = np.array([im.get_body2ned(opt=True).dot(ct.CAM2BODY).dot(IK).ravel() for im in proj.image_list])
    pos = prob['cams_true'][:, :3].copy()
    k4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    d5 = np.array(DIST)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()          # noqa: E731
    d_ptr, d_img, d_uv, d_group, d_ned, d_M, d_pos = (dev(x) for x in (
        sc_arrays[0], sc_arrays[1], sc_arrays[2], sc_arrays[3], sc_arrays[4], M, pos))
    d_in = torch.ones(C, dtype=torch.uint8, device='cuda')
    d_status = torch.empty(n, dtype=torch.int32, device='cuda')
    d_count = torch.empty(total, dtype=torch.int32, device='cuda')
    d_total = torch.empty(1, dtype=torch.int64, device='cuda')
    d_uv32 = dev(uv.astype(np.float32))
    d_out32 = torch.empty_like(d_uv32)
    P = lambda x: _lib.c_void_p(x.data_ptr())                                 # noqa: E731
    H = lambda x: x.ctypes.data_as(_lib.c_void_p)                             # noqa: E731
    L = _lib.lib()
    launches = {
        'iamx_chain_triangulate': lambda: L.iamx_chain_triangulate(
            P(d_ptr), P(d_img), P(d_uv), P(d_group), n, 0, P(d_M), P(d_pos), P(d_in), C, H(k4), H(d5),
            P(d_ned), P(d_status), _lib.stream_ptr()),
        'iamx_chain_pair_angles': lambda: L.iamx_chain_pair_angles(
            P(d_ptr), P(d_img), P(d_group), P(d_ned), n, 0, P(d_pos), P(d_in), C, a.min_angle,
            P(d_count), P(d_total), P(d_status), _lib.stream_ptr()),
        'iamx_undistort_points': lambda: L.iamx_undistort_points(
            P(d_uv32), total, H(k4), H(d5), P(d_out32), _lib.stream_ptr()),
    }
    work = {'iamx_chain_triangulate': (total, 'members'), 'iamx_chain_pair_angles': (pairs, 'pairs'),
            'iamx_undistort_points': (total, 'points')}
    say('kernels alone (device events, back-to-back launches, first launch dropped):')
    for name, launch in launches.items():
        ts = []
        for _ in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(launch(), name)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 1e3)
        med = sorted(ts[1:])[len(ts[1:]) // 2]
        say('    %-24s s: %s = %.3g %s/s' % (name, spread(ts[1:]), work[name][0] / med, work[name][1]))
    assert int(d_total.item()) == len(marks)
    assert torch.equal(d_out32.cpu(), torch.from_numpy(und.astype(np.float32)))

    # the numpy loop restatements on a subset
    pick = np.linspace(0, n - 1, min(a.loop_chains, n)).astype(int)
    rows = [[chains.ned[c].tolist(), 0] + [[int(i), p] for i, p in zip(img[ptr[c]:ptr[c + 1]].tolist(),
                                                                      uv[ptr[c]:ptr[c + 1]].tolist())]
            for c in pick.tolist()]
    sub_members = int(counts[pick].sum())
    sub_pairs = int((counts[pick] * (counts[pick] - 1) // 2).sum())
    sc = types.SimpleNamespace(K=K, dist=d5, M=M, pos=pos, in_group=np.ones(C, np.uint8), group_index=0)
    r_tri, r_colo, r_und = [], [], []
    for _ in range(a.repeats):
        t = clock()
        ct.triangulate_restatement(sc, rows)
        r_tri.append(clock() - t)
        t = clock()
        ct.pair_angles_restatement(sc, rows, a.min_angle)
        r_colo.append(clock() - t)
        t = clock()
        for row in rows:
            for m in row[2:]:
                ur.undistort_points(np.array([m[1]], np.float32), K, d5)
        r_und.append(clock() - t)
    say('numpy loop restatements on this host (one thread), %d chains = %d members, %d pairs; NOT the '
        "reference's loop:" % (len(rows), sub_members, sub_pairs))
    for label, ts, have, whole, unit in (('triangulate', r_tri, sub_members, total, 'members'),
                                         ('pair angles', r_colo, sub_pairs, pairs, 'pairs'),
                                         ('undistort, a call per point', r_und, sub_members, total, 'points')):
        say('    %-28s measured s: %s; EXTRAPOLATED by %s to the survey s: %s'
            % (label, spread(ts), unit, spread([x * whole / have for x in ts])))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
