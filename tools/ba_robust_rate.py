#!/usr/bin/env python3
"""Robust loss on BASELINE configs[3] (synth.make_ba_problem): what the two kernels of
csrc/ba_robust.hip cost beside the residual / Jacobian kernels of the same problem, and what a
soft_l1 refine costs per TRF iteration beside the linear solve.

  kernels   iamx_ba_robust_scale (224 B read + 224 B written per observation) and iamx_ba_robust_cost
            (16 B read per observation) per call by device events, every loss, beside
            iamx_ba_residual_jac and iamx_ba_residual_prepared; GB/s against the plain device copy of
            the same bytes (iamx_hbm_copy16, the stream kernel of DESIGN.md section 4 K3) in the
            same run.  Every timed scale launch follows a fresh residual_jac (it works in place).
  solves    5 % of the observations displaced by 40-200 px; the linear solve from the synthetic
            start, then from ITS solution a linear and a soft_l1 (f_scale = 2) refine, alternating,
            `--repeats` times: outer iterations, seconds, iterations/s, inner iterations.

    python tools/ba_robust_rate.py [--launches 40] [--repeats 2] [--no-solves] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from imageanalysis_amd import _lib, ba_solver, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--launches', type=int, default=40)
ap.add_argument('--repeats', type=int, default=2)
ap.add_argument('--no-solves', action='store_true')
ap.add_argument('--out', default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


p = synth.make_ba_problem()
C, P, O = len(p['cams0']), len(p['pts0']), len(p['uv'])
K = p['K']
fixed = [K[0, 0], K[1, 1], K[0, 2], K[1, 2], *p['dist']]
rng = np.random.default_rng(7)
uv = np.array(p['uv'], np.float64)
bad = rng.choice(O, int(round(0.05 * O)), replace=False)
rad, ang = rng.uniform(40, 200, bad.size), rng.uniform(0, 2 * np.pi, bad.size)
uv[bad] += np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
x0 = np.hstack([p['cams0'].ravel(), p['pts0'].ravel()])
lb, ub = np.full(x0.size, -np.inf), np.full(x0.size, np.inf)
for j, dlt in ((0, 3.0), (1, 3.0), (2, 9.0)):
    lb[j:C * 7:7] = p['cams0'][:, j] - dlt
    ub[j:C * 7:7] = p['cams0'][:, j] + dlt
say('configs[3]: %d cameras, %d points, %d observations (%d displaced by 40-200 px)' % (C, P, O, bad.size))

prob = ba_solver.DeviceBA(C, P, p['cam_idx'], p['pt_idx'], uv, False, fixed_calib=fixed)
prob.set_x(x0)
L = _lib.lib()
V = prob.vec_ops()


def timed(fn, before=None, n=args.launches, warm=3):
    """mean and min..max of n launches by device events (`before` runs untimed in front of each)"""
    ts = []
    for k in range(warm + n):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warm:
            ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return ts.mean(), ts.min(), ts.max()


def row(name, t, nbytes):
    say('  %-44s %8.1f us (%.1f .. %.1f)  %7.1f MB  %6.0f GB/s' % (name, t[0], t[1], t[2], nbytes / 1e6,
                                                                   nbytes / t[0] / 1e3))


f_res, f_jac = prob.bound_launchers()
say('kernels, per call by device events, %d launches each:' % args.launches)
t_res = timed(f_res)
row('iamx_ba_residual_prepared', t_res, 64 * O)
t_jac = timed(f_jac)
row('iamx_ba_residual_jac', t_jac, 224 * O)
n16 = 224 * O // 16
src, dst = torch.empty(n16 * 2, dtype=torch.float64, device='cuda'), torch.empty(n16 * 2, dtype=torch.float64, device='cuda')
src.normal_()
t_copy = timed(lambda: L.iamx_hbm_copy16(_lib.c_void_p(src.data_ptr()), _lib.c_void_p(dst.data_ptr()), n16, 1, 1024,
                                         _lib.stream_ptr()))
row('iamx_hbm_copy16, the scale pass\'s bytes', t_copy, 448 * O)
del src, dst
slot = V._slot_ptr(0)
t_scale = {}
for loss, fs in (('soft_l1', 2.0), ('huber', 2.0), ('cauchy', 2.0), ('arctan', 2.0)):
    prob.loss, prob.f_scale = loss, fs
    t = timed(prob.robust_scale, before=f_jac)
    t_scale[loss] = t
    row('iamx_ba_robust_scale %s' % loss, t, 448 * O)
    t = timed(lambda: L.iamx_ba_robust_cost(ba_solver._ptr(prob.r), prob.m, ba_solver.LOSSES[loss], fs, slot,
                                            ba_solver._ptr(V.scratch), _lib.stream_ptr()), before=f_res)
    row('iamx_ba_robust_cost %s' % loss, t, 16 * O)
prob.loss, prob.f_scale = 'linear', 1.0
s = t_scale['soft_l1'][0]
say('  scale pass (soft_l1) = %.2f x residual_jac, %.2f x the copy of its bytes%s'
    % (s / t_jac[0], s / t_copy[0], ': longer than the Jacobian evaluation itself -- the case for fusing it'
       if s > t_jac[0] else ''))

if not args.no_solves:
    from threadpoolctl import threadpool_limits

    def solve(start, loss, fs):
        q = ba_solver.DeviceBA(C, P, p['cam_idx'], p['pt_idx'], uv, False, fixed_calib=fixed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ba_solver.trf_device(q, start, lb, ub, ftol=1e-4, loss=loss, f_scale=fs)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        say('  %-8s f_scale %-4g status %d, %3d outer iterations (nfev %d, njev %d) in %.3f s = %.1f it/s, inner '
            'iterations %d, cost %.6g' % (loss, fs, res.status, res.iterations, res.nfev, res.njev, dt,
                                          res.iterations / dt, sum(q.inner_iterations), res.cost))
        return res

    with threadpool_limits(limits=1, user_api='blas'):
        say('solves (inner solver: schur):')
        say(' from the synthetic start:')
        solve(x0, 'linear', 1.0)                     # (warms every kernel and the allocator)
        lin = solve(x0, 'linear', 1.0)
        cam_err = lambda x: float(np.sqrt(np.mean(np.sum((x[:C * 7].reshape(C, 7)[:, :3] - p['cams_true'][:, :3]) ** 2, 1))))
        say(' from the linear solution (rms camera position error against the truth %.3f m):' % cam_err(lin.x))
        for _ in range(args.repeats):
            a = solve(lin.x, 'linear', 1.0)
            b = solve(lin.x, 'soft_l1', 2.0)
        say(' rms camera position error: linear refine %.3f m, soft_l1 refine %.3f m' % (cam_err(a.x), cam_err(b.x)))

if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
