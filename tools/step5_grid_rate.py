#!/usr/bin/env python3
"""The grid stage of Step 5 (render_panda3d.build_map: rays of every image against the Delaunay
surface) three ways on one synthetic survey of BASELINE config 4's shape (synth.make_step5_scene:
300 k surface points, 10 000 nadir poses with a few degrees of jitter, 81 rays per image):

  (a) the device path build_map takes (render_panda3d.surface_grids) on a FRESH Delaunay object per
      repeat, as build_map has it, split into Delaunay on the host (qhull), its barycentric
      transforms (scipy computes them on first access), seed grid on the host, upload + record
      packing, kernel, download;
  (b) the reference's loop form -- one scipy LinearNDInterpolator call per look-up -- on
      --loop-images images, EXTRAPOLATED to the survey and labelled so;
  (c) the vectorised host form: one batched LinearNDInterpolator call per iteration round over all
      rays still iterating, on --batched-images images (EXTRAPOLATED when fewer than the survey);

(b) and (c) evaluate through scipy on a triangulation whose transforms are already computed, so the
triangulation (qhull + transforms) is common to all three forms and reported once; the text ends with
the whole grid stage of each form, triangulation included.  Then the .egg writer (panda3d.generate_from_grid, textures stubbed) per 1 000 files.  Every figure is
taken --repeats times; the text gives the median and the spread (min .. max).

    python tools/step5_grid_rate.py [--out profiles/r11_step5_grid_rate.txt]
"""
import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs):
    xs = sorted(xs)
    return '%.4g (min %.4g .. max %.4g, n=%d)' % (xs[len(xs) // 2], xs[0], xs[-1], len(xs))


def batched_form(interp, M, ned, avg_ground, uv):
    """all rays at once, one scipy call per iteration round over the rays still iterating"""
    uvh = np.concatenate([uv, np.ones((len(uv), 1))], 1)
    proj = np.einsum('cij,nj->cni', M, uvh)
    v = (proj / np.sqrt((proj * proj).sum(-1, keepdims=True))).reshape(-1, 3)
    nd = np.repeat(ned, len(uv), axis=0)
    ag = np.repeat(avg_ground, len(uv))
    p = nd.copy()
    down = v[:, 2] > 0.0
    tmp = interp(p[:, 1], p[:, 0])
    surface = np.where(np.isnan(tmp), ag, tmp)
    error = np.abs(p[:, 2] - surface)
    rounds = 0
    live = np.nonzero(down & (error > 0.01))[0]
    while len(live) and rounds < 25:
        d_proj = -(nd[live, 2] - surface[live])
        factor = d_proj / v[live, 2]
        p[live, 0] = nd[live, 0] + v[live, 0] * factor
        p[live, 1] = nd[live, 1] + v[live, 1] * factor
        p[live, 2] = nd[live, 2] + d_proj
        tmp = interp(p[live, 1], p[live, 0])
        surface[live] = np.where(np.isnan(tmp), surface[live], tmp)
        error[live] = np.abs(p[live, 2] - surface[live])
        live = live[error[live] > 0.01]
        rounds += 1
    d = nd - p
    angle = np.degrees(np.arctan2(-d[:, 2], np.hypot(d[:, 0], d[:, 1])))
    p[down & (angle < 30)] = np.nan
    return p.reshape(len(M), len(uv), 3), rounds


class _Image(object):
    def __init__(self, name, grid_list, uv):
        self.name, self.grid_list, self.distorted_uv = name, grid_list, uv
        self.image_file = name


class _Proj(object):
    def __init__(self, images):
        self.image_list = images
        self._by = {im.name: im for im in images}

    def findImageByName(self, name):
        return self._by[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=100)
    ap.add_argument('--cols', type=int, default=100)
    ap.add_argument('--points', type=int, default=300000)
    ap.add_argument('--loop-images', type=int, default=64)
    ap.add_argument('--batched-images', type=int, default=10000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import scipy.interpolate
    import scipy.spatial
    import torch
    from imageanalysis_amd import kernels, panda3d, render_panda3d as rp, synth
    from imageanalysis_amd.hostlib import camera

    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    clock = time.perf_counter
    sc = synth.make_step5_scene(rows=a.rows, cols=a.cols, n_points=a.points)
    C = len(sc['M'])
    grid = rp.pixel_grid(sc['width'], sc['height'], 8)
    uv = np.array(grid, np.float64)
    say('Step 5 grid stage: %d images x %d rays over %d surface points (%s)'
        % (C, len(grid), a.points, torch.cuda.get_device_name(0)))

    # (a) the device path, on a fresh Delaunay object per repeat (build_map always has a fresh one;
    # the first repeat also loads libraries and warms the allocator, and is reported apart)
    runs = []
    for k in range(a.repeats + 1):
        t = clock()
        tri = scipy.spatial.Delaunay(sc['points'])
        t_del = clock() - t
        stats = {'stage_s': dict.fromkeys(rp.grid_stats['stage_s'], 0.0)}
        t = clock()
        pts = rp.surface_grids(tri, sc['values'], sc['M'], sc['ned'], sc['avg_ground'], grid, stats=stats)
        stats['total'] = clock() - t
        stats['stage_s']['delaunay'] = t_del
        stats['after'] = stats['total'] - stats['stage_s']['transform']
        runs.append(stats)
    say('(a) device path (render_panda3d.surface_grids), a fresh Delaunay per repeat, %d triangles, %.1f MB of records'
        % (len(tri.simplices), len(tri.simplices) * 128 / 1e6))
    first = runs[0]['stage_s']
    say('    first repeat (also library load, allocator): qhull %.4g s, transforms %.4g s, the rest %.4g s'
        % (first['delaunay'], first['transform'], runs[0]['after']))
    for key, label in (('delaunay', 'Delaunay on the host (qhull)'),
                       ('transform', 'its transforms (first access)'),
                       ('seed', 'seed grid on the host'), ('upload', 'upload + record packing'),
                       ('kernel', 'kernel + its argument uploads'), ('download', 'download')):
        say('    %-30s s: %s' % (label, spread([r['stage_s'][key] for r in runs[1:]])))
    say('    %-30s s: %s' % ('seed grid .. download', spread([r['after'] for r in runs[1:]])))
    say('    %-30s s: %s' % ('transforms .. download', spread([r['total'] for r in runs[1:]])))
    t_tri = [r['stage_s']['delaunay'] + r['stage_s']['transform'] for r in runs[1:]]
    say('    %-30s s: %s' % ('triangulation (qhull + transforms), common to (a) (b) (c)', spread(t_tri)))
    # the kernel alone, device-resident arguments, timed by events
    surf = kernels.Surface(tri, sc['values'])
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sc['M'], sc['ned'], sc['avg_ground'], uv)]
    t_k = []
    for _ in range(a.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kernels.surface_grid(surf, *dev)
        e1.record()
        torch.cuda.synchronize()
        t_k.append(e0.elapsed_time(e1) / 1e3)
    say('    kernel alone (events)          s: ' + spread(t_k[1:]))
    st = runs[-1]
    say('    rays %d: sky %d, below 30 degrees %d, host fallback %d' % (st['rays'], st['sky'], st['high_angle'], st['fallback']))
    say('    look-ups %d (%.2f per ray), records read %d (%.2f steps per look-up), most rounds of a ray %d'
        % (st['lookups'], st['lookups'] / st['rays'], st['steps'], st['steps'] / st['lookups'], int(st['rounds'].max())))
    med_kernel = sorted(t_k[1:])[len(t_k[1:]) // 2]
    say('    = %.3g rays/s, %.3g look-ups/s, %.3g records/s through the kernel'
        % (st['rays'] / med_kernel, st['lookups'] / med_kernel, st['steps'] / med_kernel))

    # (tri's transforms are computed by now: (b) and (c) are timed without the triangulation)
    interp = scipy.interpolate.LinearNDInterpolator(tri, sc['values'])
    # (b) the reference's loop form
    n_b = min(a.loop_images, C)
    pick = np.linspace(0, C - 1, n_b).astype(int)
    t_b, worst, calls = [], 0.0, 0
    for rep in range(a.repeats):
        t = clock()
        calls = 0
        for i in pick.tolist():
            ned_i, ground_i = sc['ned'][i].tolist(), float(sc['avg_ground'][i])
            got = []
            for v in rp.unit_rays(sc['M'][i], grid):
                p, rounds = rp.intersect2d_host(interp, ned_i, v, ground_i)
                got.append(p)
                calls += rounds + 1 if v[2] > 0.0 else 0
            if rep == 0:
                got = np.array(got)
                assert np.array_equal(np.isnan(got), np.isnan(pts[i])), i
                ok = ~np.isnan(got)
                worst = max(worst, float(np.abs(got[ok] - pts[i][ok]).max()))
        t_b.append(clock() - t)
    say('(b) reference loop form (a scipy call per look-up), %d images, %d calls' % (n_b, calls))
    say('    measured                       s: ' + spread(t_b))
    say('    per look-up                   us: ' + spread([x / calls * 1e6 for x in t_b]))
    say('    EXTRAPOLATED to %d images  s: %s' % (C, spread([x * C / n_b for x in t_b])))
    say('    device result against it: largest difference %.3g m on these images' % worst)

    # (c) one batched scipy call per round
    n_c = min(a.batched_images, C)
    pick = np.linspace(0, C - 1, n_c).astype(int)
    t_c = []
    for rep in range(a.repeats):
        t = clock()
        got, rounds = batched_form(interp, sc['M'][pick], sc['ned'][pick], sc['avg_ground'][pick], uv)
        t_c.append(clock() - t)
    assert np.array_equal(np.isnan(got), np.isnan(pts[pick]))
    ok = ~np.isnan(got)
    say('(c) batched host form (one scipy call per round), %d images, %d rounds' % (n_c, rounds))
    say('    measured                       s: ' + spread(t_c))
    if n_c < C:
        say('    EXTRAPOLATED to %d images  s: %s' % (C, spread([x * C / n_c for x in t_c])))
    say('    device result against it: largest difference %.3g m' % float(np.abs(got[ok] - pts[pick][ok]).max()))
    dev_after = sorted(r['after'] for r in runs[1:])
    host = sorted(x * C / n_c for x in t_c)
    say('    device (seed grid .. download, max %.4g s) against (c) (min %.4g s): %s'
        % (dev_after[-1], host[0], 'the device is ahead by more than the spread' if dev_after[-1] < host[0]
           else 'NOT ahead by more than the spread'))
    med = lambda xs: sorted(xs)[len(xs) // 2]                                      # noqa: E731
    m_tri = med(t_tri)
    say('the whole grid stage, triangulation (median %.4g s) included, medians:' % m_tri)
    say('    (a) device                     s: %.4g' % (m_tri + med(dev_after)))
    say('    (b) loop form, EXTRAPOLATED    s: %.4g' % (m_tri + med([x * C / n_b for x in t_b])))
    say('    (c) batched host form%s s: %.4g' % (', EXTRAPOLATED' if n_c < C else '              ',
                                              m_tri + med(host)))

    # the egg writer, 1 000 files
    camera.set_image_params(sc['width'], sc['height'])
    enu = np.stack([pts[:1000, :, 1], pts[:1000, :, 0], -pts[:1000, :, 2]], -1)
    shared = rp.redistort(grid, sc['K'], np.zeros(5))
    images = [_Image('IMG_%05d.JPG' % i, enu[i].tolist(), shared) for i in range(len(enu))]
    proj = _Proj(images)
    saved = panda3d.make_textures_opencv
    panda3d.make_textures_opencv = lambda *x, **k: None
    t_e = []
    try:
        for _ in range(a.repeats):
            d = tempfile.mkdtemp(prefix='iamx_eggs_')
            os.makedirs(os.path.join(d, 'models'))
            try:
                t = clock()
                with contextlib.redirect_stdout(io.StringIO()):
                    panda3d.generate_from_grid(proj, [im.name for im in images], analysis_dir=d)
                t_e.append((clock() - t) * 1000.0 / len(images))
                n_files = len(os.listdir(os.path.join(d, 'models')))
            finally:
                shutil.rmtree(d, ignore_errors=True)
    finally:
        panda3d.make_textures_opencv = saved
    say('egg writer (one host thread, text built in memory, one write per file), %d files written' % n_files)
    say('    per 1 000 files                s: ' + spread(t_e))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
