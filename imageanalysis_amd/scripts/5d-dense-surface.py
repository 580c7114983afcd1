#!/usr/bin/env python3
"""A dense surface beside the Step 5 map and the orthomosaic (no counterpart in the reference, whose
surface is the sparse chains' triangulation): plane-sweep depth maps of one group's images against
their best neighbours, cross-checked between views and fused into a height raster on the device
(imageanalysis_amd/dense.py), written as <analysis_dir>/dense/dsm.npy, count.npy, dsm.wld and
dense.json, with --ply the surviving points as dense/points.ply.  --regularize sgm puts the semi-global
aggregation of dense.py's SEMI-GLOBAL RULES between the cost volume and the winner (2 to 64 planes).
--refine LEVELS goes coarse to fine (dense.py's REFINEMENT RULES): the sweep above runs at
scale / 2^LEVELS, and each level after it doubles the scale and sweeps, per tile, only a window of
--refine-ratio times finer planes around the depths of the level before; --scale stays the final scale.
--fusion robust replaces the mean of a cell's points by dense.py's ROBUST FUSION RULES (per-cell height
histograms pick the cluster to average) and writes dense/support.npy beside the count.
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/5d-dense-surface.py PROJECT
"""
import argparse
import os
import pickle
import time

from lib import groups, project

from imageanalysis_amd import dense

ap = argparse.ArgumentParser(description='Dense depth maps and a DSM raster of one group.')
ap.add_argument('project', help='project directory')
ap.add_argument('--group', type=int, default=0, help='group index')
ap.add_argument('--scale', type=float, default=0.125, help='sweep scale of the frames')
ap.add_argument('--planes', type=int, default=64, help='depth hypotheses per image, uniform in inverse depth')
ap.add_argument('--neighbors', type=int, default=4, help='images to sweep each image against')
ap.add_argument('--radius', type=int, default=3, help='correlation window radius, 1 .. 7')
ap.add_argument('--min-score', type=float, default=0.6, help='least mean correlation of a kept pixel')
ap.add_argument('--gsd', type=float, default=0.0, help='metres per cell (default: the sweep pixel\'s footprint at the median depth)')
ap.add_argument('--ply', action='store_true', help='write the surviving points as dense/points.ply')
ap.add_argument('--regularize', choices=dense.REGULARIZE, default='none', help='none: winner-take-all; sgm: semi-global aggregation')
ap.add_argument('--p1', type=int, default=dense.SGM_P1, help='sgm: penalty of a change by one plane')
ap.add_argument('--p2', type=int, default=dense.SGM_P2, help='sgm: penalty of a larger change, P1 <= P2 <= 255')
ap.add_argument('--paths', type=int, choices=(4, 8), default=8, help='sgm: directions aggregated')
ap.add_argument('--refine', type=int, default=0, metavar='LEVELS',
                help='coarse to fine: sweep at scale / 2^LEVELS, then LEVELS guided levels up to --scale')
ap.add_argument('--refine-ratio', type=int, default=4, metavar='R', help='refine: fine planes per coarse plane step')
ap.add_argument('--fusion', choices=dense.FUSIONS, default='mean', help='mean: every point of a cell; robust: the cluster its histograms find')
ap.add_argument('--fusion-bins', type=int, default=32, help='robust: histogram bins per cell, 4 .. 64')
ap.add_argument('--fusion-levels', type=int, default=2, help='robust: histogram levels, 1 .. 4')
ap.add_argument('--fusion-band', type=float, default=None, metavar='METRES', help='robust: least bin width (default: half the gsd)')
ap.add_argument('--fusion-share', type=int, default=256, help='robust: first level accepts a cluster of this many 256ths of the strongest, 1 .. 256')
args = ap.parse_args()
try:
    sgm = dense.sgm_parameters(args.planes, args.regularize, args.p1, args.p2, args.paths)
    fusion = dense.fusion_parameters(args.fusion, args.fusion_bins, args.fusion_levels, args.fusion_band, args.fusion_share)
    if not 0 <= args.refine <= 8:
        raise ValueError("--refine is 0 to 8 levels, got %d" % args.refine)
    planes_total = args.planes
    for _ in range(args.refine):
        planes_total = dense.refine_planes(planes_total, args.refine_ratio)
except ValueError as e:
    ap.error(str(e))

proj = project.ProjectMgr(args.project)
proj.load_images_info()
group_list = groups.load(proj.analysis_dir)
print('Group sizes:', " ".join(str(len(g)) for g in group_list))
with open(os.path.join(proj.analysis_dir, "matches_grouped"), "rb") as f:
    matches = pickle.load(f)

t0 = time.perf_counter()
views, group = dense.views_from_project(proj, group_list, args.group, matches, args.scale / 2 ** args.refine)
if not views:
    raise SystemExit("group %d has no images" % args.group)
poses = [(v.R, v.C) for v in views]
neighbours = dense.choose_neighbours(matches, group, poses, n=args.neighbors)
ranges = dense.depth_range(matches, group, poses)
swept = sum(1 for n, r in zip(neighbours, ranges) if n and r is not None)
print('Views: %d of %d x %d pixels, %d with neighbours and a depth range' % (len(views), views[0].G.shape[1],
                                                                            views[0].G.shape[0], swept))
mode = {} if sgm is None else dict(regularize=args.regularize, p1=sgm[2], p2=sgm[3], paths=sgm[1])
maps = dense.depth_maps(views, neighbours, ranges, planes=args.planes, radius=args.radius, min_score=args.min_score, **mode)
planes = args.planes
for level in range(1, args.refine + 1):
    views, _group = dense.views_from_project(proj, group_list, args.group, matches, args.scale / 2 ** (args.refine - level))
    maps = dense.refine(views, neighbours, ranges, maps, planes, ratio=args.refine_ratio, radius=args.radius,
                        min_score=args.min_score)
    planes = maps.total
    count = maps.windows[..., 1].float()
    print('Level %d: %d x %d pixels, %d planes, %.1f of them walked per tile (most %d)'
          % (level, views[0].G.shape[1], views[0].G.shape[0], planes, float(count.mean()), int(count.max())))
if args.refine:
    mode = dict(mode, refine=args.refine, ratio=args.refine_ratio, planes_total=planes)
gsd = args.gsd
if gsd <= 0.0:
    mids = sorted(0.5 * (r[0] + r[1]) for r in ranges if r is not None)
    if not mids:
        raise SystemExit("no image of group %d observes a positioned chain" % args.group)
    gsd = mids[len(mids) // 2] / float(views[0].K[0])
if fusion is None:
    surface = dense.fuse(views, maps, gsd)
else:
    surface = dense.fuse(views, maps, gsd, method=args.fusion, bins=fusion['bins'], levels=fusion['levels'],
                         band=fusion['band'], share=fusion['share'])
info = dense.save(surface, proj.analysis_dir, points=dense.surface_points(views, maps) if args.ply else None,
                  extra=mode)
print('DSM: %d x %d cells at %.3f m, %d of them filled by %d points, %.1f s'
      % (info['width'], info['height'], gsd, info['cells_filled'], info['points_fused'], time.perf_counter() - t0))
if fusion is not None:
    print('Robust fusion: %d of the %d points support their cells (%d bins, %d levels, band %.3f m, share %d/256)'
          % (info['points_supporting'], info['points_fused'], info['bins'], info['levels'], info['band'], info['share']))
print('Wrote %s to %s/dense' % (', '.join(sorted(info['files'].values())), proj.analysis_dir))
