#!/usr/bin/env python3
"""The true orthophoto that goes with the dense surface (no counterpart in the reference, as the DSM
has none): every map pixel placed at its DSM height, projected into the full-resolution frames through
the camera model and coloured only from the frames that see it -- no leaning walls, no doubled roof
edges, no ground taken from a frame that cannot see it.  Reads <analysis_dir>/dense/ (5d-dense-surface.py),
closes its holes (dense.fill), drapes one group's frames on the device (imageanalysis_amd/ortho.py,
THE TRUE-ORTHO RULES) and writes <analysis_dir>/true_ortho/tile_<row>_<col>.<format> with a world file
each and ortho.json.  5c-ortho.py, the map over the sparse chains' grids, is unchanged.
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/5e-true-ortho.py PROJECT
"""
import argparse
import os

from lib import groups, project

from imageanalysis_amd import dense, histogram, ortho

ap = argparse.ArgumentParser(description='Drape the frames over the dense DSM: a true orthophoto.')
ap.add_argument('project', help='project directory')
ap.add_argument('--group', type=int, default=0, help='group index')
ap.add_argument('--upsample', type=int, default=1, help='mosaic pixels per DSM cell and side, 1 .. 8')
ap.add_argument('--mode', choices=ortho.DENSE_MODES, default='best',
                help="best: the frame that looks most steeply down on the pixel; feather: the frames that see it, "
                     "blended by distance from their borders")
ap.add_argument('--bands', type=int, default=0,
                help='blend along the seams of mode best with this many pyramid levels, 1 .. %d (0: no blend)'
                     % ortho.MAX_BANDS)
ap.add_argument('--bias', type=float, default=None,
                help='metres a DSM cell must stand above the ray to hide a pixel (default: one DSM cell, unmeasured)')
ap.add_argument('--fill-rounds', type=int, default=8, help='rounds of the DSM hole fill, 0 .. 254')
ap.add_argument('--tile', type=int, default=4096, help='tile side in pixels')
ap.add_argument('--format', default='jpg', help='tile file format (jpg, png, tif)')
ap.add_argument('--histogram', action='store_true',
                help="apply the neighbour histogram matching (<analysis_dir>/histogram, 99-vignette.py --histogram)")
ap.add_argument('--vignette', action='store_true', help='add models/vignette-mask.jpg (99-vignette.py)')
ap.add_argument('--no-prefilter', action='store_true',
                help='sample the full-resolution frame even where it is much finer than the mosaic')
args = ap.parse_args()

proj = project.ProjectMgr(args.project)
proj.load_images_info()
group_list = groups.load(proj.analysis_dir)
print('Group sizes:', " ".join(str(len(g)) for g in group_list))

if not os.path.exists(os.path.join(proj.analysis_dir, 'dense', 'dense.json')):
    raise SystemExit("%s/dense is missing: make the dense surface with 5d-dense-surface.py first" % proj.analysis_dir)
if not 0 <= args.bands <= ortho.MAX_BANDS or (args.bands and args.mode != 'best'):
    raise SystemExit("--bands is 0 .. %d and blends along the seams of --mode best (got --bands %d with --mode %s)"
                     % (ortho.MAX_BANDS, args.bands, args.mode))
if args.histogram and not histogram.load(proj.analysis_dir):
    raise SystemExit("--histogram: %s/histogram is missing (make it with 99-vignette.py --histogram)"
                     % proj.analysis_dir)

surface, round_of = dense.fill(dense.load(proj.analysis_dir), rounds=args.fill_rounds)
filled, empty = int(((round_of > 0) & (round_of < 255)).sum()), int((round_of == 255).sum())
print('DSM: %d x %d cells at %.3f m, %d filled in %d rounds, %d still empty'
      % (surface.shape[1], surface.shape[0], surface.gsd, filled, args.fill_rounds, empty))
mosaic = ortho.render_dense(proj, group_list, args.group, surface, mode=args.mode, upsample=args.upsample,
                            bias=args.bias, prefilter=not args.no_prefilter, histogram=args.histogram,
                            vignette=args.vignette, bands=args.bands)
h, w = mosaic.shape
print('Mosaic: %d x %d pixels at %.3f m, bias %.3f m, %d images, %.1f frames/s'
      % (w, h, mosaic.gsd, mosaic.bias, ortho.render_dense_stats['images'], ortho.render_dense_stats['frames_per_s']))
if args.bands:
    print('Blended over %d pyramid levels' % mosaic.bands)
info = ortho.save(mosaic, proj.analysis_dir, tile=args.tile, fmt=args.format, subdir='true_ortho')
print('Wrote %d tiles and ortho.json to %s/true_ortho' % (len(info['tiles']), proj.analysis_dir))
