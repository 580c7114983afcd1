#!/usr/bin/env python3
"""The Step 5 map as an orthomosaic on disk (no counterpart among the reference's live scripts: its
raster export, lib/render4geotiff.py and 2f-gen-warped-images.py, is dead Python 2; its map is
explorer.py's Panda3D window).  One group's surface grids, textured from the full-resolution frames
and composed top-down on the device (imageanalysis_amd/ortho.py), written as
<analysis_dir>/ortho/tile_<row>_<col>.<format> with a world file each and ortho.json.
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/5c-ortho.py PROJECT
"""
import argparse

from lib import groups, project

from imageanalysis_amd import histogram, ortho

ap = argparse.ArgumentParser(description='Render the map to an orthomosaic raster.')
ap.add_argument('project', help='project directory')
ap.add_argument('--group', type=int, default=0, help='group index')
ap.add_argument('--gsd', type=float, default=0.1, help='metres per pixel')
ap.add_argument('--mode', choices=sorted(ortho.MODES), default='best',
                help="best: the explorer's ordering, one image per pixel; feather: blended by distance from the "
                     "frame's border; multiband: best's seams blended band by band (Laplacian pyramids), wide for "
                     "coarse detail and narrow for fine")
ap.add_argument('--bands', type=int, default=5, help='multiband: pyramid levels, 1 .. 16 (fewer are used on a small mosaic)')
ap.add_argument('--tile', type=int, default=4096, help='tile side in pixels')
ap.add_argument('--format', default='jpg', help='tile file format (jpg, png, tif)')
ap.add_argument('--histogram', action='store_true',
                help="apply the neighbour histogram matching (<analysis_dir>/histogram, 99-vignette.py --histogram)")
ap.add_argument('--vignette', action='store_true', help='add models/vignette-mask.jpg (99-vignette.py)')
ap.add_argument('--no-prefilter', action='store_true',
                help='sample the full-resolution frame even where it is much finer than the raster')
args = ap.parse_args()

proj = project.ProjectMgr(args.project)
proj.load_images_info()
group_list = groups.load(proj.analysis_dir)
print('Group sizes:', " ".join(str(len(g)) for g in group_list))

if args.histogram and not histogram.load(proj.analysis_dir):
    raise SystemExit("--histogram: %s/histogram is missing (make it with 99-vignette.py --histogram)"
                     % proj.analysis_dir)

mosaic = ortho.render(proj, group_list, args.group, args.gsd, mode=args.mode, prefilter=not args.no_prefilter,
                      histogram=args.histogram, vignette=args.vignette, bands=args.bands)
h, w = mosaic.shape
print('Mosaic: %d x %d pixels at %.3f m, %d images, %.1f frames/s' % (w, h, args.gsd, ortho.render_stats['images'],
                                                                     ortho.render_stats['frames_per_s']))
info = ortho.save(mosaic, proj.analysis_dir, tile=args.tile, fmt=args.format)
print('Wrote %d tiles and ortho.json to %s/ortho' % (len(info['tiles']), proj.analysis_dir))
