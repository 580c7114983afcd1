#!/usr/bin/env python3
"""CLI twin of scripts/99-vignette.py on the MI355X path: the survey's mean frame
(models/vignette-avg.jpg), the radial fit and the vignette mask (models/vignette-mask.jpg), with
the decode, the sum, the fit's sums and the mask on the device (imageanalysis_amd/vignette.py).
--histogram also writes <analysis_dir>/histogram (lib/histogram.py's file) from the same pass over
the frames.  No windows and no plots; --scale only sized the reference's preview and is ignored.
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/99-vignette.py PROJECT
"""
import argparse

from lib import camera, project

from imageanalysis_amd import vignette

parser = argparse.ArgumentParser(description='I want to vignette.')
parser.add_argument('project', help='project directory')
parser.add_argument('--scale', type=float, default=0.2, help='preview scale (accepted, ignored: no preview)')
parser.add_argument('--nofit', action='store_true',
                    help='skip fitting the ideal function and just process the average as the mask')
parser.add_argument('--histogram', action='store_true',
                    help='also write the neighbour histogram templates, from the same pass over the frames')
parser.add_argument('--dist-cutoff', type=float, default=40, help='template neighbour cutoff (m)')
parser.add_argument('--self-weight', type=float, default=0.1, help="template weight of the image's own histogram")
args = parser.parse_args()

proj = project.ProjectMgr(args.project)

# load existing images info which could include things like camera pose
proj.load_images_info()

# camera paramters
K = camera.get_K(optimized=True)
cu = K[0, 2]
cv = K[1, 2]
print("Project cu = %.2f  cv = %.2f:" % (cu, cv))

width, height = camera.get_image_params()
vignette.make_vignette(proj.analysis_dir, list(proj.image_list), cu, cv, width, height, nofit=args.nofit,
                       histograms=args.histogram, dist_cutoff=args.dist_cutoff, self_weight=args.self_weight)
