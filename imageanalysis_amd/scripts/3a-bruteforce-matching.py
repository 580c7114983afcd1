#!/usr/bin/env python3
"""Step 3a with the reference's 'bruteforce' strategy on the MI355X path: matcher.bruteforce_matches,
the pair loop of scripts/lib/matcher.py:923-1031 with bruteforce_pair_matches (:696-850) per pair --
among every feature's three nearest neighbours the one of the smallest size_diff / ratio, the choices
grouped by their image-space motion into 41 x 21 overlapping cells, a RANSAC homography per cell.

The strategy needs no pose prior: it is the one for a survey with bad pose metadata.  Its pairs are
independent of each other, so they run through the batched rounds; ONE GPU.
Run from the reference's scripts/ directory (it provides lib.project / lib.camera / lib.smart):
    python <repo>/imageanalysis_amd/scripts/3a-bruteforce-matching.py PROJECT [--sort]
"""
import argparse

from props import getNode

from lib import camera, project, smart
try:
    from lib import srtm
except ImportError:                     # (pylab / navpy missing: the mirror, tiles from the cache only)
    from imageanalysis_amd import srtm
from lib.logger import log

from imageanalysis_amd import matcher

ap = argparse.ArgumentParser(description="Feature matching on MI355X, the 'bruteforce' strategy.")
ap.add_argument('project', help='project directory')
ap.add_argument('--scale', type=float, default=0.4, help='image scale for feature detection')
ap.add_argument('--detector', default='SIFT', choices=['SIFT'])
ap.add_argument('--match-ratio', default=0.75, type=float)
ap.add_argument('--min-pairs', default=25, type=int)
ap.add_argument('--sort', action='store_true', help='closest pairs first (scripts/lib/matcher.py:905-916)')
args = ap.parse_args()

proj = project.ProjectMgr(args.project)
proj.load_images_info()
proj.load_match_pairs()

node = getNode('/config/detector', True)
node.setString('detector', args.detector)
node.setString('scale', args.scale)
node = getNode('/config/matcher', True)
node.setFloat('match_ratio', args.match_ratio)
node.setInt('min_pairs', args.min_pairs)
proj.save()

ref_node = getNode('/config/ned_reference', True)
ref = [ref_node.getFloat('lat_deg'), ref_node.getFloat('lon_deg'), ref_node.getFloat('alt_m')]
log("NED reference location:", ref)
srtm.initialize(ref, 6000, 6000, 30)
smart.load(proj.analysis_dir)
smart.update_srtm_elevations(proj)
smart.set_yaw_error_estimates(proj)
proj.save_images_info()

matcher.configure()
matcher.bruteforce_matches(proj, camera.get_K(), sort=args.sort)

n = sum(image.num_features for image in proj.image_list)
log("Average # of features per image found = %.0f" % (n / max(len(proj.image_list), 1)))
