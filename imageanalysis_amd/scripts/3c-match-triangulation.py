#!/usr/bin/env python3
"""CLI twin of scripts/3c-match-triangulation.py on the MI355X path: every chain's 3-D position is
computed again, by ground intersection (--method srtm: match_cleanup.triangulate_smart) or by the
least-squares intersection of the chain's undistorted rays (--method triangulate:
match_cleanup.triangulate_rays, one device thread per chain).

--attitude says where --method triangulate takes the camera attitude from.  The reference's script
takes the POSITION from the optimised pose and the ATTITUDE from the initial one
(image.get_body2ned() defaults to opt=False); `initial` (the default) reproduces that, `optimized`
takes both from the optimised pose.

The per-chain `i old >>> new` lines are printed with --verbose only; without it a count of written
and "WHOA!" (below the ground plane: x[2] > 0) chains.
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/3c-match-triangulation.py PROJECT
"""
import argparse
import os
import pickle

from lib import groups, project

from imageanalysis_amd import match_cleanup
from imageanalysis_amd._deps import getNode, logger

ap = argparse.ArgumentParser(description='Keypoint projection.')
ap.add_argument('project', help='project directory')
ap.add_argument('--group', type=int, default=0, help='group number')
ap.add_argument('--method', default='srtm', choices=['srtm', 'triangulate'])
ap.add_argument('--attitude', default='initial', choices=['initial', 'optimized'],
                help='triangulate: camera attitude from the initial pose (as the reference does) '
                     'or from the optimized pose, like the position')
ap.add_argument('--verbose', action='store_true', help='print every chain: index old >>> new')
args = ap.parse_args()

proj = project.ProjectMgr(args.project)
proj.load_images_info()

source = 'matches_grouped'
print("Loading source matches:", source)
matches = pickle.load(open(os.path.join(proj.analysis_dir, source), 'rb'))

group_list = groups.load(proj.analysis_dir)
print('Group sizes:', end=" ")
for group in group_list:
    print(len(group), end=" ")
print()

if args.method == 'srtm':
    try:
        from lib import srtm
    except ImportError:                 # (pylab / navpy missing: the mirror, tiles from the cache only)
        from imageanalysis_amd import srtm
    ref_node = getNode('/config/ned_reference', True)
    ref = [ref_node.getFloat('lat_deg'), ref_node.getFloat('lon_deg'), ref_node.getFloat('alt_m')]
    logger().log("NED reference location:", ref)
    srtm.initialize(ref, 6000, 6000, 30)
    match_cleanup.triangulate_smart(proj, matches)
else:
    if args.attitude == 'initial':
        logger().log("triangulate: optimized camera positions with INITIAL attitudes (as the reference "
                     "script does; --attitude optimized takes both from the optimized pose)")
    else:
        logger().log("triangulate: optimized camera positions and optimized attitudes")
    res = match_cleanup.triangulate_rays(proj, matches, group_list, args.group, attitude=args.attitude)
    below = set(res.below.tolist())
    if args.verbose:
        for i, old, new in zip(res.written.tolist(), res.old.tolist(), res.new.tolist()):
            print(i, None if old[0] != old[0] else old, '>>>', end=" ")
            if i in below:
                print("WHOA!")
            print(new)
    print('Chains written:', len(res.written), 'WHOA! (below the ground plane):', len(below))

print("Writing:", source)
pickle.dump(matches, open(os.path.join(proj.analysis_dir, source), "wb"))
