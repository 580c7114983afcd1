#!/usr/bin/env python3
"""The reference's `--filter homography | fundamental | essential` (scripts/lib/matcher.py:90-142
filter_by_transform) as a pass of its own on the MI355X path: every stored pair's matches go through
a RANSAC fit of the chosen two-view model on the device (matcher.verify_matches), matches that
disagree with the pair's best model are dropped from both directions, and the .match files of the
images that changed are rewritten.  Run it after 3a-matching and before 3b.

Running it twice filters twice: the second run fits to the survivors of the first.

Parity with cv2's RANSAC is UNPINNED (its sample sequence is its own); this one is fixed by --seed.

Run from the reference's scripts/ directory:
    python <repo>/imageanalysis_amd/scripts/3a-verify-matches.py PROJECT --filter fundamental
"""
import argparse

from lib import camera, project

from imageanalysis_amd import matcher, undistort

ap = argparse.ArgumentParser(description='RANSAC verification of stored matches on MI355X.')
ap.add_argument('project', help='project directory')
ap.add_argument('--filter', required=True, choices=['homography', 'fundamental', 'essential'])
ap.add_argument('--hypotheses', type=int, default=None,
                help='minimal samples tried per pair (default: 2048; 256 for essential, whose five-point '
                     'samples are all-inlier as often at an inlier share of 0.5)')
ap.add_argument('--seed', type=int, default=0)
ap.add_argument('--dry-run', action='store_true', help='print the counts, write nothing')
args = ap.parse_args()

proj = project.ProjectMgr(args.project)
proj.load_images_info()
proj.load_features(descriptors=False)
proj.load_match_pairs()
undistort.install(project.ProjectMgr)
proj.undistort_keypoints()

counts = matcher.verify_matches(proj, camera.get_K(), args.filter, hypotheses=args.hypotheses,
                                seed=args.seed)
for key in ('pairs', 'matches_in', 'matches_out', 'lists_emptied', 'too_few', 'no_model',
            'orphans_dropped'):
    print('%-16s %d' % (key, counts[key]))
if args.dry_run:
    print('dry run: nothing written')
else:
    matcher.saveMatches(proj.image_list, check_if_dirty=True)
