#!/usr/bin/env python3
"""CLI twin of scripts/4b-colocated-feats.py on the MI355X path: chain members whose two cameras
see the feature under less than --min-angle degrees are marked and (on `y`) deleted from
matches_grouped.  The pair loop over every chain runs on the device (match_culling.colocated_features);
only the per-member counts come back.  The angle is the one the reference's compute_angle() means:
its script never imports math, so as written every pair of the group is marked.
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/4b-colocated-feats.py PROJECT
"""
import argparse
import os
import pickle

from lib import groups, project

from imageanalysis_amd import match_culling as cull
from imageanalysis_amd._deps import getNode

ap = argparse.ArgumentParser(description='Keypoint projection.')
ap.add_argument('project', help='project directory')
ap.add_argument('--group', type=int, default=0, help='group index')
ap.add_argument('--min-angle', type=float, default=1.0, help='max feature angle')
args = ap.parse_args()

proj = project.ProjectMgr(args.project)
proj.load_images_info()

matcher_node = getNode('/config/matcher', True)
min_chain_len = matcher_node.getInt("min_chain_len")
if min_chain_len == 0:
    min_chain_len = 3
print("Notice: min_chain_len is:", min_chain_len)

source = 'matches_grouped'
print("Loading matches:", source)
matches = pickle.load(open(os.path.join(proj.analysis_dir, source), "rb"))
print('Number of original features:', len(matches))

group_list = groups.load(proj.analysis_dir)
print('Group sizes:', end=" ")
for group in group_list:
    print(len(group), end=" ")
print()

print("Scanning match pair angles:")
mark_list = cull.colocated_features(proj, matches, group_list, args.group, args.min_angle)

cull.mark_using_list(mark_list, matches)
mark_sum = len(mark_list)
if mark_sum > 0:
    print('Outliers to remove from match lists:', mark_sum)
    result = input('Save these changes? (y/n):')
    if result == 'y' or result == 'Y':
        cull.delete_marked_features(matches, min_chain_len)
        print("Writing original matches:", source)
        pickle.dump(matches, open(os.path.join(proj.analysis_dir, source), "wb"))
