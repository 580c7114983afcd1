#!/usr/bin/env python3
"""CLI twin of scripts/4b-mre-by-image.py on the MI355X path: the mean reprojection error per
image, then the outlier observations marked and (on `y`) deleted from matches_grouped.  The
residual, the per-image table and the threshold pass run on the device (match_culling.py);
only the flagged observations come back to the host.
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/4b-mre-by-image.py PROJECT
"""
import argparse
import os
import pickle

from lib import groups, project

from imageanalysis_amd import match_culling as cull
from imageanalysis_amd import optimizer
from imageanalysis_amd._deps import getNode

ap = argparse.ArgumentParser(description='Keypoint projection.')
ap.add_argument('project', help='project directory')
ap.add_argument('--group', type=int, default=0, help='group number')
ap.add_argument('--stddev', type=float, default=5,
                help='how many stddevs above the mean for auto discarding features')
ap.add_argument('--max', type=float, help='maximum error cutoff, in addition to stddev check')
ap.add_argument('--initial-pose', action='store_true',
                help='work on initial pose, not optimized pose')
ap.add_argument('--strong', action='store_true',
                help='remove entire match chain, not just the worst offending element.')
ap.add_argument('--interactive', action='store_true',
                help='interactively review reprojection errors from worst to best and select for deletion or keep.')
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

opt = optimizer.Optimizer(args.project)
opt.setup(proj, group_list, args.group, matches, optimized=not args.initial_pose)
print('cameras:', opt.n_cameras)

report = cull.mre_by_image(opt, matches, proj=proj)
print(report.n_error)
print('mre: %.3f std: %.3f max: %.2f' % (report.mre, report.std, report.max))

print('Tabulating results...')
print("Report of images that aren't fitting well:")
worst = [line for line in report.by_cam if line[0] > report.mre + 3 * report.std]
for line in worst:
    print("%s - mean: %.3f max: %.3f" % (line[2], line[0], line[1]))
for line in worst:
    print(line[2], end=" ")
print()

if args.interactive:
    # the whole list, worst first, with (match, feature) of every observation (host side)
    obs, err, _, _ = cull.flagged(report, float('-inf'))
    fmap = report.feat_map_rev
    mi = [fmap[j] for j in report.pt_idx[obs].tolist()]
    fi = cull.observation_features(matches, mi, report.camera_map_fwd[report.cam_idx[obs]])
    error_list = [[e, m, f] for e, m, f in zip(err.tolist(), mi, fi.tolist())]
    mark_list = cull.show_outliers(error_list, matches, proj.image_list)
    cull.mark_using_list(mark_list, matches)
    mark_sum = len(mark_list)
else:
    mark_sum = cull.mark_outliers(matches, report, args.stddev, max_error=args.max)

if mark_sum > 0:
    print('Outliers removed from match lists:', mark_sum)
    result = input('Save these changes? (y/n):')
    if result == 'y' or result == 'Y':
        cull.delete_marked_features(matches, min_chain_len, strong=args.strong)
        print("Writing:", source)
        pickle.dump(matches, open(os.path.join(proj.analysis_dir, source), "wb"))
