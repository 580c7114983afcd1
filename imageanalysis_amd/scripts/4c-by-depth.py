#!/usr/bin/env python3
"""CLI twin of scripts/4c-by-depth.py on the MI355X path, in today's matches_grouped layout: per image
the distance from the camera to each of its features, their mean and deviation; a chain whose members
lie far from their images' typical depth (by more than --stddev deviations of that metric above its
mean) has its first member marked; then every feature of an image left with fewer than --min-features
features is marked too (0 switches that rule off), and (on `y`) the marked are deleted from
matches_grouped.  The depths and the statistics run on the device (match_culling.depth_outliers).
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/4c-by-depth.py PROJECT
"""
import argparse
import os
import pickle


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Cull chains by their depth from the cameras.')
    ap.add_argument('project', help='project directory')
    ap.add_argument('--group', type=int, default=0, help='group index')
    ap.add_argument('--stddev', type=float, default=3,
                    help='how many standard deviations above the mean for auto discarding features')
    ap.add_argument('--strong', action='store_true', help='remove entire match chain, not just the worst offending element.')
    ap.add_argument('--min-features', type=int, default=25,
                    help='mark every feature of an image left with fewer than this many (0: off)')
    ap.add_argument('--interactive', action='store_true',
                    help='interactively review depth errors from worst to best and select for deletion or keep.')
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)

    from lib import groups, project

    from imageanalysis_amd import match_culling as cull
    from imageanalysis_amd._deps import getNode

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

    print("Computing depths for all match points...")
    if args.interactive:
        report = cull.chain_depths(proj, matches, group_list, args.group)
        metric = report.metric.cpu().numpy()
        looked = report.looked.cpu().numpy() != 0
        error_list = sorted(([float(metric[c]), int(c), 0] for c in looked.nonzero()[0]),
                            key=lambda fields: fields[0], reverse=True)
        mark_list = cull.show_outliers(error_list, matches, proj.image_list)
    else:
        mark_list, rows = cull.depth_outliers(proj, matches, group_list, args.group, args.stddev)
        for name, count, avg, std in rows:
            print(name, 'features:', count, 'avg:', avg, 'std:', std)
        print(" marking outliers...")
    cull.mark_using_list(mark_list, matches)
    mark_sum = len(mark_list)

    if args.min_features > 0:
        weak_list = cull.weak_images(matches, len(proj.image_list), args.min_features)
        print('weak images:', sorted(set(matches[c][2 + j][0] for c, j in weak_list)))
        for c, j in weak_list:
            cull.mark_feature(matches, c, j, "-", quiet=True)
        mark_sum += len(weak_list)

    if mark_sum > 0:
        print('Outliers removed from match lists:', mark_sum)
        result = input('Save these changes? (y/n):')
        if result == 'y' or result == 'Y':
            cull.delete_marked_features(matches, min_chain_len, strong=args.strong)
            print("Writing original matches:", source)
            pickle.dump(matches, open(os.path.join(proj.analysis_dir, source), "wb"))


if __name__ == '__main__':
    main()
