#!/usr/bin/env python3
"""CLI twin of scripts/4c-surface-outliers3.py on the MI355X path, in today's matches_grouped layout:
chains whose position does not go with the surface its image neighbours lie on (the distance to
them in space against the distance to them in the image) are culled in rounds until a round finds
none, and (on `y`) deleted from matches_grouped.  The neighbour search and the line fits of every
observation run on the device (match_culling.cull_surface); per round a few scalars and the culled
chain indices come back.  Neighbourhoods are taken in the stored (distorted) pixels.
Run from the reference's scripts/ directory: python <repo>/imageanalysis_amd/scripts/4c-surface-outliers.py PROJECT
"""
import argparse
import os
import pickle


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Cull chains that leave the surface of their image neighbours.')
    ap.add_argument('project', help='project directory')
    ap.add_argument('--group', type=int, default=0, help='group index')
    ap.add_argument('--stddev', type=float, default=5, help='standard dev threshold')
    ap.add_argument('--neighbors', type=int, default=30, help='nearest observations looked at per observation')
    ap.add_argument('--positives', type=int, default=10, help='of them, how many at a distance are used')
    ap.add_argument('--max-rounds', type=int, default=None, help='stop after this many rounds')
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

    print("Evaluating surface consistency:")
    rounds = cull.cull_surface(proj, matches, group_list, args.group, stddev=args.stddev,
                               max_rounds=args.max_rounds, k=args.neighbors, positives=args.positives)
    deleted_sum = sum(len(r) for r in rounds)
    if deleted_sum > 0:
        print('Outliers to remove from match lists:', deleted_sum)
        result = input('Save these changes? (y/n):')
        if result == 'y' or result == 'Y':
            cull.delete_marked_features(matches, min_chain_len)
            print("Writing original matches:", source)
            pickle.dump(matches, open(os.path.join(proj.analysis_dir, source), "wb"))


if __name__ == '__main__':
    main()
