"""CPU: the plain reference of the match post-filters (postfilter_reference.py) against the host
path, and the edge cases of test_postfilter_edges_gpu.py against themselves -- every case must
tell the right rule from the wrong one it is there to catch, and the isolation scene must be what
it claims to be.  Everything compared is integer lists and counts."""
import glob
import os

import numpy as np
import pytest

import postfilter_reference as pr
from conftest import GOLDEN

CASES = pr.cases()
BY_NAME = dict((c['name'], c) for c in CASES)
MATCH_CASES = sorted(glob.glob(os.path.join(GOLDEN, 'match_*.npz')))

# The cases that name no wrong rule, and why none of the four can change them.  (A case that is
# added without a rule has to be added here too.)
NO_RULE = {
    'sort_n0': 'first gate: nothing comes out', 'sort_n1': 'first gate', 'sort_n24': 'first gate',
    'select_distinct_n2049': 'no equal metrics', 'select_distinct_n2304': 'no equal metrics',
    'select_distinct_n2305': 'no equal metrics', 'select_distinct_n4097': 'no equal metrics',
    'select_quota_end_last_n2305': 'every tie is kept: the last one is the last survivor',
    'select_quota_end_last_n4097': 'every tie is kept: the last one is the last survivor',
    'gms_threshold_above': 'every cell is below the threshold', 'gms_threshold_below': 'every cell is above it',
    'gms_last_row_col': 'pins the cells the shifted grids leave out (asserted below)',
    'dedupe_half_even': 'pins the "%.2f" keys (drop count asserted below)',
    'dedupe_float32_print': 'pins the "%.2f" keys (drop count asserted below)',
    'dedupe_no_repeat': 'nothing is dropped', 'gate_fwd40_rev24': 'gate only', 'gate_fwd40_rev25': 'gate only',
    'gate_rev_dedupe_leaves_24': 'gate only',
}
NO_RULE.update(('gms_rotation_%d' % a, 'winning rotation asserted below') for a in pr.ROTATION_ANGLES)


@pytest.fixture
def host():
    """the host filters with a case's min_pairs / image size; the module's settings are put back"""
    from imageanalysis_amd import matcher
    from imageanalysis_amd.hostlib import camera
    old_pairs, old_size = matcher.min_pairs, camera.get_image_params()

    def run(fwd, rev, xy1, xy2, size, min_pairs):
        matcher.min_pairs = min_pairs
        camera.set_image_params(*size)
        f = matcher._post_filter(None, None, matcher._threshold_sort_clip(*fwd), (xy1, xy2))
        r = []
        if len(f) >= matcher.min_pairs:                           # bidirectional_pair_matches
            r = matcher._post_filter(None, None, matcher._threshold_sort_clip(*rev), (xy2, xy1))
        return np.array(matcher.filter_cross_check(f, r)[0], np.int64).reshape(-1, 2)

    yield run
    matcher.min_pairs = old_pairs
    camera.set_image_params(*old_size)


@pytest.mark.parametrize('case', [c for c in CASES if c['thr_factor'] == 5.0], ids=lambda c: c['name'])
def test_reference_equals_host_path(case, host):
    want, _stat = pr.expected(case)
    got = host(case['fwd'], case['rev'], case['xy1'], case['xy2'], pr.SIZE, case['min_pairs'])
    assert np.array_equal(got, want)


@pytest.mark.parametrize('path', MATCH_CASES, ids=os.path.basename)
def test_reference_equals_golden_pairs(path, host):
    g = np.load(path)
    thresh = 270.0 * float(g['match_ratio'])                      # matcher.max_distance for SIFT
    surv = []
    for tag in ('fwd', 'rev'):
        d0 = g['knn_%s_dist' % tag][:, 0].astype(np.float64)
        d1 = g['knn_%s_dist' % tag][:, 1].astype(np.float64)
        metric = d0 * (d0 / d1)
        keep = np.nonzero(metric < thresh)[0]
        surv.append((keep.astype(np.int32), g['knn_%s_idx' % tag][keep, 0], metric[keep]))
    size, min_pairs = (int(g['width']), int(g['height'])), int(g['min_pairs'])
    got, stat = pr.postfilter(surv[0], surv[1], g['xy1'], g['xy2'], size, min_pairs, 5.0)
    assert np.array_equal(got, g['bidir_fwd'])
    if len(g['pregms_fwd']):
        assert stat[:2] == [len(g['postgms_fwd']), len(g['basic_fwd'])]
    if len(g['pregms_rev']):
        assert stat[2:] == [len(g['postgms_rev']), len(g['basic_rev'])]
    assert np.array_equal(host(surv[0], surv[1], g['xy1'], g['xy2'], size, min_pairs), got)


def test_every_case_names_its_wrong_rule_or_says_why_not():
    assert sorted(c['name'] for c in CASES if c['wrong'] is None) == sorted(NO_RULE)
    assert set(c['wrong'] for c in CASES) == set(pr.WRONG) | {None}


@pytest.mark.parametrize('case', [c for c in CASES if c['wrong']], ids=lambda c: c['name'])
def test_wrong_rule_changes_the_case(case):
    want, stat = pr.expected(case)
    got, stat_w = pr.run_case(case, wrong=case['wrong'])
    assert not (np.array_equal(got, want) and stat_w == stat), case['wrong']


def test_wrong_rules_are_the_right_rules_elsewhere():
    """the variants differ from the rules only in what they name: with no equal metrics, no cell at
    its threshold, no repeated position and no split left cell all five agree"""
    case = BY_NAME['select_distinct_n2049']
    want, stat = pr.expected(case)
    for wrong in pr.WRONG:
        got, stat_w = pr.run_case(case, wrong=wrong)
        assert np.array_equal(got, want) and stat_w == stat, wrong


@pytest.mark.parametrize('case', [c for c in CASES if c['name'].startswith('gms_')], ids=lambda c: c['name'])
def test_loop_gms_equals_host_gms(case):
    """the cell-by-cell GMS that carries the two wrong GMS rules is, without them, the host's"""
    from imageanalysis_amd.gms import gms_inlier_mask
    for surv, xa, xb in ((case['fwd'], case['xy1'], case['xy2']), (case['rev'], case['xy2'], case['xy1'])):
        pairs = pr.sort_clip(*surv)
        mask = pr.gms_loop(xa, xb, pr.SIZE, pairs, case['thr_factor'])[0]
        assert np.array_equal(mask, gms_inlier_mask(xa, xb, pr.SIZE, pr.SIZE, pairs,
                                                    threshold_factor=case['thr_factor']))


ISOLATION = [c for c in CASES if c['name'].startswith(('sort_', 'select_'))]


@pytest.mark.parametrize('case', ISOLATION, ids=lambda c: c['name'])
def test_isolation_scene_does_what_it_claims(case):
    from imageanalysis_amd.gms import gms_inlier_mask
    assert case['thr_factor'] == 5.0
    for xy in (case['xy1'], case['xy2']):
        cell = np.floor(xy / 100.0)
        assert (cell == cell[0]).all()                                        # one grid cell
        inside = xy - 100.0 * cell
        assert (inside >= 5.0).all() and (inside <= 45.0).all()              # clear of the half-cell lines
        assert np.array_equal(xy * 4.0, np.round(xy * 4.0))                  # 0.25 px lattice
        keys = set("%.2f-%.2f" % tuple(p) for p in xy.tolist())
        assert len(keys) == len(xy)                                           # distinct at two decimals
    q, t, metric = case['fwd']
    assert len(set(q.tolist())) == len(q) and len(set(t.tolist())) == len(t)
    ordered = pr.sort_clip(q, t, metric)
    assert len(ordered) == min(len(q), pr.CLIP)
    if len(ordered) >= 3:
        assert gms_inlier_mask(case['xy1'], case['xy2'], pr.SIZE, pr.SIZE, ordered).all()
        assert len(pr.dedupe(case['xy1'], case['xy2'], ordered)) == len(ordered)
    # the reverse survivors hold the mirror of the ordered forward list (and nothing else that
    # survives their own clip), so the whole chain returns that list, in order
    rq, rt, rmetric = case['rev']
    kept_rev = pr.sort_clip(rq, rt, rmetric)
    assert set(map(tuple, kept_rev[:, ::-1].tolist())) == set(map(tuple, ordered.tolist()))
    want, stat = pr.expected(case)
    if len(ordered) >= case['min_pairs']:
        assert np.array_equal(want, ordered)
        assert stat == [len(ordered)] * 4
    else:
        assert len(want) == 0 and stat == [-1] * 4


def test_sort_counts_and_patterns_are_all_there():
    names = set(BY_NAME)
    for n in pr.SORT_COUNTS:
        assert ('sort_n%d' % n in names) if n <= 2048 else ('select_all_equal_n%d' % n in names)
    for n in pr.SELECT_COUNTS:
        for p in pr.SELECT_PATTERNS:
            assert 'select_%s_n%d' % (p, n) in names
    for c in CASES:
        n = len(c['fwd'][0])
        if c['name'].startswith('select_quota_end_') and c['name'].split('_')[3].isdigit():
            # the last kept tie sits where the name says, with ties behind it
            metric = c['fwd'][2]
            ties = np.nonzero(metric == 10.0)[0]
            quota = pr.CLIP - int((metric < 10.0).sum())
            end = int(c['name'].split('_')[3])
            assert 0 < quota < len(ties) and ties[quota - 1] % 256 == end % 256
            assert ties[quota - 1] // 256 < (n - 1) // 256
    for name in ('select_quota_end_last_n2305', 'select_quota_end_last_n4097'):
        metric = BY_NAME[name]['fwd'][2]
        ties = np.nonzero(metric == 10.0)[0]
        assert ties[-1] == len(metric) - 1 and len(ties) + int((metric < 10.0).sum()) == pr.CLIP
        assert (len(metric) - 1) % 256 == 0                                   # a chunk of its own
    metric = BY_NAME['select_quota_end_partial_n2100']['fwd'][2]
    ties = np.nonzero(metric == 10.0)[0]
    assert ties[pr.CLIP - int((metric < 10.0).sum()) - 1] == 2070 and 2070 // 256 == 2099 // 256
    m = BY_NAME['select_quota_1_n2305']['fwd'][2]
    assert (np.sort(m)[:1999] < 3.0).all() and len(np.unique(m[m < 3.0])) == 1999 and (m[1999:] == 3.0).all()
    m = BY_NAME['select_exponents_n4097']['fwd'][2]
    assert (m == 0.0).any() and (m == 5e-324).any() and m.max() > 1e290 and m[m > 5e-324].min() < 1e-290
    m = BY_NAME['select_low_byte_n2049']['fwd'][2].view(np.int64)
    assert len(np.unique(m >> 8)) == 1 and len(np.unique(m)) > 200
    m = BY_NAME['select_low_two_bytes_n2049']['fwd'][2].view(np.int64)
    assert len(np.unique(m >> 16)) == 1 and len(np.unique(m >> 8)) > 200


def test_threshold_lattice_counts():
    """interior cells of the lattice score exactly 18 sqrt(tot / npair)"""
    assert len(BY_NAME['gms_threshold_equal']['fwd'][0]) == 1224
    for name, kept in (('gms_threshold_equal', 960), ('gms_threshold_above', 0), ('gms_threshold_below', 960)):
        want, stat = pr.expected(BY_NAME[name])
        assert stat[0] == kept and len(want) == kept, name
    assert BY_NAME['gms_threshold_above']['thr_factor'] > 18.0 > BY_NAME['gms_threshold_below']['thr_factor']


def test_argmax_tie_scene_has_ties():
    case = BY_NAME['gms_argmax_tie']
    pairs = pr.sort_clip(*case['fwd'])
    lg = pr.left_cells(case['xy1'], pairs[:, 0], pr.SIZE)[0]
    rg = pr.right_cells(case['xy2'], pairs[:, 1], pr.SIZE)
    first_is_larger = 0
    for c in np.unique(lg):
        cells, counts = np.unique(rg[lg == c], return_counts=True)
        assert len(cells) >= 2 and len(set(counts.tolist())) == 1
        first_is_larger += rg[lg == c][0] != cells.min()
    assert first_is_larger >= 1
    want, _stat = pr.expected(case)
    assert len(want) == 30 + 28 + 26


def test_border_scene_has_cells_the_shifted_grids_leave_out():
    case = BY_NAME['gms_last_row_col']
    pairs = pr.sort_clip(*case['fwd'])
    grids = pr.left_cells(case['xy1'], pairs[:, 0], pr.SIZE)
    assert (grids[0] >= 0).all()
    assert (grids[0] % 20 == 19).sum() > 100 and (grids[0] // 20 == 19).sum() > 100
    assert (grids[0] == 399).any()
    for g in grids[1:]:
        assert (g < 0).sum() > 100
    assert ((grids[1] < 0) & (grids[2] < 0)).any()             # the corner: outside all three
    want, _stat = pr.expected(case)
    kept = set(want[:, 0].tolist())
    assert any(int(q) in kept for q in pairs[grids[3] < 0, 0])


def test_rotations_select_different_patterns():
    """image 2 = image 1 turned in 45 degree steps: every angle is won by a pattern of its own"""
    winners = []
    for a in pr.ROTATION_ANGLES:
        case = BY_NAME['gms_rotation_%d' % a]
        pairs = pr.sort_clip(*case['fwd'])
        _mask, best, per_rot = pr.gms_loop(case['xy1'], case['xy2'], pr.SIZE, pairs, case['thr_factor'])
        assert best >= 0 and (per_rot < per_rot[best]).sum() == 7          # no tie for the first place
        winners.append(best)
        assert len(pr.expected(case)[0]) > 1500
    assert len(set(winners)) >= 4 and any(w != 0 for w in winners)
    assert winners[0] == 0


def test_dedupe_scenes_drop_what_they_say():
    want, stat = pr.expected(BY_NAME['dedupe_chain'])
    assert stat[0] - stat[1] == 12                              # two of every chain's four
    _want, stat = pr.expected(BY_NAME['dedupe_half_even'])
    assert stat[0] - stat[1] == 8                               # 0.125 | 0.12 ... on either side
    _want, stat = pr.expected(BY_NAME['dedupe_float32_print'])
    assert stat[0] - stat[1] == 4
    case = BY_NAME['dedupe_full_tables']
    for xy, rows in ((case['xy1'], case['fwd'][0]), (case['xy2'], case['fwd'][1])):
        keys = ["%.2f-%.2f" % tuple(p) for p in xy[rows].tolist()]
        assert len(keys) == 2000 and min(keys.count(k) for k in set(keys)) >= 2
    _want, stat = pr.expected(BY_NAME['dedupe_no_repeat'])
    assert stat == [2000] * 4
    for c in CASES:
        if c['name'].startswith(('dedupe_', 'gate_dedupe')):
            s = pr.expected(c)[1]
            assert s[0] == len(c['fwd'][0])                     # GMS is out of the way


def test_kp_key2_is_the_two_decimal_string():
    """matcher.kp_key2 feeds the kernel: equal keys <=> equal "%.2f-%.2f" strings, on every scene"""
    from imageanalysis_amd import matcher
    for c in CASES:
        if not c['name'].startswith(('dedupe_', 'gate_')):
            continue
        for xy in (c['xy1'], c['xy2']):
            keys = matcher.kp_key2(xy)
            text = ["%.2f-%.2f" % tuple(p) for p in xy.tolist()]
            assert [tuple(k) for k in keys.tolist()] == [(int(t.split('-')[0].replace('.', '')),
                                                          int(t.split('-')[1].replace('.', ''))) for t in text]


def test_gates_leave_minus_one_for_what_was_not_reached():
    for name, stat in (('sort_n24', [-1, -1, -1, -1]), ('sort_n25', [25, 25, 25, 25]),
                       ('gate_dedupe_leaves_25', [33, 25, 33, 25]), ('gate_dedupe_leaves_24', [32, 24, -1, -1]),
                       ('gate_fwd40_rev24', [40, 40, -1, -1]), ('gate_fwd40_rev25', [40, 40, 25, 25]),
                       ('gate_rev_dedupe_leaves_24', [40, 40, 25, 24])):
        want, got = pr.expected(BY_NAME[name])
        assert got == stat, name
        assert len(want) == (0 if -1 in stat or min(stat) < 25 else 25), name


def test_pack_reference():
    cnt, status, lists, z = pr.pack_inputs(50)
    total = int(cnt[status == 0].sum())
    off, out, out_z = pr.pack(cnt, status, lists, pr.PACK_CLIP, total + 3, z)
    assert off[-1] == total and (out[total:] == pr.PACK_FILL_I32).all() and (out_z[total:] == pr.PACK_FILL_F64).all()
    rows = np.concatenate([lists[k, :cnt[k]] for k in range(50) if status[k] == 0])
    assert np.array_equal(out[:total], rows)
    assert (status != 0).any() and cnt[status != 0].max() > 0 and (cnt == 0).mean() > 0.4
    off2, out2, _z = pr.pack(cnt, status, lists, pr.PACK_CLIP, total // 2)
    # cap below the total: the offsets are complete, the pairs that fit are where they were
    assert np.array_equal(off2, off) and len(out2) == total // 2
    last = np.nonzero((status == 0) & (cnt > 0) & (off[:-1] + cnt <= total // 2))[0].max()
    end = off[last] + cnt[last]
    assert np.array_equal(out2[:end], out[:end]) and (out2[end:] == pr.PACK_FILL_I32).all()
