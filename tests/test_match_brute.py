"""The 'bruteforce' strategy without a GPU: the numpy restatement (tests/brute_reference.py) against
the goldens of the reference's own bruteforce_pair_matches (tools/gen_brute_golden.py), the
restatement's cells against the same binning written append by append, the argument checks of
the two new entry points, and the guards of matcher.bruteforce_pair_matches."""
import ctypes
from math import atan2, pi

import numpy as np
import pytest

import brute_reference as br

PAIR_GOLDENS = br.PAIR_CASES + ('guards',)


def cell_of_call(res):
    """the cells behind walk_cells()' calls, in walk order"""
    return [int(c) for c in np.nonzero(res['fit_cnt'] >= 0)[0]]


@pytest.mark.parametrize('name', PAIR_GOLDENS)
def test_restatement_equals_golden(name):
    """lists, every findHomography call of the walk (members, fitted) in order, the taken cells, and
    the per-bin lines the reference printed: by equality"""
    g = br.load_golden(name)
    res = br.restate(g, br.host_ransac(g['hypotheses'], g['seed']))
    assert len(res) == len(g['results'])
    for got, want in zip(res, g['results']):
        assert np.array_equal(got['fwd'], want['fwd']) and np.array_equal(got['rev'], want['rev'])
        assert got['calls'] == want['calls'] and got['taken'] == want['taken']
        assert got['lines'] == want['lines']
        # the chosen cell is the last call taken; the fitted counts per cell are the calls'
        cells = cell_of_call(got)
        assert [int(got['fit_cnt'][c]) for c in cells] == [f for _n, f in want['calls']]
        assert [int(got['bin_cnt'][c]) for c in cells] == [n for n, _f in want['calls']]
        assert got['chosen'] == (cells[want['taken'][-1]] if want['taken'] else -1)
        assert got['stats'][0] == (want['filtered'][-1][1] if want['filtered'] else 0)
        assert got['stats'][2] == len(want['lines']) and got['stats'][3] == len(want['calls'])


def test_the_zero_case_raises_in_the_reference_and_in_the_restatement():
    g = br.load_golden('zero')
    assert 'division by zero' in g['results'][0]['raised']
    with pytest.raises(ZeroDivisionError):
        br.restate(g, br.host_ransac(g['hypotheses'], g['seed']))


def test_goldens_show_what_their_names_say():
    res = {n: br.load_golden(n)['results'] for n in PAIR_GOLDENS}
    gold = {n: br.load_golden(n) for n in PAIR_GOLDENS}
    assert len(res['clean'][0]['fwd']) == 300 and len(res['clean'][0]['lines']) == 8      # the exit fired
    # choice: which neighbour the taken matches are
    p, fwd = gold['choice']['pairs'][0], res['choice'][0]['fwd']
    idx, d2 = br.knn3_exact(p['des1'], p['des2'])
    col = np.array([list(idx[q]).index(t) for q, t in fwd])
    assert (col == 0).sum() == 50 and (col == 1).sum() == 20 and (col == 2).sum() == 10
    equal = [q for q in range(len(idx)) if d2[q][0] == d2[q][1]]
    assert len(equal) == 10 and all(col[list(fwd[:, 0]).index(q)] == 0 for q in equal)
    # cuts: 84099 looked at and 84100 not; 150 / 200 is not below 0.75, 150 / sqrt(40001) is
    p, fwd = gold['cuts']['pairs'][0], res['cuts'][0]['fwd']
    idx, d2 = br.knn3_exact(p['des1'], p['des2'])
    got = [int(d2[q][list(idx[q]).index(t)]) for q, t in fwd]
    assert sorted(set(got) & {84099, 84100, 40000, 40001}) == [40000, 84099]
    assert got.count(84099) == 15 and got.count(40000) == 10 and len(fwd) == 55
    # angles: angle bins 0 and 20, rows that do not move, an angle just below 0
    p = gold['angles']['pairs'][0]
    idx, d2 = br.knn3_exact(p['des1'], p['des2'])
    chosen, _z = br.choose(idx, d2, p['xy1'], p['xy2'], p['size1'], p['size2'], 0.75)
    coded = br.codes(chosen, gold['angles']['step_d'])
    abins = np.array([c[3] for c in coded])
    assert (abins == 0).sum() >= 30 and (abins == 20).sum() >= 26 + 12 and (abins == 10).sum() >= 24
    still = [c for c in chosen if c[2] == 0.0]
    assert len(still) == 12 and all(c[3] == 0.0 for c in still)
    below = [c for c in chosen if 6.2831 < c[3] < 2 * pi]
    assert len(below) >= 12
    # dists: distance bins 0 and 40 are there, bin 41 is dropped
    p = gold['dists']['pairs'][0]
    idx, d2 = br.knn3_exact(p['des1'], p['des2'])
    chosen, _z = br.choose(idx, d2, p['xy1'], p['xy2'], p['size1'], p['size2'], 0.75)
    dall = np.array([int(round(float(c[2]) / gold['dists']['step_d'])) for c in chosen])
    assert (dall == 0).sum() >= 30 and (dall == 40).sum() >= 28 and (dall == 41).sum() >= 40
    assert max(c[2] for c in br.codes(chosen, gold['dists']['step_d'])) == 40
    a, b = res['gates']
    assert sorted(set(n for n, _f in a['calls'])) == [25] and len(a['fwd']) == 25          # the 24 are not looked at
    assert b['filtered'] == [(26, 26)] and len(b['fwd']) == 0                             # 23 unique < 25
    assert gold['small']['pairs'][0]['min_pairs'] == 3 and res['small'][0]['filtered'] == [(4, 4)]
    e = res['exit']
    assert [len(r['lines']) for r in e] == [5, 13, 11, 5]
    assert e[0]['lines'][-1][2:] == (9, 51, 9) and e[3]['lines'][-1][2:] == (0, 51, 0)
    assert e[1]['lines'][4][2:] == (0, 50, 0) and len(e[1]['fwd']) == 80                  # best 50: on
    assert e[2]['lines'][4][2:] == (10, 51, 10) and len(e[2]['fwd']) == 80                # best_of_bin 10: on
    assert len(e[0]['fwd']) == len(e[3]['fwd']) == 51
    assert res['dups'][0]['filtered'] == [(66, 66)] and len(res['dups'][0]['fwd']) == 60
    assert len(gold['two_rows']['pairs'][0]['des2']) == 2 and not len(res['two_rows'][0]['fwd'])
    assert all(not len(r['fwd']) and not r['lines'] and not r['calls'] for r in res['guards'])
    # the number the reference prints after a taken cell is not the bin (matcher.py:813 re-uses `i`)
    assert res['clean'][0]['lines'][4][:2] == (4, 300)


def append_by_append(chosen, diag):
    """the binning of matcher.py:756-795 in the order that code fills its lists -- a row goes to its
    own distance ring first, then the inner, then the outer one; within a ring to its own sector first,
    then to the two beside it, with the wrap as it stands -> {(ring, sector): [[query row, train row]]}"""
    width = int(diag * 0.55) / 40
    sector = 2 * pi / 20
    rings = [[] for _ in range(41)]
    for c in chosen:
        d = int(round(float(c[2]) / width))
        if d <= 40:
            for k in (d, d - 1, d + 1):
                if 0 <= k <= 40:
                    rings[k].append(c)
    beside = {0: (0, 20, 1), 20: (20, 19, 0)}
    out = {}
    for d, ring in enumerate(rings):
        sectors = [[] for _ in range(21)]
        for c in ring:
            a = int(round(c[3] / sector))
            for k in beside.get(a, (a, a - 1, a + 1)):
                sectors[k].append([c[0], c[1]])
        for a, members in enumerate(sectors):
            out[(d, a)] = members
    return out


def test_cells_equal_the_append_by_append_form():
    """random motions over the whole range, every angle bin and every distance bin up to past the
    last, the exact corners included; the append form puts a row into its own sector FIRST and into the
    neighbours after, so within a cell the order is the query-row order only because every row is in a
    cell once -- which is what the restatement's predicate form relies on"""
    rng = np.random.default_rng(5)
    diag = br.diagonal(br.W_PX, br.H_PX)
    step_d = br.step_dist(br.W_PX, br.H_PX)
    n = 4000
    ang = rng.uniform(-pi, pi, n)
    mag = rng.uniform(0, 42 * step_d, n)
    vx, vy = (mag * np.cos(ang)).astype(np.float32), (mag * np.sin(ang)).astype(np.float32)
    vx[:4], vy[:4] = [0, 100, -100, 100], [0, 0, 0, -2.0 ** -14]
    chosen = []
    for q in range(n):
        raw = np.float32(np.sqrt(np.float64(np.float32(vx[q] * vx[q]) + np.float32(vy[q] * vy[q]))))
        va = atan2(float(vy[q]), float(vx[q]))
        chosen.append((q, int(rng.integers(0, 9999)), raw, va + 2 * pi if va < 0 else va))
    want = append_by_append(chosen, diag)
    got = br.cells(br.codes(chosen, step_d))
    assert len(got) == br.NC == len(want)
    seen = set()
    for c, mem in enumerate(got):
        w = want[(c // br.NA, c % br.NA)]
        assert sorted(w) == sorted(mem) == mem, c
        assert len(set(q for q, _t in mem)) == len(mem)
        assert w == mem, c                              # (the append form's own order is the row order too)
        seen.update(q for q, _t in mem)
    dropped = set(range(n)) - seen
    assert dropped and all(int(round(float(chosen[q][2]) / step_d)) > 40 for q in dropped)
    per_row = np.bincount([q for mem in got for q, _t in mem], minlength=n)
    assert set(per_row.tolist()) == {0, 6, 9}           # distance bins 0 and 40 have one neighbour


def test_select_equals_the_walk_on_random_masks():
    """brute_reference.select() and walk_cells() are written apart: on cells with random masks and
    statuses they agree, the early exit included"""
    rng = np.random.default_rng(9)
    for trial in range(20):
        seg_cnt = np.zeros(br.NC, np.int32)
        for c in rng.choice(br.NC, 30, replace=False):
            seg_cnt[c] = rng.integers(4, 70)
        m = int(seg_cnt.sum())
        rows = np.stack([np.arange(m) % 500, rng.permutation(m) % 700], 1).astype(np.int32)
        mask = (rng.uniform(size=m) < rng.uniform(0.1, 1.0)).astype(np.uint8)
        vstatus = (rng.uniform(size=br.NC) < 0.1).astype(np.int32) * 2
        xy1, xy2 = rng.uniform(0, 4000, (500, 2)).astype(np.float32), rng.uniform(0, 4000, (700, 2)).astype(np.float32)
        got = br.select(seg_cnt, rows, mask, vstatus, xy1, xy2, 10)
        off = np.concatenate([[0], np.cumsum(seg_cnt)])
        members = [rows[off[c]:off[c + 1]].tolist() for c in range(br.NC)]
        fit_of = lambda c: (mask[off[c]:off[c + 1]] != 0) & (vstatus[c] == 0)
        want = br.walk_cells(members, fit_of, xy1, xy2, 4)
        # (walk_cells at min_pairs = 4 looks at exactly the cells handed in; its final gates are
        #  then at 4 too, so the lists are compared where both gates agree)
        assert got['chosen'] == want['chosen'] and np.array_equal(got['fit_cnt'], want['fit_cnt'])
        assert got['stats'][[0, 2, 3]].tolist() == want['stats'][[0, 2, 3]].tolist()
        if want['stats'][0] >= 10 and want['stats'][1] >= 10:
            assert np.array_equal(got['fwd'], want['fwd'])


def test_constants_agree():
    from imageanalysis_amd import _lib, kernels, matcher
    assert (kernels.BRUTE_DIST_BINS, kernels.BRUTE_ANGLE_BINS, kernels.BRUTE_CELLS) == (br.ND, br.NA, br.NC) == (41, 21, 861)
    assert kernels.BRUTE_STEP_A == br.STEP_A == 2 * pi / 20
    assert (matcher.BRUTE_MAX_DISTANCE, matcher.BRUTE_SIZE_RATIO) == (290, 1.25)
    assert (matcher.BRUTE_DIST_DIVS, matcher.BRUTE_ANGLE_DIVS) == (40, 20)
    assert matcher.BRUTE_HYPOTHESES == matcher.RATIO_HYPOTHESES == 2048
    text = open(_lib.HEADER_PATH).read()
    assert '#define IAMX_BRUTE_CELLS 861' in text and 'NumPy 1.20' in text
    for name in ('iamx_brute_bins', 'iamx_brute_select'):
        assert ('int %s(' % name) in text and hasattr(_lib.lib(), name)
    assert kernels.brute_bytes([]) == 0 and kernels.brute_bytes([100, 50]) > kernels.brute_bytes([100])
    assert kernels.brute_bytes([4096]) >= 4096 * (24 + 9 * 25 + 8) + 861 * 3 * 4


def test_new_entries_check_their_arguments_without_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                  # (an address that is never read)
    bins_args = (('idx', p), ('d2', p), ('row_off', p), ('pairs', p), ('kp_off', p), ('xy', p), ('size', p),
                 ('n_pairs', 1), ('match_ratio', 0.75), ('min_pairs', 25.0), ('step_d', 90.4),
                 ('step_a', br.STEP_A), ('cap', 9), ('bin_cnt', p), ('seg_cnt', p), ('seg_off', p), ('pts', p),
                 ('rows', p), ('flag', p), ('stream', None))
    select_args = (('pairs', p), ('kp_off', p), ('key2', p), ('n_pairs', 1), ('min_pairs', 25.0), ('seg_cnt', p),
                   ('seg_off', p), ('rows', p), ('mask', p), ('vstatus', p), ('cap', 9), ('stride', 1),
                   ('tab_size', 64), ('work', p), ('out_slots', p), ('out_cnt', p), ('out_off', p),
                   ('out_rows', p), ('out_cap', 1), ('chosen', p), ('stats', p), ('fit_cnt', p), ('flag', p),
                   ('stream', None))
    bins = lambda **kw: L.iamx_brute_bins(*[kw.get(k, d) for k, d in bins_args])
    select = lambda **kw: L.iamx_brute_select(*[kw.get(k, d) for k, d in select_args])
    for fn, spec in ((bins, bins_args), (select, select_args)):
        for name, default in spec:
            if default is p:
                assert fn(**{name: None}) == -1 and b'null pointer' in L.iamx_last_error(), name
        assert fn(n_pairs=-1) == -1 and b'negative' in L.iamx_last_error()
        assert fn(cap=-1) == -1
        assert fn(n_pairs=(1 << 31) // 861 + 1) == -1 and b'segments' in L.iamx_last_error()
        assert fn(n_pairs=0) == 0                          # nothing to do: no launch, no device
    odd = ctypes.c_void_p(p.value + 4)
    assert bins(pts=odd) == -1 and b'aligned' in L.iamx_last_error()
    assert bins(match_ratio=float('nan')) == -1
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert bins(step_d=bad) == -1 and b'steps' in L.iamx_last_error()
        assert bins(step_a=bad) == -1
    assert select(stride=0) == -1 and select(stride=(1 << 24) + 1, tab_size=1 << 26) == -1
    assert select(tab_size=48) == -1 and select(stride=64, tab_size=64) == -1 and select(tab_size=32) == -1
    assert select(out_cap=-1) == -1


class _Image(object):
    def __init__(self, des):
        self.des_list, self.kp_list, self.name = des, [], 'x'


def test_bruteforce_pair_matches_returns_nothing_under_the_guards():
    """raw_matches' guards (matcher.py:205-210) come before anything touches the device"""
    from imageanalysis_amd import matcher
    full = np.zeros((5, 128), np.float32)
    for a, b in ((None, full), (full, None), (np.float32(3.0), full), (full, np.float32(3.0)),
                 (full[:1], full), (full, full[:1]), (full[:0], full), (full, full[:0])):
        matcher.brute_last = 'stale'
        assert matcher.bruteforce_pair_matches(_Image(a), _Image(b)) == ([], [])
        assert matcher.bruteforce_pair_matches(_Image(a), _Image(b), review=True, hypotheses=64, seed=3) == ([], [])
        assert matcher.brute_last is None


def test_brute_tolerance_and_step():
    from imageanalysis_amd import matcher
    from imageanalysis_amd.hostlib import camera
    old = camera.get_image_params()
    try:
        for w, h in ((br.W_PX, br.H_PX), (640, 480), (1100, 300)):
            camera.set_image_params(w, h)
            assert matcher._brute_tol() == br.tolerance(w, h) and matcher._brute_step() == br.step_dist(w, h)
        camera.set_image_params(1100, 300)              # diag 1140: 5.7 truncates to 5 where round() gives 6
        assert matcher._brute_tol() == 5 and matcher._ratio_tol() == 6
    finally:
        camera.set_image_params(*old)


def test_the_log_lines_follow_the_reference(monkeypatch):
    """matcher._brute_log from per-cell figures: the lines the reference prints, its re-used `i` included"""
    from imageanalysis_amd import _deps, matcher
    g = br.load_golden('exit')
    res = br.restate(g, br.host_ransac(g['hypotheses'], g['seed']))
    for got, want in zip(res, g['results']):
        said = []

        class Log(object):
            def log(self, *a):
                said.append(' '.join(str(x) for x in a))
            qlog = log
        monkeypatch.setattr(_deps, 'logger', lambda: Log())
        matcher._brute_log(got['bin_cnt'], got['fit_cnt'], got['stats'][2])
        second = [s for s in said if s.startswith('bin:') and len(s.split()) == 6]
        assert second == ['bin: %d len: %d %d %d' % l[1:] for l in want['lines']]
        assert [s for s in said if s.startswith('Filtered')] == \
            ['Filtered matches: %d Fitted matches: %d' % f for f in want['filtered']]
