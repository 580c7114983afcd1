"""Plain reference of the per-pair match filters (csrc/match_post.hip) and the inputs that pin them.

postfilter() restates what iamx_match_postfilter computes for one image pair from pieces that are
not the code under test: numpy's stable argsort, imageanalysis_amd.gms.gms_inlier_mask (pinned to
the reference project's golden vectors by test_host_logic.py), a loop over "%.2f-%.2f" strings, a
python set.  pack() restates iamx_match_pack_results with np.cumsum.

`wrong=` selects one of four deliberately wrong rules.  A case names the wrong rule it is there to
catch (`case['wrong']`), and test_postfilter.py asserts that this rule changes the case's result:
a case on which the wrong rule gives the right answer would pass a wrong kernel too.

  'last_ties'    equal metrics: the LAST survivors in position order win (clip and order)
  'score_le'     GMS rejects a cell at score <= thresh instead of score < thresh
  'reserve'      a pair dropped as a duplicate still reserves its two position keys
  'argmax_last'  the best right cell of a left cell is the LARGEST one among equal counts

The case builders are shared by test_postfilter.py (CPU) and test_postfilter_edges_gpu.py.
"""
import math

import numpy as np

CLIP = 2000
GRID = 20
NCELL = GRID * GRID
SIZE = (2000, 2000)                 # every built scene: cells of 100 x 100 px
WRONG = ('last_ties', 'score_le', 'reserve', 'argmax_last')


# ------------------------------------------------------------------------------------------
# the rules
# ------------------------------------------------------------------------------------------
def sort_clip(q, t, metric, wrong=None):
    """[m,2] (q, t) of the CLIP best survivors in stable metric order"""
    metric = np.asarray(metric, np.float64)
    n = len(metric)
    if wrong == 'last_ties':
        order = np.lexsort((-np.arange(n), metric))[:CLIP]        # metric up, position DOWN
        if n > CLIP:
            # the wrong SET of ties in the right order: what a selection that counts the quota
            # from the wrong end leaves once the final sort has run
            order = order[np.lexsort((order, metric[order]))]
    else:
        order = np.argsort(metric, kind='stable')[:CLIP]
    return np.stack([np.asarray(q, np.int64)[order], np.asarray(t, np.int64)[order]], axis=1)


# rotation r of the 3x3 neighbourhood: the eight outer cells move r places round the ring
_RING = (0, 1, 2, 5, 8, 7, 6, 3)
ROT = np.zeros((8, 9), np.int64)
for _r in range(8):
    ROT[_r, 4] = 4
    for _i, _k in enumerate(_RING):
        ROT[_r, _k] = _RING[(_i - _r) % 8]


def _nb(c, k):
    x, y = c % GRID + (k % 3 - 1), c // GRID + (k // 3 - 1)
    return x + y * GRID if 0 <= x < GRID and 0 <= y < GRID else -1


def left_cells(xy, rows, size):
    """[4][n] left grid cell of every pair in the four half-cell shifted grids, -1 = outside"""
    lp = np.asarray(xy, np.float64)[rows] / np.array(size, np.float64)
    out = []
    for ox, oy in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)):
        x = np.floor(lp[:, 0] * GRID + ox).astype(np.int64)
        y = np.floor(lp[:, 1] * GRID + oy).astype(np.int64)
        out.append(np.where((x >= GRID) | (y >= GRID), -1, x + y * GRID))
    return out


def right_cells(xy, rows, size):
    rp = np.asarray(xy, np.float64)[rows] / np.array(size, np.float64)
    return (np.floor(rp[:, 0] * GRID).astype(np.int64)
            + np.floor(rp[:, 1] * GRID).astype(np.int64) * GRID)


def gms_loop(xy1, xy2, size, pairs, thr_factor, wrong=None):
    """GMS cell by cell (20 x 20 grids, four shifted left grids, eight rotations, no scales).
    Returns (mask [n] bool, winning rotation or -1, inliers of every rotation [8])."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    masks = np.zeros((8, n), bool)
    if n:
        rg = right_cells(xy2, pairs[:, 1], size)
        for lg in left_cells(xy1, pairs[:, 0], size):
            stats = np.zeros((NCELL, NCELL), np.int64)
            np.add.at(stats, (lg[lg >= 0], rg[lg >= 0]), 1)
            cnt = stats.sum(1)
            if wrong == 'argmax_last':
                jbest = NCELL - 1 - np.argmax(stats[:, ::-1], axis=1)
            else:
                jbest = np.argmax(stats, axis=1)
            for r in range(8):
                for c in np.nonzero(cnt)[0]:
                    score = tot = npair = 0
                    for k in range(9):
                        ll, rr = _nb(c, k), _nb(jbest[c], ROT[r, k])
                        if ll < 0 or rr < 0:
                            continue
                        npair += 1
                        tot += cnt[ll]
                        score += stats[ll, rr]
                    thresh = thr_factor * math.sqrt(float(tot) / max(npair, 1))
                    bad = score <= thresh if wrong == 'score_le' else score < thresh
                    if not bad:
                        masks[r] |= (lg == c) & (rg == jbest[c])
    per_rot = masks.sum(1)
    best = int(np.argmax(per_rot)) if n and per_rot.max() > 0 else -1       # first of the largest
    return (masks[best] if best >= 0 else np.zeros(n, bool)), best, per_rot


def dedupe(xy1, xy2, pairs, wrong=None):
    used1, used2, out = set(), set(), []
    for a, b in pairs:
        k1 = "%.2f-%.2f" % tuple(np.asarray(xy1)[a].tolist())
        k2 = "%.2f-%.2f" % tuple(np.asarray(xy2)[b].tolist())
        dup = k1 in used1 or k2 in used2
        if not dup or wrong == 'reserve':
            used1.add(k1)
            used2.add(k2)
        if not dup:
            out.append([int(a), int(b)])
    return out


def _one_direction(surv, xya, xyb, size, min_pairs, thr_factor, wrong):
    from imageanalysis_amd.gms import gms_inlier_mask
    pairs = sort_clip(*surv, wrong=wrong)
    if len(pairs) < min_pairs:
        return [], -1, -1
    if wrong in ('score_le', 'argmax_last'):
        mask = gms_loop(xya, xyb, size, pairs, thr_factor, wrong)[0]
    else:
        mask = gms_inlier_mask(xya, xyb, size, size, pairs, threshold_factor=thr_factor)
    kept = pairs[mask]
    out = dedupe(xya, xyb, kept, wrong)
    if len(out) < min_pairs:
        return [], len(kept), len(out)
    return out, len(kept), len(out)


def postfilter(fwd, rev, xy1, xy2, size, min_pairs, thr_factor, wrong=None):
    """fwd / rev: (q_rows, t_rows, metric) survivors of the two directions.  Returns (forward list
    [k,2] int64, [fwd after GMS, fwd after de-dup, rev after GMS, rev after de-dup]), -1 where a
    stage was not reached."""
    assert wrong is None or wrong in WRONG
    f, s0, s1 = _one_direction(fwd, xy1, xy2, size, min_pairs, thr_factor, wrong)
    stat = [s0, s1, -1, -1]
    r = []
    if len(f) >= min_pairs:
        r, stat[2], stat[3] = _one_direction(rev, xy2, xy1, size, min_pairs, thr_factor, wrong)
    back = set((a, b) for a, b in r)
    out = [p for p in f if (p[1], p[0]) in back]
    return np.array(out, np.int64).reshape(-1, 2), stat


def run_case(case, wrong=None):
    return postfilter(case['fwd'], case['rev'], case['xy1'], case['xy2'], SIZE, case['min_pairs'],
                      case['thr_factor'], wrong=wrong)


PACK_FILL_I32 = -123456789
PACK_FILL_F64 = -7.25e300


def pack(cnt, status, lists, clip, cap, z=None):
    """off [n+1] (exclusive scan of the counts of the status-0 pairs), out_pairs [cap,2] and out_z
    [cap] with the fill value wherever nothing is written"""
    cnt, status = np.asarray(cnt, np.int64), np.asarray(status, np.int64)
    n = len(cnt)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.where(status == 0, cnt, 0), out=off[1:])
    out = np.full((cap, 2), PACK_FILL_I32, np.int32)
    out_z = np.full(cap, PACK_FILL_F64, np.float64)
    lists = np.asarray(lists).reshape(n, clip, 2)
    for k in range(n):
        c = int(cnt[k])
        if status[k] != 0 or c <= 0 or off[k] + c > cap:
            continue
        out[off[k]:off[k] + c] = lists[k, :c]
        if z is not None:
            out_z[off[k]:off[k] + c] = np.asarray(z).reshape(n, clip)[k, :c]
    return off, out, out_z


# ------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------
def lattice_xy(n, cell):
    """n positions on a 0.25 px lattice inside the first quarter of grid cell `cell` = (cx, cy):
    at least 5 px from the cell's border and from its half-cell lines, distinct at two decimals"""
    assert n <= 160 * 160
    i = np.arange(n)
    return np.stack([100.0 * cell[0] + 5.0 + 0.25 * (i % 160),
                     100.0 * cell[1] + 5.0 + 0.25 * (i // 160)], axis=1).astype(np.float32)


def mirror(surv, keep=None, by_query=False):
    """the survivors of the reverse direction that mirror `surv` (optionally a subset of
    positions; optionally in query-row order, as the matching stage leaves them)"""
    q, t, m = np.asarray(surv[0]), np.asarray(surv[1]), np.asarray(surv[2], np.float64)
    idx = np.arange(len(q)) if keep is None else np.asarray(keep)
    if by_query:
        idx = idx[np.argsort(t[idx], kind='stable')]
    return t[idx].astype(np.int32), q[idx].astype(np.int32), np.asarray(m, np.float64)[idx]


def _case(name, fwd, rev, xy1, xy2, min_pairs=25, thr_factor=5.0, wrong=None, small=None):
    fwd = (np.asarray(fwd[0], np.int32), np.asarray(fwd[1], np.int32), np.asarray(fwd[2], np.float64))
    rev = (np.asarray(rev[0], np.int32), np.asarray(rev[1], np.int32), np.asarray(rev[2], np.float64))
    for s in (fwd, rev):
        assert np.isfinite(s[2]).all() and (s[2] >= 0).all()         # the kernel's stated domain
    if small is None:
        small = max(len(fwd[0]), len(rev[0])) <= 600
    return dict(name=name, fwd=fwd, rev=rev, xy1=np.asarray(xy1, np.float32),
                xy2=np.asarray(xy2, np.float32), min_pairs=min_pairs, thr_factor=thr_factor,
                wrong=wrong, small=small)


def isolation_case(name, metric, n_rev=None, wrong='last_ties', seed=0, **kw):
    """The isolation scene: every keypoint of image 1 inside one cell, every keypoint of image 2
    inside another, no position twice.  GMS keeps everything at factor 5.0 (one populated cell:
    score = tot = m, nine neighbours, m >= 5 sqrt(m / 9) from m = 3 on), nothing is a duplicate,
    and the reverse survivors mirror the forward ones in the same order with the same metrics --
    so the output is the sorted, clipped survivor list itself, in order."""
    rng = np.random.default_rng(seed)
    metric = np.asarray(metric, np.float64)
    n = len(metric)
    n_kp = n + 7
    xy1, xy2 = lattice_xy(n_kp, (1, 1)), lattice_xy(n_kp, (12, 7))
    fwd = (rng.permutation(n_kp)[:n], rng.permutation(n_kp)[:n], metric)
    keep = None
    if n_rev is not None and n_rev != n:
        # drop what the forward clip drops anyway: the survivors that sort last
        keep = np.sort(np.argsort(metric, kind='stable')[:n_rev])
    return _case(name, fwd, mirror(fwd, keep), xy1, xy2, wrong=wrong, **kw)


SORT_COUNTS = (0, 1, 24, 25, 1999, 2000, 2001, 2047, 2048, 2049, 2304, 2305, 4097)
SELECT_COUNTS = (2049, 2304, 2305, 4097)


def _tied_metric(n, seed):
    return np.random.default_rng(seed).choice(np.linspace(1.0, 50.0, 7), n)


def _straddle(m, rng):
    """three of the values above the CLIP-th smallest become equal to it: there are more ties of
    that value than the clip keeps, wherever the random draw put them"""
    t = np.sort(m)[CLIP - 1]
    above = np.nonzero(m > t)[0]
    m[rng.permutation(above)[:3]] = t
    return m


def select_metric(pattern, n, seed=0):
    """metrics of n > 2048 survivors for the radix select"""
    rng = np.random.default_rng(seed)
    if pattern == 'all_equal':
        return np.full(n, 7.5)
    if pattern == 'quota_1':
        # 1999 distinct smaller values, then one value to the end: the first of the ties is kept
        return np.concatenate([rng.permutation(1999) * 0.001 + 1.0, np.full(n - 1999, 3.0)])
    if pattern == 'distinct':
        # no ties at all: 1999 values below a unique 2000th
        return rng.permutation(n) * 0.25 + 0.5
    if pattern == 'low_byte':
        base = np.full(n, 123.456).view(np.int64) & ~0xFFFF
        return _straddle((base + rng.integers(0, 256, n)).view(np.float64), rng)
    if pattern == 'low_two_bytes':
        base = np.full(n, 123.456).view(np.int64) & ~0xFFFF
        return _straddle((base + rng.integers(0, 65536, n)).view(np.float64), rng)
    if pattern == 'exponents':
        m = 2.0 ** rng.integers(-1000, 1000, n)
        m[rng.permutation(n)[:40]] = 0.0
        m[rng.permutation(n)[:40]] = 5e-324
        return _straddle(m, rng)
    raise ValueError(pattern)


SELECT_PATTERNS = ('all_equal', 'quota_1', 'distinct', 'low_byte', 'low_two_bytes', 'exponents')


def quota_end_metric(n, end, extra, seed=0):
    """n survivors, 1700 below a value T, ties of T placed so that the 300-th tie -- the last one
    the clip keeps -- sits at position `end`, `extra` more ties behind it, the rest above T"""
    rng = np.random.default_rng(seed)
    quota, n_less = 300, CLIP - 300
    assert quota - 1 <= end < n and extra <= n - 1 - end and n_less + quota + extra <= n
    m = np.full(n, -1.0)
    m[rng.permutation(end)[:quota - 1]] = 10.0
    m[end] = 10.0
    if extra:
        m[end + 1 + rng.permutation(n - 1 - end)[:extra]] = 10.0
    free = np.nonzero(m < 0)[0]
    free = free[rng.permutation(len(free))]
    m[free[:n_less]] = rng.uniform(1.0, 9.0, n_less)
    m[free[n_less:]] = rng.uniform(11.0, 20.0, len(free) - n_less)
    return m


# The reverse of sort_f2048_r2049 has one survivor more than the forward direction: a mirror of a
# pair that is not in the forward list (it sorts last, the cross check has nothing to pair it with).
def _fix_f2048_r2049(case):
    q, t, m = case['rev']
    case['rev'] = (np.append(q, q[0]).astype(np.int32), np.append(t, t[1]).astype(np.int32),
                   np.append(m, 99.0))
    return case


def sort_cases():
    out = []
    for n in SORT_COUNTS:
        # (below the first gate nothing is left for a tie rule to change)
        wrong = 'last_ties' if n >= 25 else None
        if n <= 2048:
            out.append(isolation_case('sort_n%d' % n, _tied_metric(n, n), wrong=wrong, seed=n))
    out.append(isolation_case('sort_f2049_r2048', _tied_metric(2049, 5), n_rev=2048, seed=5))
    out.append(_fix_f2048_r2049(isolation_case('sort_f2048_r2049', _tied_metric(2049, 6)[:2048], seed=6)))
    for n in SELECT_COUNTS:
        for p in SELECT_PATTERNS:
            out.append(isolation_case('select_%s_n%d' % (p, n), select_metric(p, n, n),
                                      wrong=None if p == 'distinct' else 'last_ties', seed=n))
    # the kept ties end at lane 63 / 64 of a wave, at position 255 / 256 of a 256-chunk
    for n, chunk in ((2049, 5), (2304, 6), (4097, 11)):
        for pos in (63, 64, 255, 256):
            out.append(isolation_case('select_quota_end_%d_n%d' % (pos, n),
                                      quota_end_metric(n, 256 * chunk + pos, 9, seed=pos),
                                      seed=n + pos))
    # ... and in the last, partial chunk: its only element for the counts above (nothing behind it
    # for a tie rule to prefer), in the middle of it for 2100
    out.append(isolation_case('select_quota_end_last_n2305', quota_end_metric(2305, 2304, 0), wrong=None))
    out.append(isolation_case('select_quota_end_last_n4097', quota_end_metric(4097, 4096, 0), wrong=None))
    out.append(isolation_case('select_quota_end_partial_n2100', quota_end_metric(2100, 2070, 9)))
    return out


def threshold_lattice_case(thr_factor, name):
    """Four keypoints per cell at 0.25 / 0.75 of the cell, image 2 = image 1 shifted by (300, 200);
    the 1224 pairs that stay inside.  Interior cells score exactly 18 sqrt(tot / npair): the
    reference keeps 960 pairs at factor 18.0 and at the double below it, none at the double above."""
    c = np.arange(GRID)
    p = np.sort(np.concatenate([100.0 * c + 25.0, 100.0 * c + 75.0]))
    xy1 = np.stack(np.meshgrid(p, p), axis=-1).reshape(-1, 2)
    moved = xy1 + [300.0, 200.0]
    inside = np.nonzero((moved[:, 0] < SIZE[0]) & (moved[:, 1] < SIZE[1]))[0]
    xy2 = moved[inside]
    rng = np.random.default_rng(4)
    fwd = (inside, np.arange(len(inside)), rng.permutation(len(inside)) * 0.5 + 1.0)
    return _case(name, fwd, mirror(fwd, by_query=True), xy1, xy2, thr_factor=thr_factor,
                 wrong='score_le' if thr_factor == 18.0 else None, small=False)


def argmax_tie_case():
    """left cells whose matches split evenly between two (three) right cells: the smallest right
    cell wins, whichever of them the list names first"""
    blocks = (((2, 3), ((9, 9), (4, 4)), 30),            # larger cell first in the list
              ((6, 3), ((3, 12), (15, 12)), 28),
              ((10, 8), ((17, 2), (1, 16), (8, 5)), 26))
    xy1, xy2, q, t = [], [], [], []
    for lcell, rcells, k in blocks:
        for rc in rcells:
            q.extend(range(len(xy1), len(xy1) + k))
            t.extend(range(len(xy2), len(xy2) + k))
            xy1.extend(lattice_xy(len(xy1) + k, lcell)[len(xy1):].tolist())
            xy2.extend(lattice_xy(len(xy2) + k, rc)[len(xy2):].tolist())
    n = len(q)
    fwd = (q, t, np.arange(n) * 0.5 + 1.0)
    return _case('gms_argmax_tie', fwd, mirror(fwd, by_query=True), xy1, xy2, thr_factor=1.0,
                 wrong='argmax_last')


def border_case():
    """keypoints of image 1 in cell row / column 19, half of them in the last half cell (x or y
    >= 1950: the shifted grids have no cell for them), image 2 = image 1 moved by (-500, -300)"""
    rng = np.random.default_rng(8)
    n = 1400
    a = rng.integers(0, 4 * 2000, n) * 0.25                      # along the border
    b = 1800.0 + rng.integers(0, 4 * 200, n) * 0.25              # across it: cells 18, 19
    xy1 = np.where((np.arange(n) % 2 == 0)[:, None], np.stack([a, b], 1), np.stack([b, a], 1))
    xy1 = np.unique(xy1, axis=0)
    xy1 = xy1[(xy1[:, 0] >= 500.0) & (xy1[:, 1] >= 300.0)]
    xy1 = xy1[rng.permutation(len(xy1))]
    xy2 = xy1 - [500.0, 300.0]
    n = len(xy1)
    fwd = (np.arange(n), np.arange(n), rng.permutation(n) * 0.5 + 1.0)
    return _case('gms_last_row_col', fwd, mirror(fwd, by_query=True), xy1, xy2, small=False)


ROTATION_ANGLES = (0, 45, 90, 135, 180, 225, 270, 315)


def rotation_case(angle, thr_factor=5.0):
    """image 2 = image 1 rotated by `angle` degrees about the image centre"""
    rng = np.random.default_rng(21)
    n = 1900
    rad, phi = 690.0 * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2.0 * np.pi, n)
    p = np.stack([rad * np.cos(phi), rad * np.sin(phi)], 1)
    a = np.deg2rad(angle)
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    xy1 = (p + 1000.0).astype(np.float32)
    xy2 = (p @ rot.T + 1000.0).astype(np.float32)
    fwd = (np.arange(n), np.arange(n), rng.permutation(n) * 0.5 + 1.0)
    return _case('gms_rotation_%d' % angle, fwd, mirror(fwd, by_query=True), xy1, xy2,
                 thr_factor=thr_factor, small=False)


def _dedupe_case(name, pos_q, pos_t, row_q=None, row_t=None, wrong='reserve', **kw):
    """pairs in list order; pos_q[i] / pos_t[i] = (x, y) offsets inside the cell of image 1 / 2.
    Every pair gets keypoint rows of its own unless row_q / row_t name them."""
    pos_q, pos_t = np.asarray(pos_q, np.float64).reshape(-1, 2), np.asarray(pos_t, np.float64).reshape(-1, 2)
    n = len(pos_q)
    rng = np.random.default_rng(n)
    row_q = rng.permutation(n) if row_q is None else np.asarray(row_q)
    row_t = rng.permutation(n) if row_t is None else np.asarray(row_t)
    xy1, xy2 = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    xy1[row_q] = (pos_q + [105.0, 105.0]).astype(np.float32)
    xy2[row_t] = (pos_t + [1205.0, 705.0]).astype(np.float32)
    fwd = (row_q, row_t, np.arange(n) * 0.5 + 1.0)           # distinct metrics: list order = given
    return _case(name, fwd, mirror(fwd, by_query=True), xy1, xy2, wrong=wrong, **kw)


def _unique_pos(n, start=0):
    i = np.arange(start, start + n)
    return np.stack([0.25 * (i % 160), 20.0 + 0.25 * (i // 160)], 1)


def dedupe_cases():
    out = []
    # (a,b) (a,c) (d,c) (e,c): the second goes for a, and because it reserves nothing the third
    # stays; the fourth goes for c.  Six such chains between 40 pairs with positions of their own.
    pq, pt = list(_unique_pos(40)), list(_unique_pos(40))
    for j in range(6):
        a, d, e = (1.0 + j, 1.0), (1.0 + j, 2.0), (1.0 + j, 3.0)
        b, c = (1.0 + j, 5.0), (1.0 + j, 6.0)
        at = 5 * j + 3
        pq[at:at] = [a, a, d, e]
        pt[at:at] = [b, c, c, c]
    out.append(_dedupe_case('dedupe_chain', pq, pt))
    # k / 8: the exact half-way cases of "%.2f" (0.125 -> 0.12, 0.375 -> 0.38, 0.625 -> 0.62,
    # 0.875 -> 0.88), each followed by the two-decimal value it collides with and the one a
    # round-half-up would collide it with
    pq, pt = list(_unique_pos(30)), list(_unique_pos(30))
    for j, (half, same, other) in enumerate(((0.125, 0.12, 0.13), (0.375, 0.38, 0.37),
                                             (0.625, 0.62, 0.63), (0.875, 0.88, 0.87))):
        for v in (half, same, other):
            pq.append((3.0 + j + v, 1.0))
            pt.append(_unique_pos(1, 100 + len(pq))[0])
            pq.append(_unique_pos(1, 200 + len(pq))[0])
            pt.append((1.0, 3.0 + j + v))
    out.append(_dedupe_case('dedupe_half_even', pq, pt, wrong=None))
    # float32 values that differ but print alike, and values one float32 step apart on either
    # side of a rounding boundary, which print differently
    pq, pt = list(_unique_pos(30)), list(_unique_pos(30))
    lo = float(np.nextafter(np.float32(105.0 + 7.125), np.float32(0.0))) - 105.0
    hi = float(np.nextafter(np.float32(105.0 + 7.125), np.float32(1e9))) - 105.0
    for v in (7.121, 7.124, lo, hi, 7.1251, 7.1349):
        pq.append((v, 2.0))
        pt.append(_unique_pos(1, 100 + len(pq))[0])
    out.append(_dedupe_case('dedupe_float32_print', pq, pt, wrong=None))
    # 2000 pairs, every position three times on both sides, grouped differently on each
    rng = np.random.default_rng(77)
    gq, gt = rng.permutation(2000) // 3, rng.permutation(2000) // 3
    out.append(_dedupe_case('dedupe_full_tables', _unique_pos(667)[gq], _unique_pos(667)[gt], small=False))
    # 2000 pairs, no position twice: the early return
    out.append(_dedupe_case('dedupe_no_repeat', _unique_pos(2000), _unique_pos(2000), wrong=None,
                            small=False))
    return out


def gate_cases():
    """the min_pairs gates at their borders (exactly min_pairs after the clip: sort_n25 / sort_n24)"""
    out = []
    for left in (25, 24):
        # 33 / 32 survivors, four chains take two pairs each: `left` pairs after the de-duplication
        pq, pt = list(_unique_pos(left - 8)), list(_unique_pos(left - 8))
        for j in range(4):
            pq[3 * j:3 * j] = [(1.0 + j, 1.0), (1.0 + j, 1.0), (1.0 + j, 2.0), (1.0 + j, 3.0)]
            pt[3 * j:3 * j] = [(1.0 + j, 5.0), (1.0 + j, 6.0), (1.0 + j, 6.0), (1.0 + j, 6.0)]
        out.append(_dedupe_case('gate_dedupe_leaves_%d' % left, pq, pt,
                                wrong='reserve'))
    # the forward direction passes, the reverse has min_pairs - 1 survivors / exactly min_pairs
    for n_rev in (24, 25):
        c = isolation_case('gate_fwd40_rev%d' % n_rev, np.arange(40) * 0.5 + 1.0, n_rev=n_rev,
                           wrong=None, seed=n_rev)
        out.append(c)
    # ... and the reverse direction loses its 25th pair to the de-duplication: two reverse
    # survivors share a query position (rows of image 2 at one place), the forward list has only one
    c = isolation_case('gate_rev_dedupe_leaves_24', np.arange(40) * 0.5 + 1.0, n_rev=24, wrong=None, seed=3)
    q, t, m = c['rev']
    spare = int(np.setdiff1d(np.arange(len(c['xy2'])), c['fwd'][1])[0])
    c['xy2'][spare] = c['xy2'][q[0]]
    spare1 = int(np.setdiff1d(np.arange(len(c['xy1'])), c['fwd'][0])[0])
    c['rev'] = (np.append(q, spare).astype(np.int32), np.append(t, spare1).astype(np.int32), np.append(m, 50.0))
    out.append(c)
    return out


def gms_cases():
    out = [threshold_lattice_case(18.0, 'gms_threshold_equal'),
           threshold_lattice_case(float(np.nextafter(18.0, np.inf)), 'gms_threshold_above'),
           threshold_lattice_case(float(np.nextafter(18.0, 0.0)), 'gms_threshold_below'),
           argmax_tie_case(), border_case()]
    out.extend(rotation_case(a) for a in ROTATION_ANGLES)
    return out


def all_cases():
    cases = sort_cases() + gms_cases() + dedupe_cases() + gate_cases()
    names = [c['name'] for c in cases]
    assert len(set(names)) == len(names)
    return cases


_CACHE = {}


def cases():
    """all_cases(), built once per process (read only: the tests share them)"""
    if 'cases' not in _CACHE:
        _CACHE['cases'] = all_cases()
    return _CACHE['cases']


def expected(case):
    """the right rule's (list, stat) of a case, computed once"""
    key = ('want', case['name'])
    if key not in _CACHE:
        _CACHE[key] = run_case(case)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------
# packing / scan inputs
# ------------------------------------------------------------------------------------------
PACK_SIZES = (0, 1, 1023, 1024, 1025, 2049, 3000)
PACK_CLIP = 8


def pack_inputs(n, seed=0):
    """counts in [0, 8], about two thirds zero; some pairs with status 1 and a non-zero count"""
    rng = np.random.default_rng(1000 + n + seed)
    cnt = np.where(rng.random(n) < 2.0 / 3.0, 0, rng.integers(1, PACK_CLIP + 1, n)).astype(np.int32)
    status = (rng.random(n) < 0.1).astype(np.int32)
    if n >= 4:
        cnt[n // 2], status[n // 2] = 5, 1                 # a refused pair that has a count ...
        cnt[n - 1], status[n - 1] = 3, 0                   # ... and a last pair that has rows
    lists = rng.integers(0, 1 << 24, (n, PACK_CLIP, 2)).astype(np.int32)
    z = rng.normal(0.0, 100.0, (n, PACK_CLIP))
    return cnt, status, lists, z


SCAN_LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3001)


def scan_input(n):
    rng = np.random.default_rng(n)
    v = rng.integers(0, 1 << 31, n).astype(np.int32)
    if n:
        v[rng.integers(0, n, max(1, n // 8))] = (1 << 31) - 1
    return v
