"""Shared by tests/test_match_ratio.py (host), tests/test_match_ratio_gpu.py and
tools/gen_ratio_golden.py: the 'bestratio' strategy -- scripts/lib/matcher.py:595-694
ratio_pair_matches() -- restated in numpy with the RANSAC handed in as a callable, and the
constructed inputs of its cases.

* knn2_exact(): exact k=2 neighbours, ties to the lowest train row.
* ratio_pair(): guards, ratio, bins, tolerance, selection, result; every bin that passes the gate
  is handed to the callable (the kernels' shortcut for a bin that repeats the one before is NOT
  taken here, which is what checks it).
* host_ransac(): verify_reference.consensus() as that callable (this package's rule, float64).
* construct(): descriptors that put every query row at a chosen pair of squared distances (a to its
  train row, b to a decoy, in disjoint dimensions, every other row at 65025 or more), keypoints from
  verify_reference.scene() on the flat field -- at 100 m and a 30 m baseline 25 m of relief would be
  about 275 px of parallax, far over the tolerance of 33 px --, false matches displaced by at least
  5 tol.
* case(): the named cases of the goldens.

Needs numpy only; every input comes from a seed.
"""
import functools
import gzip
import os
import pickle
from math import sqrt

import numpy as np

import verify_reference as vr

CUTOFFS = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85]
MIN_UNIQUE = 20
W_PX, H_PX = vr.W_PX, vr.H_PX
HYPOTHESES, SEED = 256, 0
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('clean', 'early', 'below20', 'twentyone', 'gates', 'dups', 'exact', 'guards')


def tolerance(w, h):
    diag = int(sqrt(h * h + w * w))
    tol = int(round(diag * 0.005))
    return 5 if tol < 5 else tol


TOL = tolerance(W_PX, H_PX)


def knn2_exact(des_q, des_t):
    """(idx int32 [nq, 2], d2 int32 [nq, 2]): the two train rows of smallest squared distance,
    nearest first, equal distances by train row"""
    q, t = np.asarray(des_q).astype(np.int64), np.asarray(des_t).astype(np.int64)
    d = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)
    order = np.argsort(d, axis=1, kind='stable')[:, :2]
    return order.astype(np.int32), np.take_along_axis(d, order, 1).astype(np.int32)


def dedupe(xy1, xy2, pairs):
    """filter_duplicates (matcher.py:157-182): first come wins on the "%.2f-%.2f" keys"""
    used1, used2, out = set(), set(), []
    for a, b in pairs:
        k1 = "%.2f-%.2f" % (xy1[a][0], xy1[a][1])
        k2 = "%.2f-%.2f" % (xy2[b][0], xy2[b][1])
        if k1 in used1 or k2 in used2:
            continue
        used1.add(k1)
        used2.add(k2)
        out.append([int(a), int(b)])
    return out


def ratios(d2):
    """ratio of every row as Python doubles: float32 distances, one f64 division (matcher.py:619);
    raises what python raises where the second distance is 0"""
    d = np.sqrt(np.asarray(d2).astype(np.float64)).astype(np.float32)
    out = []
    for d0, d1 in d.tolist():
        if d1 == 0.0:
            raise ZeroDivisionError("float division by zero")
        out.append(d0 / d1)
    return out


def ratio_pair(idx, d2, xy1, xy2, n1, n2, tol, min_pairs, ransac, cutoffs=CUTOFFS, min_members=4):
    """steps 1-6 for one ordered pair.  idx / d2: the k = 2 neighbours of the n1 query rows (ignored
    under the guards); ransac(points float32 [n, 4], tol) -> bool mask [n], or None for a bin
    without a model.  -> dict(fwd, rev [m, 2] int32, stats [bins, 3] = members, fit, unique (-1
    where the bin is not looked at), chosen)"""
    nb = len(cutoffs)
    stats = np.full((nb, 3), -1, np.int32)
    stats[:, 0] = 0
    empty = np.zeros((0, 2), np.int32)
    res = dict(fwd=empty, rev=empty, stats=stats, chosen=-1)
    if n1 <= 1 or n2 <= 1:
        return res
    idx, xy1, xy2 = np.asarray(idx), np.asarray(xy1, np.float32), np.asarray(xy2, np.float32)
    bins = [[] for _ in cutoffs]
    for row, ratio in enumerate(ratios(d2)):
        for b, c in enumerate(cutoffs):
            if ratio <= c:
                bins[b].append(row)
    best, matches_best = MIN_UNIQUE, []
    for b, rows in enumerate(bins):
        stats[b, 0] = len(rows)
        # (cv2 raises below 4 points; the kernel's TOO_FEW would pass every match: skipped)
        if len(rows) >= min_pairs and len(rows) >= min_members:
            rows = np.asarray(rows, np.int64)
            train = idx[rows, 0].astype(np.int64)
            pts = np.concatenate([xy1[rows], xy2[train]], axis=1).astype(np.float32)
            mask = ransac(pts, tol)
            fit = [] if mask is None else [[int(q), int(t)] for q, t, m in zip(rows, train, mask) if m]
            unique = len(dedupe(xy1, xy2, fit))
            stats[b, 1], stats[b, 2] = len(fit), unique
            if unique > best:
                matches_best, best = fit, unique
                res['chosen'] = b
    if len(matches_best) >= min_pairs:
        pairs = dedupe(xy1, xy2, matches_best)
        if len(pairs) >= min_pairs:
            res['fwd'] = np.asarray(pairs, np.int32).reshape(-1, 2)
            res['rev'] = np.ascontiguousarray(res['fwd'][:, ::-1])
    return res


def host_ransac(hypotheses=HYPOTHESES, seed=SEED, log=None):
    """verify_reference.consensus() as ratio_pair's callable; log: a list that receives every
    consensus dict (tools/gen_ratio_golden.py reads the margins there)"""
    def run(pts, tol):
        c = vr.consensus(pts, float(tol), vr.HOMOGRAPHY, hypotheses, seed)
        if log is not None:
            log.append(c)
        if c['status'] != vr.OK:
            return None
        with np.errstate(invalid='ignore'):
            return c['err'][c['best'][0]] <= c['tol2']
    return run


# ---------------------------------------------------------------------------------------------
# constructed inputs
# ---------------------------------------------------------------------------------------------
BASE, FAR = 100, 255
CODE_DIMS = 12                          # query row i carries the bits of i as 0 / 255: 4096 rows
A_DIMS, B_DIMS, C_DIMS = (96, 97, 98, 99), (100, 101), (102, 103, 104, 105)


@functools.lru_cache(maxsize=None)
def _squares(a, k):
    """k non-negative integers <= 100 whose squares sum to a"""
    if k == 1:
        r = int(round(sqrt(a)))
        return (r,) if r * r == a and r <= 100 else None
    for x in range(min(100, int(sqrt(a))), -1, -1):
        rest = _squares(a - x * x, k - 1)
        if rest is not None:
            return (x,) + rest
    return None


def _code(i):
    v = np.full(128, BASE, np.int64)
    for bit in range(CODE_DIMS):
        v[bit] = FAR if (i >> bit) & 1 else 0
    return v


def spec(a, b=10000, true=True, twin_q=None, twin_t=None, onto=None, c=0):
    """one query row: squared distance a to its train row and b to the decoy; true: the train
    keypoint is where the plane maps the query keypoint (else displaced by >= 5 tol); twin_q = j:
    the query keypoint is the pixel of row j's; twin_t = j: the train keypoint is the pixel of row
    j's train keypoint; onto = j: no train rows of its own -- the row sits at squared distance c
    from query row j, so its neighbours are j's train row (a_j + c) and j's decoy (b_j + c)"""
    return dict(a=int(a), b=int(b), true=bool(true), twin_q=twin_q, twin_t=twin_t, onto=onto, c=int(c))


def for_ratio(r, b=10000):
    """the a that puts sqrt(a / b) nearest to r"""
    return int(round(r * r * b))


def construct(specs, seed):
    """-> dict(des1 uint8 [n, 128], xy1 float32 [n, 2], des2, xy2, want int32 [n]: the train row
    every query row must find first)"""
    rng = np.random.default_rng(seed)
    n = len(specs)
    assert n < (1 << CODE_DIMS)
    pts, _ = vr.scene(n, 1.0, 0.0, seed + 7)
    pts = pts.astype(np.float64)
    own = [i for i, s in enumerate(specs) if s['onto'] is None]
    slot = {i: k for k, i in enumerate(own)}
    perm = rng.permutation(2 * len(own))                  # train rows in a seeded order
    des1, des2 = np.zeros((n, 128), np.int64), np.zeros((2 * len(own), 128), np.int64)
    xy1, xy2 = np.zeros((n, 2)), np.zeros((2 * len(own), 2))
    want = np.zeros(n, np.int32)
    inside = lambda p: 40 < p[0] < W_PX - 40 and 40 < p[1] < H_PX - 40
    for i, s in enumerate(specs):
        xy1[i] = pts[i, :2]
        if s['onto'] is not None:
            continue
        t_row, d_row = perm[2 * slot[i]], perm[2 * slot[i] + 1]
        want[i] = t_row
        des1[i] = _code(i)
        des2[t_row] = _code(i)
        des2[t_row][list(A_DIMS)] += _squares(s['a'], 4)
        des2[d_row] = _code(i)
        des2[d_row][list(B_DIMS)] += _squares(s['b'], 2)
        assert s['a'] < s['b'] < FAR * FAR
        xy2[t_row] = pts[i, 2:]
        if not s['true']:
            while True:
                ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(5 * TOL + 5, 900.0)
                cand = pts[i, 2:] + mag * np.array([np.cos(ang), np.sin(ang)])
                if inside(cand):
                    xy2[t_row] = cand
                    break
        xy2[d_row] = [rng.uniform(40, W_PX - 40), rng.uniform(40, H_PX - 40)]
    for i, s in enumerate(specs):                         # rows that lean on another row
        j = s['onto'] if s['onto'] is not None else (s['twin_q'] if s['twin_q'] is not None else s['twin_t'])
        if j is None:
            continue
        if s['onto'] is not None:
            des1[i] = _code(j)
            des1[i][list(C_DIMS)] += _squares(s['c'], 4)
            want[i] = want[j]
            xy1[i] = pts[j, :2] + [0.29, -0.33]
        elif s['twin_q'] is not None:
            xy1[i] = xy1[j]
            xy2[want[i]] = xy2[want[j]] + [0.37, -0.21]
        else:
            xy1[i] = pts[j, :2] + [0.41, 0.23]
            xy2[want[i]] = xy2[want[j]]
    assert des1.min() >= 0 and des1.max() <= 255 and des2.min() >= 0 and des2.max() <= 255
    return dict(des1=des1.astype(np.uint8), xy1=xy1.astype(np.float32), des2=des2.astype(np.uint8),
                xy2=xy2.astype(np.float32), want=want)


def _shuffled(specs, seed):
    """the rows in a seeded order, cross references followed"""
    order = np.random.default_rng(seed).permutation(len(specs))
    where = np.empty(len(specs), np.int64)
    where[order] = np.arange(len(specs))
    out = []
    for k in order.tolist():
        s = dict(specs[k])
        for key in ('twin_q', 'twin_t', 'onto'):
            if s[key] is not None:
                s[key] = int(where[s[key]])
        out.append(s)
    return out


def _case_specs(name):
    """(list of query row specs, min_pairs, seed)"""
    rng = np.random.default_rng(abs(hash_name(name)))
    far = lambda k: [spec(for_ratio(r), true=False) for r in rng.uniform(0.9, 0.98, k)]
    if name == 'clean':
        s = [spec(for_ratio(r)) for r in np.linspace(0.3, 0.84, 300)]
        s += [spec(for_ratio(r), true=False) for r in rng.uniform(0.3, 0.84, 60)]
        return _shuffled(s + far(240), 11), 25, 101
    if name == 'early':
        s = [spec(for_ratio(r)) for r in np.linspace(0.3, 0.49, 40)]
        s += [spec(for_ratio(r), twin_q=k) for k, r in enumerate(np.linspace(0.52, 0.84, 12))]
        s += [spec(for_ratio(r), true=False) for r in rng.uniform(0.3, 0.84, 10)]
        return _shuffled(s + far(30), 12), 25, 102
    if name in ('below20', 'twentyone'):
        k = 20 if name == 'below20' else 21
        s = [spec(for_ratio(r)) for r in np.linspace(0.3, 0.84, k)]
        s += [spec(for_ratio(r), true=False) for r in rng.uniform(0.3, 0.84, 6)]
        return _shuffled(s + far(20), 13), 10, 103 if name == 'below20' else 104
    if name == 'gates':
        # bins of 24, 25 and 26 members at min_pairs = 25; three of the 26 share a pixel with an
        # earlier one: fit 26 >= 25, unique 23 > 20 is taken, and 23 < 25 empties the result
        s = [spec(for_ratio(r)) for r in np.linspace(0.3, 0.49, 21)]
        s += [spec(for_ratio(r), twin_q=k) for k, r in enumerate((0.35, 0.4))]
        s += [spec(for_ratio(0.45), twin_t=5)]
        s += [spec(for_ratio(0.52)), spec(for_ratio(0.57))]
        return _shuffled(s + far(12), 14), 25, 105
    if name == 'dups':
        s = [spec(for_ratio(r)) for r in np.linspace(0.3, 0.84, 60)]
        s += [spec(for_ratio(r), twin_q=k) for k, r in zip((3, 17, 40), (0.33, 0.58, 0.81))]
        s += [spec(for_ratio(r), twin_t=k) for k, r in zip((8, 22, 51), (0.47, 0.62, 0.79))]
        s += [spec(0, onto=k, c=c) for k, c in zip((5, 30), (400, 900))]
        s += [spec(for_ratio(r), true=False) for r in rng.uniform(0.3, 0.84, 12)]
        return _shuffled(s + far(40), 15), 25, 106
    if name == 'exact':
        s = [spec(25, 100) for _ in range(30)] + [spec(9, 16) for _ in range(10)]
        s += [spec(26, 100) for _ in range(10)]
        s += [spec(81, 100, true=False) for _ in range(14)]
        return _shuffled(s, 16), 25, 107
    raise KeyError(name)


def hash_name(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(pairs = [dict(des1, xy1, des2, xy2)], min_pairs, width, height) of a named case"""
    if name == 'guards':
        full = construct(_case_specs('twentyone')[0], 108)
        e = lambda n: dict(des=np.zeros((n, 128), np.uint8) + np.arange(n, dtype=np.uint8)[:, None],
                           xy=np.array([[100.5 + 7 * k, 200.25 + 3 * k] for k in range(n)], np.float32).reshape(n, 2))
        pair = lambda q, t: dict(des1=q['des'], xy1=q['xy'], des2=t['des'], xy2=t['xy'])
        big1, big2 = dict(des=full['des1'], xy=full['xy1']), dict(des=full['des2'], xy=full['xy2'])
        pairs = [pair(e(0), big2), pair(big1, e(0)), pair(e(1), big2), pair(big1, e(1)),
                 pair(e(2), e(2)), pair(e(2), big2)]
        return dict(pairs=pairs, min_pairs=10, width=W_PX, height=H_PX)
    specs, min_pairs, seed = _case_specs(name)
    c = construct(specs, seed)
    idx, d2 = knn2_exact(c['des1'], c['des2'])
    assert (idx[:, 0] == c['want']).all(), name          # the construction holds
    own = np.array([s['onto'] is None for s in specs])
    assert (d2[own, 0] == np.array([s['a'] for s in specs])[own]).all(), name
    assert (d2[own, 1] == np.array([s['b'] for s in specs])[own]).all(), name
    return dict(pairs=[{k: c[k] for k in ('des1', 'xy1', 'des2', 'xy2')}], min_pairs=min_pairs,
                width=W_PX, height=H_PX)


def restate(inp, ransac):
    """ratio_pair() for every pair of a case's inputs"""
    tol = tolerance(int(inp['width']), int(inp['height']))
    out = []
    for p in inp['pairs']:
        n1, n2 = len(p['des1']), len(p['des2'])
        idx, d2 = knn2_exact(p['des1'], p['des2']) if n1 > 1 and n2 > 1 else (None, None)
        out.append(ratio_pair(idx, d2, p['xy1'], p['xy2'], n1, n2, tol, inp['min_pairs'], ransac))
    return out


def load_golden(name):
    with gzip.open(os.path.join(GOLD, 'ratio_%s.pkl.gz' % name), 'rb') as f:
        return pickle.load(f)
