"""Shared by tests/test_match_brute.py (host), tests/test_match_brute_gpu.py and
tools/gen_brute_golden.py: the 'bruteforce' strategy -- scripts/lib/matcher.py:696-850
bruteforce_pair_matches() -- restated in numpy, and the constructed inputs of its cases.

* choose(): the per-row walk over the three neighbours (:711-754) -> the row's choice with its
  raw_dist (float32) and vangle (float).
* codes() / cells(): the distance and angle bin of every choice (:767, :785) and the 861 overlapping
  cells as MEMBERSHIP PREDICATES (a row is in cell (d, a) where d is within one of its distance bin
  and a is one of its three angle bins) -- tests/test_match_brute.py holds the same binning append by append,
  in the order the reference fills its lists, which is what checks this form.
* bins(): what iamx_brute_bins leaves for one pair: bin_cnt, seg_cnt, the materialised cells.
* walk_cells() / select() / brute_pair(): the walk over the cells with the early exit (:776-834), the
  gates and filter_duplicates (:839-850), with the fitted mask of a cell handed in as a callable --
  select() reads masks and statuses as iamx_brute_select does, brute_pair() asks a RANSAC callable for
  the cells the walk reaches, as the reference does.
* construct() / case(): descriptors that put every query row at chosen squared distances from up to
  three train rows of its own (smart_reference's code book), keypoints placed so that every
  neighbour's image-space motion is the vector the case names.

Needs numpy only; every input comes from a seed.
"""
import functools
import gzip
import os
import pickle
from math import atan2, pi, sqrt

import numpy as np

import smart_reference as sr
import verify_reference as vr
from smart_reference import dedupe, host_ransac, knn3_exact          # noqa: F401  (re-exported)

D2_NONE = sr.D2_NONE
ND, NA = 41, 21
NC = ND * NA
STEP_A = 2 * pi / 20
MATCH_RATIO = 0.75
W_PX, H_PX = vr.W_PX, vr.H_PX
HYPOTHESES, SEED = 256, 0
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def diagonal(w, h):
    return int(sqrt(h * h + w * w))


def tolerance(w, h):
    """matcher.py:760-761: int(), not int(round()) as in the 'bestratio' strategy"""
    tol = int(diagonal(w, h) * 0.005)
    return 5 if tol < 5 else tol


def step_dist(w, h):
    """matcher.py:756-759"""
    return int(diagonal(w, h) * 0.55) / 40


TOL, STEP_D = tolerance(W_PX, H_PX), step_dist(W_PX, H_PX)


# ---------------------------------------------------------------------------------------------
# the per-row choice and the cells
# ---------------------------------------------------------------------------------------------
def choose(idx, d2, xy1, xy2, s1, s2, match_ratio, on_zero='raise', log=None):
    """matcher.py:711-754 -> ([(query row, train row, raw_dist float32, vangle float)] in query-row
    order, rows whose nearest distance is 0).  on_zero = 'raise': what python raises at such a row;
    'count': the row has no choice (iamx_brute_bins' flag[0]).  log: a list that receives, per
    decision, ('ratio', value), ('size', value, exact) and, per row with a choice, ('row', [metric,
    ...], chosen position) for the generator's margins"""
    xy1, xy2 = np.asarray(xy1, np.float32), np.asarray(xy2, np.float32)
    dist = np.sqrt(np.asarray(d2).astype(np.float64)).astype(np.float32)
    out, zeros = [], 0
    for i in range(len(idx)):
        if d2[i][0] == 0:                               # ratio = 0.0 / 0.0 at j = 0
            if on_zero == 'raise':
                raise ZeroDivisionError("float division by zero")
            zeros += 1
            continue
        best, best_metric, pick, cands = -1, 9, None, []
        for j in range(3):
            if d2[i][j] >= 84100:                       # m[j].distance >= 290; a missing neighbour
                break
            ratio = float(dist[i][0]) / float(dist[i][j])
            if log is not None and j:
                log.append(('ratio', ratio))
            if ratio < match_ratio:
                break
            t = int(idx[i][j])
            v = xy2[t] - xy1[i]                         # float32
            raw = np.float32(np.sqrt(np.float64(np.float32(v[0] * v[0]) + np.float32(v[1] * v[1]))))
            vangle = atan2(float(v[1]), float(v[0]))
            if vangle < 0:
                vangle += 2 * pi
            a, b = float(s1[i]), float(s2[t])
            with np.errstate(all='ignore'):
                size_diff = np.float64(a) / np.float64(b) if a > b else np.float64(b) / np.float64(a)
            if log is not None:
                log.append(('size', float(size_diff), max(a, b) == 1.25 * min(a, b)))
            if size_diff > 1.25:
                continue
            metric = float(size_diff) / ratio
            cands.append(metric)
            if best < 0 or metric < best_metric:
                best, best_metric, pick, at = j, metric, (i, t, raw, vangle), len(cands) - 1
        if best >= 0:
            out.append(pick)
            if log is not None:
                log.append(('row', cands, at))
    return out, zeros


def codes(chosen, step_d, quotient=np.float64):
    """[(query row, train row, dbin, abin)] of the choices that are in a distance bin.  quotient:
    np.float64 is the reference's (NumPy 1.20: np.float32 / float is a float64 quotient); np.float32
    what the same expression gives under NumPy 2."""
    out = []
    for q, t, raw, vangle in chosen:
        if quotient is np.float64:
            x = float(raw) / step_d
        else:
            x = float(np.float32(raw) / np.float32(step_d))
        dbin = int(round(x))
        if dbin < ND:
            out.append((q, t, dbin, int(round(vangle / STEP_A))))
    return out


def in_cell(dbin, abin, cd, ca):
    if abs(cd - dbin) > 1:
        return False
    if abin == 0:
        return ca in (NA - 1, 0, 1)
    if abin == NA - 1:
        return ca in (NA - 2, NA - 1, 0)
    return abs(ca - abin) <= 1


def cells(coded):
    """the NC cells' members [[query row, train row]] in query-row order: every row is asked, for
    each cell of the three distance bins around its own, whether it belongs there"""
    out = [[] for _ in range(NC)]
    for q, t, dbin, abin in coded:
        for cd in range(max(dbin - 1, 0), min(dbin + 1, ND - 1) + 1):
            for ca in range(NA):
                if in_cell(dbin, abin, cd, ca):
                    out[cd * NA + ca].append([q, t])
    return out


def looked_at(n, min_pairs, min_members=4):
    # (cv2 raises below 4 points; the kernel's TOO_FEW would pass every match: skipped)
    return n >= min_pairs and n >= min_members


def bins(idx, d2, xy1, xy2, s1, s2, match_ratio, min_pairs, step_d):
    """what iamx_brute_bins leaves for one pair -> dict(bin_cnt [NC], seg_cnt [NC], pts float32 [m, 4],
    rows int32 [m, 2] the looked-at cells back to back, zeros, members)"""
    xy1, xy2 = np.asarray(xy1, np.float32), np.asarray(xy2, np.float32)
    chosen, zeros = choose(idx, d2, xy1, xy2, s1, s2, match_ratio, on_zero='count')
    members = cells(codes(chosen, step_d))
    bin_cnt = np.array([len(m) for m in members], np.int32)
    seg_cnt = np.array([len(m) if looked_at(len(m), min_pairs) else 0 for m in members], np.int32)
    rows = np.array([qt for m, n in zip(members, seg_cnt) if n for qt in m], np.int32).reshape(-1, 2)
    pts = np.concatenate([xy1[rows[:, 0]], xy2[rows[:, 1]]], axis=1).astype(np.float32).reshape(-1, 4)
    return dict(bin_cnt=bin_cnt, seg_cnt=seg_cnt, pts=pts, rows=rows, zeros=zeros, members=members)


# ---------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------
def walk_cells(members, fit_of, xy1, xy2, min_pairs):
    """matcher.py:776-850.  fit_of(cell) -> bool mask over the cell's members (all False for a cell
    without a model); asked only for the looked-at cells the walk reaches, in walk order.  -> dict(fwd,
    rev int32 [m, 2], chosen, stats int32 [4] = fitted, unique (-1: filter_duplicates did not run),
    distance bins walked, cells looked at within them, fit_cnt int32 [NC], calls [(members, fitted)]
    in walk order, taken: positions in calls of the cells that raised the best, lines [(dbin, the bin
    number the reference PRINTS, len, best, best_of_bin)]: the loop over a taken cell's matches
    (matcher.py:813) re-uses the name `i`, so after a taken cell the line at :831 shows that cell's
    last position instead of the bin)"""
    fit_cnt = np.full(NC, -1, np.int32)
    best, chosen, best_list, walked = 0, -1, [], 0
    calls, taken, lines = [], [], []
    for d in range(ND):
        best_of_bin, shown = 0, d
        for a in range(NA):
            c = d * NA + a
            mem = members[c]
            if not looked_at(len(mem), min_pairs):
                continue
            mask = np.asarray(fit_of(c)).astype(bool).reshape(-1)
            num_fit = int(np.count_nonzero(mask))
            fit_cnt[c] = num_fit
            calls.append((len(mem), num_fit))
            best_of_bin = max(best_of_bin, num_fit)
            if num_fit > best:
                best, chosen = num_fit, c
                best_list = [mem[k] for k in np.nonzero(mask)[0]]
                taken.append(len(calls) - 1)
                shown = len(mem) - 1
        walked = d + 1
        lines.append((d, shown, sum(len(members[d * NA + a]) for a in range(NA)) // 3, best, best_of_bin))
        if best > 50 and best_of_bin < 10:
            break
    empty = np.zeros((0, 2), np.int32)
    res = dict(fwd=empty, rev=empty, chosen=chosen, fit_cnt=fit_cnt, calls=calls, taken=taken, lines=lines)
    unique = -1
    if len(best_list) >= min_pairs:
        pairs = dedupe(xy1, xy2, best_list)
        unique = len(pairs)
        if len(pairs) >= min_pairs:
            res['fwd'] = np.asarray(pairs, np.int32).reshape(-1, 2)
            res['rev'] = np.ascontiguousarray(res['fwd'][:, ::-1])
    res['stats'] = np.array([best, unique, walked, len(calls)], np.int32)
    return res


def select(seg_cnt, rows, mask, vstatus, xy1, xy2, min_pairs):
    """what iamx_brute_select leaves for one pair: seg_cnt [NC] (> 0: the cell is looked at); rows [m, 2] /
    mask [m] the looked-at cells back to back; vstatus [NC] (0: a model) -> dict(fwd, chosen, fit_cnt,
    stats).  Written on its own, not through walk_cells(): the two check each other in the tests."""
    seg_cnt = np.asarray(seg_cnt, np.int64)
    off = np.concatenate([[0], np.cumsum(seg_cnt)])
    members = [np.asarray(rows)[off[c]:off[c + 1]].tolist() for c in range(NC)]
    fit_cnt = np.full(NC, -1, np.int32)
    best, chosen, best_list, walked, looked = 0, -1, [], 0, 0
    for d in range(ND):
        best_of_bin = 0
        for a in range(NA):
            c = d * NA + a
            if seg_cnt[c] <= 0:
                continue
            looked += 1
            m = np.asarray(mask)[off[c]:off[c + 1]] != 0
            if int(vstatus[c]) != 0:
                m = np.zeros(len(m), bool)
            num_fit = int(m.sum())
            fit_cnt[c] = num_fit
            best_of_bin = max(best_of_bin, num_fit)
            if num_fit > best:
                best, chosen, best_list = num_fit, c, [members[c][k] for k in np.nonzero(m)[0]]
        walked = d + 1
        if best > 50 and best_of_bin < 10:
            break
    out, unique = np.zeros((0, 2), np.int32), -1
    if chosen >= 0 and len(best_list) >= min_pairs:
        pairs = dedupe(xy1, xy2, best_list)
        unique = len(pairs)
        if unique >= min_pairs:
            out = np.asarray(pairs, np.int32).reshape(-1, 2)
    return dict(fwd=out, chosen=chosen, fit_cnt=fit_cnt, stats=np.array([best, unique, walked, looked], np.int32))


def brute_pair(idx, d2, xy1, xy2, s1, s2, n1, n2, tol, min_pairs, ransac, match_ratio=MATCH_RATIO,
               step_d=STEP_D, log=None):
    """matcher.py:696-850 for one ordered pair.  idx / d2: the k = 3 neighbours of the n1 query rows
    (ignored under the guards).  ransac(points float32 [n, 4], tol) -> (bool mask [n], model) or None
    for a cell without a model.  -> walk_cells()' dict plus bin_cnt [NC]; log: a list that receives
    choose()'s decisions and ('choice', query row, train row, raw_dist, vangle) per row (the
    generator's guard bands)."""
    empty = np.zeros((0, 2), np.int32)
    if n1 <= 1 or n2 <= 1:
        return dict(fwd=empty, rev=empty, chosen=-1, stats=np.array([0, -1, 0, 0], np.int32),
                    fit_cnt=np.full(NC, -1, np.int32), bin_cnt=np.zeros(NC, np.int32), calls=[], taken=[],
                    lines=[])
    xy1, xy2 = np.asarray(xy1, np.float32), np.asarray(xy2, np.float32)
    chosen, _zeros = choose(idx, d2, xy1, xy2, s1, s2, match_ratio, log=log)
    if log is not None:
        log.extend(('choice',) + c for c in chosen)
    members = cells(codes(chosen, step_d))

    def fit_of(c):
        m = np.asarray(members[c], np.int64)
        pts = np.concatenate([xy1[m[:, 0]], xy2[m[:, 1]]], axis=1).astype(np.float32)
        got = ransac(pts, tol)
        return np.zeros(len(m), bool) if got is None else np.asarray(got[0]).astype(bool)
    res = walk_cells(members, fit_of, xy1, xy2, min_pairs)
    res['bin_cnt'] = np.array([len(m) for m in members], np.int32)
    return res


# ---------------------------------------------------------------------------------------------
# constructed inputs
# ---------------------------------------------------------------------------------------------
ABSENT = sr.ABSENT                        # a neighbour past the cut at 290


def nbr(d2, v, size=1.0, twin_t=None):
    """one neighbour of a query row: squared distance; v = (vx, vy): its keypoint is the query
    keypoint moved by v; size: its kp.size over the query row's (a ratio that is exact in float32);
    twin_t = j: its keypoint is the pixel of row j's first neighbour's (the query keypoint follows)"""
    return dict(d2=int(d2), v=(float(v[0]), float(v[1])), size=size, twin_t=twin_t)


def row(*nbrs, at=None, twin_q=None):
    """a query row with up to three neighbours, nearest first; at = (x, y): its keypoint; twin_q = j:
    its keypoint is row j's (its first neighbour's a third of a pixel beside row j's)"""
    return dict(nbrs=list(nbrs), at=at, twin_q=twin_q)


def construct(rows, seed, sizes=(2.0, 3.2)):
    """-> dict(des1 uint8 [n, 128], xy1 float32 [n, 2], size1 float32 [n], des2, xy2, size2, want int32
    [n, 3], want_d2 int32 [n, 3]: the train rows every query row must find, in order).  Every query row
    owns three train rows; a neighbour the row does not name sits at ABSENT, far off in the image."""
    rng = np.random.default_rng(seed)
    n = len(rows)
    assert n < (1 << sr.CODE_BITS)
    perm = rng.permutation(3 * n)
    des1, des2 = np.zeros((n, 128), np.int64), np.zeros((3 * n, 128), np.int64)
    xy1, xy2 = np.zeros((n, 2)), np.zeros((3 * n, 2))
    size1 = np.round(rng.uniform(sizes[0], sizes[1], n) * 64) / 64        # (exact in float32, and x 1.25 too)
    size2 = np.zeros(3 * n)
    want, want_d2 = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.int32)
    inside = lambda p: 40 < p[0] < W_PX - 40 and 40 < p[1] < H_PX - 40
    for i, r in enumerate(rows):
        des1[i] = sr._code(i)
        named = len(r['nbrs'])
        ns = list(r['nbrs']) + [nbr(ABSENT + k, (0.0, 0.0)) for k in range(3 - named)]
        assert [x['d2'] for x in ns] == sorted(x['d2'] for x in ns)
        while True:                                          # a keypoint all of whose motions stay inside
            p = np.array(r['at'], float) if r['at'] is not None else \
                np.array([rng.uniform(40, W_PX - 40), rng.uniform(40, H_PX - 40)])
            if r['at'] is not None or all(inside(p + np.array(x['v'])) for x in ns[:named]):
                break
        xy1[i] = np.float32(p)
        trows = sorted(perm[3 * i:3 * i + 3].tolist())      # equal distances: the named order is the row order
        for k, (x, t) in enumerate(zip(ns, trows)):
            des2[t] = sr._code(i)
            sq = sr._squares(x['d2'], 6)
            assert sq is not None, x['d2']
            des2[t][list(sr.NBR_DIMS[k])] += sq
            want[i, k], want_d2[i, k] = t, x['d2']
            size2[t] = np.float32(size1[i]) * np.float32(x['size'])
            assert float(size2[t]) == size1[i] * x['size']          # the ratio is exact
            xy2[t] = xy1[i] + np.array(x['v']) if k < named else [rng.uniform(40, W_PX - 40), rng.uniform(40, H_PX - 40)]
    for i, r in enumerate(rows):                              # rows that lean on another row
        if r['twin_q'] is not None:
            xy1[i] = xy1[r['twin_q']]
            xy2[want[i, 0]] = xy1[i] + np.array(r['nbrs'][0]['v']) + [0.37, -0.21]
        for k, x in enumerate(r['nbrs']):
            if x['twin_t'] is not None:
                xy2[want[i, k]] = xy2[want[x['twin_t'], 0]]
                xy1[i] = xy2[want[i, k]] - np.array(x['v']) + [0.41, 0.23]
    assert des1.min() >= 0 and des1.max() <= 255 and des2.min() >= 0 and des2.max() <= 255
    return dict(des1=des1.astype(np.uint8), xy1=xy1.astype(np.float32), size1=size1.astype(np.float32),
                des2=des2.astype(np.uint8), xy2=xy2.astype(np.float32), size2=size2.astype(np.float32),
                want=want, want_d2=want_d2)


PAIR_CASES = ('clean', 'choice', 'cuts', 'angles', 'dists', 'gates', 'small', 'exit', 'dups', 'two_rows')
ALL_CASES = PAIR_CASES + ('guards', 'zero')
OFF = (2300.0, -1700.0)                   # where the cases send a neighbour that must not be the choice


def _case_rows(name):
    """[(rows, min_pairs, seed)] of a named case's pairs.  A `group` is a set of rows whose one true
    neighbour moves by the same vector up to a fifth of a pixel: one translation, so every hypothesis
    drawn from the group fits all of it, and all of it is in the same cells."""
    rng = np.random.default_rng(sr.hash_name('brute_' + name))
    d = lambda lo=2500, hi=60000: int(rng.integers(lo, hi))
    jit = lambda v: (v[0] + float(rng.uniform(-0.2, 0.2)), v[1] + float(rng.uniform(-0.2, 0.2)))
    group = lambda k, v: [row(nbr(d(), jit(v))) for _ in range(k)]

    def noise(k):                                            # one neighbour, moved anywhere
        out = []
        for _ in range(k):
            ang, mag = rng.uniform(0, 2 * pi), rng.uniform(60.0, 3000.0)
            out.append(row(nbr(d(), (mag * np.cos(ang), mag * np.sin(ang)))))
        return out
    V = (400.0, 150.0)                                       # raw 427.2: distance bin 5; 20.6 degrees: angle bin 1
    if name == 'clean':
        return [(sr._shuffled(group(300, V) + noise(100), 31), 25, 301)]
    if name == 'choice':
        s = group(30, V)
        # neighbour 0 fails the size test: 1 is the choice; 0 and 1 fail it: 2 is
        s += [row(nbr(a, OFF, size=2.0), nbr(a + 2000, jit(V))) for a in (d(40000, 50000) for _ in range(10))]
        s += [row(nbr(a, OFF, size=2.0), nbr(a + 1000, OFF, size=0.5), nbr(a + 2000, jit(V)))
              for a in (d(40000, 50000) for _ in range(10))]
        # equal metrics (equal distances, equal sizes): strict `<` keeps the earlier neighbour
        s += [row(nbr(a, jit(V)), nbr(a, OFF)) for a in (d() for _ in range(10))]
        # a later neighbour of a strictly smaller metric replaces it: 1.25 against 1 / 0.9
        s += [row(nbr(8100, OFF, size=1.25), nbr(10000, jit(V))) for _ in range(10)]
        # ... and one of a larger metric does not: 1 against 1.25 / 0.9
        s += [row(nbr(8100, jit(V)), nbr(10000, OFF, size=1.25)) for _ in range(10)]
        return [(sr._shuffled(s + noise(20), 32), 25, 302)]
    if name == 'cuts':
        s = group(30, V)
        s += [row(nbr(67500, OFF, size=2.0), nbr(84099, jit(V))) for _ in range(10)]   # 289.998: looked at
        s += [row(nbr(67500, OFF, size=2.0), nbr(84100, jit(V))) for _ in range(10)]   # 290: the walk stops
        s += [row(nbr(22500, OFF, size=2.0), nbr(40000, jit(V))) for _ in range(10)]   # 150 / 200 = 0.75: not below
        s += [row(nbr(22500, OFF, size=2.0), nbr(40001, jit(V))) for _ in range(10)]   # just below: the walk stops
        s += [row(nbr(84099, jit(V))) for _ in range(5)] + [row(nbr(84100, jit(V))) for _ in range(5)]
        return [(sr._shuffled(s, 33), 25, 303)]
    if name == 'angles':
        # angle bin 0 (cells 20, 0, 1) and angle bin 20 (cells 19, 20, 0), both in distance bin 3;
        # rows that do not move (raw 0, angle 0); rows whose angle is just below 0: angle bin 20
        s = group(30, (300.0, 20.0)) + group(26, (300.0, -20.0))
        s += [row(nbr(d(), (0.0, 0.0))) for _ in range(12)]
        s += [row(nbr(d(), (100.0, -2.0 ** -14)), at=(1000.0 + 3 * k, 1000.0 - 7 * k)) for k in range(12)]
        s += group(12, (-250.0, 3.0)) + group(12, (-250.0, -3.0))          # either side of pi: bin 10
        return [(sr._shuffled(s + noise(20), 34), 10, 304)]
    if name == 'dists':
        # distance bin 0 (bins 0, 1), bin 40 (bins 39, 40), bin 41 (dropped: 3700 / 90.4 = 40.9)
        s = group(30, (20.0, 5.0)) + group(28, (3616.0, 0.0)) + group(40, (3700.0, 0.0))
        return [(sr._shuffled(s + noise(20), 35), 25, 305)]
    if name == 'gates':
        # pair 0: a cell of exactly min_pairs members and one of min_pairs - 1.  pair 1: 26 rows, three
        # of them on the pixel of an earlier one: fitted 26 >= 25, unique 23 < 25 empties the result
        a = group(25, V) + group(24, (-900.0, 700.0))
        b = group(23, V) + [row(nbr(d(), jit(V)), twin_q=k) for k in (2, 9, 17)]
        return [(sr._shuffled(a, 36), 25, 306), (sr._shuffled(b, 37), 25, 307)]
    if name == 'small':
        # min_pairs < 4: a cell of 3 members is not looked at (a homography's sample), one of 4 is
        return [(group(3, V) + group(4, (-900.0, 700.0)), 3, 308)]
    if name == 'exit':
        g = lambda k, dbin: group(k, (90.4 * dbin, 0.0))
        return [
            # best 51, then a distance bin whose best is 9: the walk stops, the richer bin is not reached
            (sr._shuffled(g(51, 2) + g(9, 5) + g(80, 10), 38), 8, 309),
            # best 50 is not above 50: the walk goes on and meets the richer bin
            (sr._shuffled(g(50, 2) + g(80, 10), 39), 25, 310),
            # best_of_bin 10 is not below 10: on through bins 4 to 6; the richer bin starts at 7
            (sr._shuffled(g(51, 2) + g(10, 5) + g(80, 8), 40), 8, 311),
            # a distance bin without a looked-at cell stops it too, while a richer bin follows
            (sr._shuffled(g(51, 2) + g(80, 10), 41), 25, 312)]
    if name == 'dups':
        s = group(60, V)
        s += [row(nbr(d(), jit(V)), twin_q=k) for k in (3, 17, 40)]
        s += [row(nbr(d(), jit(V), twin_t=k)) for k in (8, 22, 51)]
        return [(sr._shuffled(s + noise(20), 42), 25, 313)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(pairs = [dict(des1, xy1, size1, des2, xy2, size2, min_pairs)], width, height, match_ratio)
    of a named case"""
    out = dict(pairs=[], width=W_PX, height=H_PX, match_ratio=MATCH_RATIO)
    keys = ('des1', 'xy1', 'size1', 'des2', 'xy2', 'size2')
    if name == 'two_rows':
        c = construct(_case_rows('clean')[0][0][:40], 314)
        keep = c['want'][:2, 0]                                   # a train image of exactly two rows
        out['pairs'].append(dict(des1=c['des1'], xy1=c['xy1'], size1=c['size1'], des2=c['des2'][keep],
                                 xy2=c['xy2'][keep], size2=c['size2'][keep], min_pairs=10))
        return out
    if name == 'guards':
        full = construct(_case_rows('small')[0][0], 315)
        e = lambda n: dict(des=np.zeros((n, 128), np.uint8) + np.arange(n, dtype=np.uint8)[:, None],
                           xy=np.array([[100.5 + 7 * k, 200.25 + 3 * k] for k in range(n)], np.float32).reshape(n, 2),
                           size=np.full(n, 2.5, np.float32))
        big1 = dict(des=full['des1'], xy=full['xy1'], size=full['size1'])
        big2 = dict(des=full['des2'], xy=full['xy2'], size=full['size2'])
        none = lambda q: dict(q, des=None)
        pair = lambda q, t: dict(des1=q['des'], xy1=q['xy'], size1=q['size'], des2=t['des'], xy2=t['xy'],
                                 size2=t['size'], min_pairs=3)
        out['pairs'] = [pair(e(0), big2), pair(big1, e(0)), pair(e(1), big2), pair(big1, e(1)),
                        pair(none(big1), big2), pair(big1, none(big2))]
        return out
    if name == 'zero':
        c = construct(_case_rows('small')[0][0], 316)
        c['des2'][c['want'][5, 0]] = c['des1'][5]                 # a row whose nearest distance is 0
        out['pairs'].append(dict({k: c[k] for k in keys}, min_pairs=3))
        return out
    for rows, min_pairs, seed in _case_rows(name):
        c = construct(rows, seed)
        idx, d2 = knn3_exact(c['des1'], c['des2'])
        assert np.array_equal(idx, c['want']) and np.array_equal(d2, c['want_d2']), name   # the construction holds
        out['pairs'].append(dict({k: c[k] for k in keys}, min_pairs=min_pairs))
    return out


def load_golden(name):
    with gzip.open(os.path.join(GOLD, 'brute_%s.pkl.gz' % name), 'rb') as f:
        return pickle.load(f)


def restate(inp, ransac, log=None):
    """brute_pair() for every pair of a case's inputs"""
    w, h = int(inp['width']), int(inp['height'])
    out = []
    for p in inp['pairs']:
        n1 = 0 if p['des1'] is None else len(p['des1'])
        n2 = 0 if p['des2'] is None else len(p['des2'])
        idx, d2 = knn3_exact(p['des1'], p['des2']) if n1 > 1 and n2 > 1 else (None, None)
        out.append(brute_pair(idx, d2, p['xy1'], p['xy2'], p['size1'], p['size2'], n1, n2, tolerance(w, h),
                              p['min_pairs'], ransac, inp['match_ratio'], step_dist(w, h), log))
    return out
