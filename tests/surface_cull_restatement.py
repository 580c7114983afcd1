"""numpy / Python restatement of the rules csrc/chain_surface.hip implements (include/iamx.h, DESIGN.md
section 4): the neighbour walk and line fit of the reference's scripts/4c-surface-outliers3.py, its
meta_stats() rule, and the depth metric of scripts/4c-by-depth.py, in today's matches_grouped layout.
Every sum is an explicit left-to-right loop over Python floats (IEEE doubles, one rounding per
operation); np.sum, which adds in pairs, is not used.  Nothing here imports the reference or the package."""
import math

import numpy as np

FITTED, SKIPPED_SMALL, SKIPPED_FLAT = 1, 2, 3


# ---------------------------------------------------------------------------------------------
# the observation table
# ---------------------------------------------------------------------------------------------
def looked_at(matches, group_index, alive=None):
    """chain indices with the group's tag, a position, and alive"""
    out = []
    for c, m in enumerate(matches):
        if m[1] != group_index or (alive is not None and not alive[c]):
            continue
        if m[0] is None:
            raise ValueError(c)
        out.append(c)
    return out


def observation_table(matches, in_group, group_index, alive=None, chains=None):
    """-> img_ptr i64 [n_images + 1], uv [n_obs, 2], ned [n_obs, 3], chain i32 [n_obs], and
    chain_ptr / chain_obs (each chain's observations in member order).  `chains`: the looked-at
    chains, when the caller has another rule for them."""
    n_img = len(in_group)
    if chains is None:
        chains = looked_at(matches, group_index, alive)
    rows = []                                                    # (image, u, v, chain) in member order
    chain_ptr = np.zeros(len(matches) + 1, np.int64)
    keep = set(chains)
    for c, m in enumerate(matches):
        if c in keep:
            for p in m[2:]:
                if not 0 <= p[0] < n_img:
                    raise IndexError(c)
                if in_group[p[0]]:
                    rows.append((p[0], p[1][0], p[1][1], c))
        chain_ptr[c + 1] = len(rows)
    img = np.array([r[0] for r in rows], np.int64)
    order = np.argsort(img, kind='stable')
    img_ptr = np.zeros(n_img + 1, np.int64)
    np.cumsum(np.bincount(img, minlength=n_img), out=img_ptr[1:])
    uv = np.array([[rows[o][1], rows[o][2]] for o in order], np.float64).reshape(-1, 2)
    chain = np.array([rows[o][3] for o in order], np.int32)
    ned = np.array([matches[c][0] for c in chain.tolist()], np.float64).reshape(-1, 3)
    chain_obs = np.zeros(len(rows), np.int32)
    chain_obs[order] = np.arange(len(rows), dtype=np.int32)
    return img_ptr, uv, ned, chain, chain_ptr, chain_obs


# ---------------------------------------------------------------------------------------------
# neighbours and fit
# ---------------------------------------------------------------------------------------------
def neighbours(uv_image, i, k):
    """(indices, d2) of the first min(k, n) observations of one image in ascending (d2, index)"""
    du = uv_image[i, 0] - uv_image[:, 0]
    dv = uv_image[i, 1] - uv_image[:, 1]
    d2 = du * du + dv * dv
    order = np.lexsort((np.arange(len(d2)), d2))[:k]
    return order, d2[order]


def walk(d2_sorted, n_pos):
    """how many of the listed neighbours the reference's double loop uses"""
    positives = m = 0
    for d2 in d2_sorted.tolist():
        if d2 > 0:
            positives += 1
        if positives > n_pos:
            break
        m += 1
    return m


def dist3(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def line(xs, ys):
    """closed-form least-squares line through (x, y): (a, b) or None when sxx == 0"""
    m = len(xs)
    sx = sy = 0.0
    for x, y in zip(xs, ys):
        sx = sx + x
        sy = sy + y
    xm, ym = sx / m, sy / m
    sxx = sxy = 0.0
    for x, y in zip(xs, ys):
        ex, ey = x - xm, y - ym
        sxx = sxx + ex * ex
        sxy = sxy + ex * ey
    if sxx == 0.0:
        return None
    a = sxy / sxx
    return a, ym - a * xm


def knn_fit(img_ptr, uv, ned, chain, k=30, n_pos=10):
    """-> tgt i32 [n_obs, k], val [n_obs, k], used i32, fit [n_obs, 2], status i32"""
    n_obs = len(uv)
    tgt = np.full((n_obs, k), -1, np.int32)
    val = np.zeros((n_obs, k))
    used = np.zeros(n_obs, np.int32)
    fit = np.zeros((n_obs, 2))
    status = np.zeros(n_obs, np.int32)
    ned_l = ned.tolist()
    for im in range(len(img_ptr) - 1):
        lo, hi = int(img_ptr[im]), int(img_ptr[im + 1])
        n = hi - lo
        if n < 3:
            status[lo:hi] = SKIPPED_SMALL
            continue
        uv_image = uv[lo:hi]
        for i in range(n):
            idx, d2 = neighbours(uv_image, i, min(k, n))
            m = walk(d2, n_pos)
            js = [lo + int(j) for j in idx[:m]]
            xs = [math.sqrt(v) for v in d2[:m].tolist()]
            ys = [dist3(ned_l[lo + i], ned_l[j]) for j in js]
            ab = line(xs, ys)
            if ab is None:
                status[lo + i] = SKIPPED_FLAT
                continue
            a, b = ab
            status[lo + i] = FITTED
            used[lo + i] = m
            fit[lo + i] = (a, b)
            for s, (j, x, y) in enumerate(zip(js, xs, ys)):
                tgt[lo + i, s] = chain[j]
                val[lo + i, s] = abs((a * x + b) - y)
    return tgt, val, used, fit, status


def chain_metric(tgt, val, n_chains):
    """-> sum, count, metric: contributions in ascending (observation, slot) order"""
    total = [0.0] * n_chains
    count = [0] * n_chains
    for t, v in zip(tgt.ravel().tolist(), val.ravel().tolist()):
        if 0 <= t < n_chains:
            total[t] = total[t] + v
            count[t] += 1
    metric = [s / n if n else 0.0 for s, n in zip(total, count)]
    return np.array(total, np.float64), np.array(count, np.int32), np.array(metric, np.float64)


# ---------------------------------------------------------------------------------------------
# statistics and flags
# ---------------------------------------------------------------------------------------------
def outlier_stats(metric, looked, factor, two_sided):
    """-> (average, stddev, flag bool [n], smallest relative distance of a looked-at chain from its
    threshold).  n == 0 or stddev == 0: nothing is flagged."""
    vals = [v for v, l in zip(np.asarray(metric, np.float64).tolist(), np.asarray(looked).tolist()) if l]
    n = len(vals)
    flag = np.zeros(len(metric), bool)
    if n == 0:
        return 0.0, 0.0, flag, math.inf
    s = 0.0
    for v in vals:
        s = s + v
    average = s / n
    s = 0.0
    for v in vals:
        d = average - v
        s = s + d * d
    stddev = math.sqrt(s / n)
    if not stddev > 0.0:
        return average, stddev, flag, math.inf
    band = factor * stddev
    margin = math.inf
    for c in np.nonzero(looked)[0].tolist():
        v = float(metric[c])
        if two_sided:
            flag[c] = abs(average - v) >= band
            margin = min(margin, abs(abs(average - v) - band) / band) if band > 0 else margin
        else:
            flag[c] = v > average + band
            margin = min(margin, abs(v - (average + band)) / (average + band))
    return average, stddev, flag, margin


def surface_round(matches, in_group, group_index, alive, k=30, n_pos=10, stddev=5):
    """one pass of the reference's compute_surface_outliers(): -> dict"""
    img_ptr, uv, ned, chain, _cp, _co = observation_table(matches, in_group, group_index, alive)
    tgt, val, used, fit, status = knn_fit(img_ptr, uv, ned, chain, k, n_pos)
    total, count, metric = chain_metric(tgt, val, len(matches))
    looked = np.zeros(len(matches), bool)
    looked[looked_at(matches, group_index, alive)] = True
    average, sd, flag, margin = outlier_stats(metric, looked, stddev, True)
    culled = np.nonzero(flag)[0]
    culled = culled[np.argsort(-np.abs(metric[culled]), kind='stable')]
    return dict(culled=culled.tolist(), average=average, stddev=sd, margin=margin, metric=metric,
                count=count, looked=looked, n_small=int(np.sum(status == SKIPPED_SMALL)),
                n_flat=int(np.sum(status == SKIPPED_FLAT)),
                n_uncounted=int(np.sum(looked & (count == 0))))


def cull_surface(matches, in_group, group_index, k=30, n_pos=10, stddev=5, max_rounds=None):
    """the reference's `while result > 0` loop on an alive mask -> list of round dicts (the last
    one culls nothing unless max_rounds ended the loop)"""
    alive = np.ones(len(matches), bool)
    rounds = []
    while max_rounds is None or len(rounds) < max_rounds:
        r = surface_round(matches, in_group, group_index, alive, k, n_pos, stddev)
        rounds.append(r)
        if not r['culled']:
            break
        alive[r['culled']] = False
    return rounds


# ---------------------------------------------------------------------------------------------
# depths
# ---------------------------------------------------------------------------------------------
def depth_chains(matches, in_group, group_index):
    """the chains scripts/4c-by-depth.py looks at: the group's, with a position and >= 2 members
    in the group"""
    out = []
    for c in looked_at(matches, group_index):
        if sum(1 for p in matches[c][2:] if 0 <= p[0] < len(in_group) and in_group[p[0]]) >= 2:
            out.append(c)
    return out


def chain_depths(img_ptr, ned, pos, chain_ptr, chain_obs):
    """-> depth [n_obs], z [n_images, 3] (mean, population deviation, count), metric [n_chains],
    looked bool [n_chains]"""
    n_img = len(img_ptr) - 1
    n_obs = len(ned)
    image_of = np.repeat(np.arange(n_img), np.diff(img_ptr))
    depth = np.array([dist3(ned[o], pos[image_of[o]]) for o in range(n_obs)], np.float64)
    z = np.zeros((n_img, 3))
    for im in range(n_img):
        d = depth[img_ptr[im]:img_ptr[im + 1]].tolist()
        if not d:
            continue
        s = 0.0
        for v in d:
            s = s + v
        mean = s / len(d)
        s = 0.0
        for v in d:
            s = s + (v - mean) * (v - mean)
        z[im] = (mean, math.sqrt(s / len(d)), len(d))
    n_chains = len(chain_ptr) - 1
    metric = np.zeros(n_chains)
    looked = np.zeros(n_chains, bool)
    for c in range(n_chains):
        obs = chain_obs[chain_ptr[c]:chain_ptr[c + 1]].tolist()
        if len(obs) < 2:
            continue
        s = 0.0
        for o in obs:
            s = s + abs(float(depth[o]) - float(z[image_of[o], 0]))
        metric[c] = s / len(obs)
        looked[c] = True
    return depth, z, metric, looked


def depth_outliers(matches, in_group, group_index, pos, stddev=3):
    """-> (mark list [[chain, 0], ...] by descending metric, stable; z; average; deviation; margin)"""
    chains = depth_chains(matches, in_group, group_index)
    img_ptr, _uv, ned, _chain, chain_ptr, chain_obs = observation_table(matches, in_group, group_index,
                                                                        chains=chains)
    _depth, z, metric, looked = chain_depths(img_ptr, ned, pos, chain_ptr, chain_obs)
    average, sd, flag, margin = outlier_stats(metric, looked, stddev, False)
    idx = np.nonzero(flag)[0]
    idx = idx[np.argsort(-metric[idx], kind='stable')]
    return [[int(c), 0] for c in idx], z, average, sd, margin


def weak_images(matches, n_images, min_features=25):
    """[chain, member] of every unmarked member in an image holding 1 .. min_features - 1 unmarked
    members"""
    count = [0] * n_images
    for m in matches:
        for p in m[2:]:
            if p != [-1, -1]:
                count[p[0]] += 1
    weak = set(i for i, n in enumerate(count) if 0 < n < min_features)
    return [[c, j] for c, m in enumerate(matches) for j, p in enumerate(m[2:])
            if p != [-1, -1] and p[0] in weak]


# ---------------------------------------------------------------------------------------------
# the planted scene of tests/test_surface_cull.py and tests/test_surface_cull_gpu.py
# ---------------------------------------------------------------------------------------------
FC6310S = dict(fx=3648.0, fy=3648.0, cu=2736.0, cv=1824.0, width=5472, height=3648)


def planted_scene(seed=5, n_points=600, n_bad=6):
    """12 nadir cameras on a 3 x 4 grid at 100 m, n_points ground points on gentle relief, pair-wise
    chains (one per pair of neighbouring cameras that see the point, as the matcher makes them),
    n_bad chains displaced vertically by 15 .. 40 m.  -> (matches, cam positions [12, 3], planted)"""
    rng = np.random.default_rng(seed)
    cam = np.array([[60.0 * r, 60.0 * c, -100.0] for r in range(3) for c in range(4)])
    K = FC6310S
    pts = np.stack([rng.uniform(-40, 160, n_points), rng.uniform(-40, 220, n_points),
                    rng.uniform(-1.0, 1.0, n_points)], 1)
    matches = []
    for p in pts:
        seen = []
        for i, c in enumerate(cam):
            d = p - c                                            # nadir: camera x = east, y = -north, z = down
            u = K['cu'] + K['fx'] * d[1] / d[2]
            v = K['cv'] - K['fy'] * d[0] / d[2]
            if 0 <= u < K['width'] and 0 <= v < K['height']:
                seen.append([i, [float(u + rng.normal(0, 0.3)), float(v + rng.normal(0, 0.3))]])
        for a in range(len(seen) - 1):                           # pair-wise chains of one feature
            matches.append([p.tolist(), 0, [seen[a][0], list(seen[a][1])],
                            [seen[a + 1][0], list(seen[a + 1][1])]])
    planted = sorted(rng.choice(len(matches), n_bad, replace=False).tolist())
    for c, dz in zip(planted, rng.uniform(15, 40, n_bad) * rng.choice([-1.0, 1.0], n_bad)):
        matches[c][0] = [matches[c][0][0], matches[c][0][1], matches[c][0][2] + float(dz)]
    return matches, cam, planted
