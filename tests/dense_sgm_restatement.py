"""imageanalysis_amd/dense.py's SEMI-GLOBAL RULES restated in numpy: the uint8 cost of the sweep's
aggregate scores, the path recurrence (integers, a whole row or column of paths per step), the sum
over the directions and the select.  csrc/dense_sgm.hip and the emission in csrc/dense_sweep.hip are
held to these functions bit for bit; tests/test_dense_sgm.py holds the recurrence here to a per-pixel
Python loop."""
import numpy as np

import dense_restatement as dr

F32 = dr.F32
NAN32 = dr.NAN32
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))     # (dx, dy)
MAX_PLANES = 64


def cost_of(S):
    """float32 scores (NaN: invalid) -> uint8 costs: 255 invalid, else clamp(rint((1 - S) 127), 0, 254)"""
    S = np.asarray(S, F32)
    with np.errstate(invalid='ignore'):
        c = np.rint((F32(1.0) - S) * F32(127.0))
        c = np.minimum(np.maximum(c, F32(0.0)), F32(254.0))
    return np.where(np.isnan(S), F32(255.0), c).astype(np.uint8)


def max_cost_of(min_score):
    """q(min_score): the largest raw cost of a kept pixel"""
    return int(cost_of(np.array([min_score], F32))[0])


def score_stack(ref, nbs, w_far, w_near, planes, radius=3, min_var=4.0):
    """S_d(p) of every plane -> float32 [h, w, planes]"""
    step = dr.plane_step(w_far, w_near, planes)
    return np.stack([dr.aggregate(ref, nbs, 1.0 / (w_far + d * step), radius, min_var) for d in range(planes)], 2)


def volume(ref, nbs, w_far, w_near, planes, radius=3, min_var=4.0):
    """the cost volume of one reference view -> uint8 [h, w, planes]"""
    return cost_of(score_stack(ref, nbs, w_far, w_near, planes, radius, min_var))


def check_params(planes, paths, p1, p2, c_invalid):
    if not 2 <= planes <= MAX_PLANES:
        raise ValueError("planes")
    if paths not in (4, 8):
        raise ValueError("paths")
    if not 0 <= p1 <= p2 <= 255:
        raise ValueError("P1, P2")
    if not 0 <= c_invalid <= 254:
        raise ValueError("c_invalid")


def _step(Cw, prev, has_prev, p1, p2):
    """one step of many paths at once: Cw, prev [n, planes] int64, has_prev [n] bool"""
    big = 1 << 30
    m = prev.min(axis=1, keepdims=True)
    lo = np.full_like(prev, big)
    hi = np.full_like(prev, big)
    lo[:, 1:] = prev[:, :-1]
    hi[:, :-1] = prev[:, 1:]
    best = np.minimum(np.minimum(prev, np.minimum(lo, hi) + p1), m + p2)
    return np.where(has_prev[:, None], Cw + (best - m), Cw)


def path_cost(vol, direction, p1, p2, c_invalid=127):
    """L_r of one direction (dx, dy) -> int64 [h, w, planes]"""
    vol = np.asarray(vol, np.uint8)
    h, w, planes = vol.shape
    dx, dy = direction
    Cw = np.where(vol == 255, c_invalid, vol).astype(np.int64)
    L = np.zeros((h, w, planes), np.int64)
    if dy != 0:                                            # row after row, the row before shifted by dx
        xs = np.arange(w)
        src = xs - dx
        inside = (src >= 0) & (src < w)
        rows = range(h) if dy > 0 else range(h - 1, -1, -1)
        for y in rows:
            yp = y - dy
            if yp < 0 or yp >= h:
                L[y] = Cw[y]
                continue
            prev = L[yp][np.clip(src, 0, w - 1)]
            L[y] = _step(Cw[y], prev, inside, p1, p2)
    else:                                                  # column after column
        cols = range(w) if dx > 0 else range(w - 1, -1, -1)
        for x in cols:
            xp = x - dx
            if xp < 0 or xp >= w:
                L[:, x] = Cw[:, x]
                continue
            L[:, x] = _step(Cw[:, x], L[:, xp], np.ones(h, bool), p1, p2)
    return L


def aggregate(vol, paths=8, p1=16, p2=128, c_invalid=127):
    """T = the sum of L_r over the first `paths` directions -> uint16 [h, w, planes]"""
    vol = np.asarray(vol, np.uint8)
    check_params(vol.shape[2], paths, p1, p2, c_invalid)
    T = np.zeros(vol.shape, np.int64)
    for r in DIRECTIONS[:paths]:
        T += path_cost(vol, r, p1, p2, c_invalid)
    assert T.max() <= paths * (254 + p2) <= 4072
    return T.astype(np.uint16)


def select(total, vol, w_far, step, max_cost):
    """-> plane int32, cost uint8 (raw), tot0 uint16, depth float32 (NaN where not kept), all [h, w]"""
    T = np.asarray(total, np.uint16).astype(np.int64)
    vol = np.asarray(vol, np.uint8)
    h, w, planes = T.shape
    best = T.argmin(axis=2)                                # (the first of equal minima)
    yy, xx = np.mgrid[0:h, 0:w]
    t0 = T[yy, xx, best]
    tm = T[yy, xx, np.maximum(best - 1, 0)]
    tp = T[yy, xx, np.minimum(best + 1, planes - 1)]
    den = (tm - 2 * t0) + tp
    curved = (best > 0) & (best < planes - 1) & (den > 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        off = (tm - tp).astype(F32) / (2 * den).astype(F32)
        off = np.where(curved, np.minimum(np.maximum(off, F32(-0.5)), F32(0.5)), F32(0)).astype(F32)
        depth = (1.0 / (w_far + (best.astype(np.float64) + off.astype(np.float64)) * step)).astype(F32)
    raw = vol[yy, xx, best]
    kept = raw.astype(np.int64) <= max_cost
    depth = np.where(kept, depth, NAN32).astype(F32)
    return best.astype(np.int32), raw.astype(np.uint8), t0.astype(np.uint16), depth


def winner_of_scores(S, w_far, w_near, min_score=0.6):
    """THE RULES' winner-take-all from a score stack [h, w, planes] -> plane, score, depth (dr.sweep's,
    without sweeping again)"""
    S = np.asarray(S, F32)
    h, w, planes = S.shape
    step = dr.plane_step(w_far, w_near, planes)
    best = -np.ones((h, w), np.int32)
    s0, sm, sp, prev = (np.full((h, w), NAN32, F32) for _ in range(4))
    for d in range(planes):
        Sd = S[:, :, d]
        with np.errstate(invalid='ignore'):
            win = ~np.isnan(Sd) & ((best < 0) | (Sd > s0))
        after = ~win & (best >= 0) & (best == d - 1)
        sm = np.where(win, prev, sm)
        sp = np.where(win, NAN32, np.where(after, Sd, sp))
        s0 = np.where(win, Sd, s0)
        best = np.where(win, d, best).astype(np.int32)
        prev = Sd
    with np.errstate(invalid='ignore', divide='ignore'):
        den = (sm - F32(2) * s0) + sp
        curved = (best >= 0) & ~np.isnan(sm) & ~np.isnan(sp) & (den < 0)
        off = (F32(0.5) * (sm - sp)) / den
        off = np.where(curved, np.minimum(np.maximum(off, F32(-0.5)), F32(0.5)), F32(0)).astype(F32)
        kept = (best >= 0) & (s0 >= F32(min_score))
        depth = (1.0 / (w_far + (best.astype(np.float64) + off.astype(np.float64)) * step)).astype(F32)
    return best, s0.astype(F32), np.where(kept, depth, NAN32).astype(F32)


def sgm_of_scores(S, w_far, w_near, min_score=0.6, p1=16, p2=128, paths=8, c_invalid=127):
    """the semi-global chain from a score stack -> plane, cost, total, depth"""
    vol = cost_of(S)
    step = dr.plane_step(w_far, w_near, vol.shape[2])
    return select(aggregate(vol, paths, p1, p2, c_invalid), vol, w_far, step, max_cost_of(min_score))


def sgm(ref, nbs, w_far, w_near, planes, radius=3, min_var=4.0, min_score=0.6, p1=16, p2=128, paths=8, c_invalid=127):
    """one view, the whole chain -> plane int32, cost uint8, total uint16, depth float32"""
    check_params(planes, paths, p1, p2, c_invalid)
    S = score_stack(ref, nbs, w_far, w_near, planes, radius, min_var)
    return sgm_of_scores(S, w_far, w_near, min_score, p1, p2, paths, c_invalid)
