"""csrc/terrain.hip once more in numpy float64, in the kernels' own order of operations: the interval
from a uniform guess corrected against the axis, scipy's bilinear blend multiplied and summed left to
right, and lib/srtm.py's interpolate_vector with every ray advanced under a mask."""
import numpy as np

FILL = -32768.0
SKY, CAPPED, LEFT_GRID = 1, 2, 4


def find_interval(a, x):
    n = len(a)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        f = (x - a[0]) * (float(n - 1) / (a[n - 1] - a[0]))
        i = np.where(f > 0.0, np.where(f < float(n - 2), np.trunc(np.where(f < float(n - 2), f, 0.0)), n - 2), 0)
    i = i.astype(np.int64)
    while True:
        m = (i > 0) & (x < a[i])
        if not m.any():
            break
        i[m] -= 1
    while True:
        m = (i < n - 2) & (x >= a[np.minimum(i + 1, n - 1)])
        if not m.any():
            break
        i[m] += 1
    return i


def look_up(axis_n, axis_e, grid, n, e):
    """-> value [N], outside [N] bool"""
    n, e = np.asarray(n, np.float64), np.asarray(e, np.float64)
    nan = np.isnan(n) | np.isnan(e)
    with np.errstate(invalid='ignore'):
        outside = ~nan & ((n < axis_n[0]) | (n > axis_n[-1]) | (e < axis_e[0]) | (e > axis_e[-1]))
    ok = ~nan & ~outside
    out = np.where(nan, np.nan, FILL)
    if ok.any():
        nn, ee = n[ok], e[ok]
        i, j = find_interval(axis_n, nn), find_interval(axis_e, ee)
        y0 = (nn - axis_n[i]) / (axis_n[i + 1] - axis_n[i])
        y1 = (ee - axis_e[j]) / (axis_e[j + 1] - axis_e[j])
        out[ok] = grid[i, j] * (1.0 - y0) * (1.0 - y1) + grid[i, j + 1] * (1.0 - y0) * y1 + \
            grid[i + 1, j] * y0 * (1.0 - y1) + grid[i + 1, j + 1] * y0 * y1
    return out, outside


def heights(axis_n, axis_e, grid, pts):
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    return look_up(axis_n, axis_e, grid, pts[:, 0], pts[:, 1])[0]


def unit_rays(M, uv):
    """M [I, 3, 3], uv [n, 2] -> v [I, n, 3]: unit(M . [u, v, 1]), the products summed left to right"""
    M = np.asarray(M, np.float64).reshape(-1, 1, 9)
    u, w = uv[None, :, 0], uv[None, :, 1]
    q = np.stack([M[..., 3 * k] * u + M[..., 3 * k + 1] * w + M[..., 3 * k + 2] * 1.0 for k in range(3)], -1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return q / np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2])[..., None]


def rays(axis_n, axis_e, grid, ned, v, errors=None):
    """ned [I, 3], v [I, n, 3] -> pts [I, n, 3], iters uint8 [I, n], flags uint8 [I, n].  `errors`: a
    list that receives (ray mask, error) of the first look-up and of every round."""
    ned = np.asarray(ned, np.float64).reshape(-1, 3)
    I = ned.shape[0]
    v = np.asarray(v, np.float64).reshape(I, -1, 3)
    nn = np.broadcast_to(ned[:, None, :], v.shape).reshape(-1, 3)
    vv = v.reshape(-1, 3)
    R = vv.shape[0]
    p = nn.copy()
    count = np.zeros(R, np.int64)
    flags = np.zeros(R, np.uint8)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        sky = vv[:, 2] <= 0.0
        flags[sky] |= SKY
        tmp, out = look_up(axis_n, axis_e, grid, p[:, 0], p[:, 1])
        outside = out & ~sky
        ground = np.where(~np.isnan(tmp) & (tmp > FILL), tmp, 0.0)
        error = np.abs(p[:, 2] + ground)
        if errors is not None:
            errors.append((~sky, error.copy()))
        while True:
            go = ~sky & (error > 0.01) & (count < 25)
            if not go.any():
                break
            d_proj = -(nn[go, 2] + ground[go])
            factor = d_proj / vv[go, 2]
            p[go, 0] = nn[go, 0] + vv[go, 0] * factor
            p[go, 1] = nn[go, 1] + vv[go, 1] * factor
            p[go, 2] = nn[go, 2] + d_proj
            tmp, out = look_up(axis_n, axis_e, grid, p[go, 0], p[go, 1])
            outside[go] |= out
            keep = ~np.isnan(tmp) & (tmp > FILL)
            g = ground[go]
            g[keep] = tmp[keep]
            ground[go] = g
            error[go] = np.abs(p[go, 2] + ground[go])
            count[go] += 1
            if errors is not None:
                errors.append((go.copy(), error.copy()))
        flags[~sky & (count >= 25) & (error > 0.01)] |= CAPPED
        flags[outside] |= LEFT_GRID
    shape = v.shape[:2]
    return p.reshape(v.shape), count.astype(np.uint8).reshape(shape), flags.reshape(shape)
