"""imageanalysis_amd/ortho.py's TRUE-ORTHO RULES and imageanalysis_amd/dense.py's fill rule restated
in numpy, operation by operation (float64, no fused multiply-add: numpy's elementwise kernels round
every product and sum).  csrc/ortho_dsm.hip is held to these functions bit for bit.

A camera here is (K4, dist5, R, C) with K4 = (fx, fy, cx, cy) AT THE FRAME'S SIZE (scaled_K()); a
frame is uint8 [h][w][3].  Every image is computed over the whole mosaic unless boxes= limits it."""
import numpy as np

F32 = np.float32


def scaled_K(K, width, height, w, h):
    """dense.scaled_K: (fx, fy, cx, cy) of a width x height camera for its w x h frame, pixel centres kept"""
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.reshape(4)
    sx, sy = w / float(width), h / float(height)
    return np.array([fx * sx, fy * sy, (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5])


# ---- dense.py: fill ----
def fill(dsm, rounds=8):
    """-> (filled float32 [H, W], round_of uint8 [H, W])"""
    rounds = int(rounds)
    if not 0 <= rounds <= 254:
        raise ValueError("rounds is 0 to 254")
    z = np.array(dsm, F32)
    H, W = z.shape
    if not np.isfinite(z).any():
        raise ValueError("the DSM has no measured cell")
    round_of = np.where(np.isfinite(z), 0, 255).astype(np.uint8)
    for k in range(1, rounds + 1):
        P = np.full((H + 2, W + 2), np.nan, F32)
        P[1:-1, 1:-1] = z
        s = np.zeros((H, W), F32)
        n = np.zeros((H, W), np.int32)
        for dy in (0, 1, 2):                                # row-major over the 8 neighbours
            for dx in (0, 1, 2):
                if dy == 1 and dx == 1:
                    continue
                u = P[dy:dy + H, dx:dx + W]
                ok = np.isfinite(u)
                with np.errstate(invalid='ignore', over='ignore'):
                    s = np.where(ok, np.where(n > 0, s + u, u), s).astype(F32)
                n = n + ok
        hole = ~np.isfinite(z) & (n > 0)
        q = (s.astype(np.float64) / np.maximum(n, 1).astype(np.float64)).astype(F32)
        z = np.where(hole, q, z).astype(F32)
        round_of = np.where(hole, k, round_of).astype(np.uint8)
    return z, round_of


# ---- ortho.py: the true-ortho rules ----
def zmax_of(dsm):
    z = np.asarray(dsm, F32)
    return float(z[np.isfinite(z)].max())


def heights(dsm, ss):
    """the bilinear DSM height at every mosaic pixel's centre -> float64 [H ss][W ss], NaN: a hole"""
    Z = np.asarray(dsm, F32).astype(np.float64)
    H, W = Z.shape

    def taps(n, N):
        g = np.minimum(np.maximum((np.arange(n * ss, dtype=np.float64) + 0.5) / ss - 0.5, 0.0), float(N - 1))
        a = np.floor(g).astype(np.int64)
        return a, np.minimum(a + 1, N - 1), g - a

    xa, xb, tx = taps(W, W)
    ya, yb, ty = taps(H, H)

    def along_row(y):
        a, b = Z[y][:, xa], Z[y][:, xb]
        with np.errstate(invalid='ignore'):
            return np.where(tx == 0, a, a + (b - a) * tx)     # (the tap of weight zero is not read)

    top, bot = along_row(ya), along_row(yb)
    with np.errstate(invalid='ignore'):
        return np.where(ty[:, None] == 0, top, top + (bot - top) * ty[:, None])


def occluded(dsm, x0, y1, gsd, ss, bias, zmax, C, h, dh, where):
    """the visibility march of the pixels in `where` towards the camera at C (NED) -> bool [H ss][W ss]"""
    Z = np.asarray(dsm, F32).astype(np.float64)
    H, W = Z.shape
    rr, cc = np.nonzero(where)
    px, py = (cc + 0.5) / ss, (rr + 0.5) / ss
    qx, qy = (C[1] - x0) / gsd, (y1 - C[0]) / gsd
    dx, dy = qx - px, qy - py
    L = np.maximum(np.abs(dx), np.abs(dy))
    hh, dd = h[rr, cc], dh[rr, cc]
    out = np.zeros(np.shape(where), bool)
    alive = np.arange(len(rr))
    for i in range(1, max(H, W) + 1):
        alive = alive[i <= L[alive]]
        if len(alive) == 0:
            break
        t = i / L[alive]
        x, y = np.floor(px[alive] + dx[alive] * t), np.floor(py[alive] + dy[alive] * t)
        inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        hr = hh[alive] + dd[alive] * t
        go = inside & ~(hr > zmax)
        z = Z[np.where(go, y, 0).astype(np.int64), np.where(go, x, 0).astype(np.int64)]
        with np.errstate(invalid='ignore'):
            occ = go & (z > hr + bias)
        out[rr[alive[occ]], cc[alive[occ]]] = True
        alive = alive[go & ~occ]
    return out


def march(dsm, x0, y1, gsd, ss, bias, C, where=None):
    """the march alone, for a camera given by its centre: every mosaic pixel with a height and
    dh > 0 (and in `where`) -> (occluded bool [H ss][W ss], h)"""
    h = heights(dsm, ss)
    dh = (-C[2]) - h
    with np.errstate(invalid='ignore'):
        todo = ~np.isnan(h) & (dh > 0)
    if where is not None:
        todo &= where
    return occluded(dsm, x0, y1, gsd, ss, bias, zmax_of(dsm), C, h, dh, todo), h


def project(cam, n, e, h):
    """dense.py's warp from D = Xw - Cn onward at P = (n, e, -h) -> (D_0, D_1, Xn_2, fx_, fy_)"""
    K, dist, R, C = cam
    fx, fy, cx, cy = K
    k1, k2, p1, p2, k3 = dist
    dn, de, dd = n - C[0], e - C[1], (-h) - C[2]
    X = (R[0, 0] * dn + R[0, 1] * de) + R[0, 2] * dd
    Y = (R[1, 0] * dn + R[1, 1] * de) + R[1, 2] * dd
    Z = (R[2, 0] * dn + R[2, 1] * de) + R[2, 2] * dd
    with np.errstate(all='ignore'):
        x, y = X / Z, Y / Z
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        return dn, de, Z, fx * xd + cx, fy * yd + cy


def sample(frame, fu, fv):
    """ortho.py's bilinear formula at (fu, fv), both inside the frame -> float64 [n][3]"""
    T = np.asarray(frame).astype(np.float64)
    h_s, w_s = T.shape[:2]
    sx0, sy0 = np.floor(fu).astype(np.int64), np.floor(fv).astype(np.int64)
    sx1, sy1 = np.minimum(sx0 + 1, w_s - 1), np.minimum(sy0 + 1, h_s - 1)
    tx, ty = (fu - sx0)[:, None], (fv - sy0)[:, None]
    top = T[sy0, sx0] + (T[sy0, sx1] - T[sy0, sx0]) * tx
    bot = T[sy1, sx0] + (T[sy1, sx1] - T[sy1, sx0]) * tx
    return top + (bot - top) * ty


def compose(dsm, x0, y1, gsd, cams, frames, mode='best', ss=1, bias=None, boxes=None):
    """-> dict(acc, index, count, bgr, visible): acc float64 [Ho][Wo] (best: the winner's m, +inf
    where uncovered) or [Ho][Wo][4] (feather: sum w b, sum w g, sum w r, sum w), index int32 (best;
    None in mode feather), count uint16, bgr uint8 [Ho][Wo][3], visible: per image the bool mask of the
    pixels it covers and sees.  boxes: per image an inclusive (c0, r0, c1, r1) the work is limited to."""
    if mode not in ('best', 'feather'):
        raise ValueError("mode must be 'best' or 'feather' (multiband over a dense surface is not built)")
    if int(ss) != ss or not 1 <= ss <= 8:
        raise ValueError("upsample is an integer 1 .. 8")
    ss = int(ss)
    bias = 1.0 * gsd if bias is None else float(bias)
    if not (bias >= 0.0 and np.isfinite(bias)):
        raise ValueError("bias is a finite number of metres, at least 0")
    for f in frames:
        if np.ndim(f) != 3 or np.shape(f)[0] < 2 or np.shape(f)[1] < 2 or np.shape(f)[2] != 3:
            raise ValueError("a frame is [h][w][3], at least 2 x 2")
    Z32 = np.asarray(dsm, F32)
    H, W = Z32.shape
    Ho, Wo = H * ss, W * ss
    g = gsd / ss
    zmax = zmax_of(Z32)
    h = heights(Z32, ss)
    e = (x0 + (np.arange(Wo, dtype=np.float64) + 0.5) * g)[None, :]
    n = (y1 - (np.arange(Ho, dtype=np.float64) + 0.5) * g)[:, None]
    best = mode == 'best'
    acc = np.full((Ho, Wo), np.inf) if best else np.zeros((Ho, Wo, 4))
    index = -np.ones((Ho, Wo), np.int32) if best else None
    count = np.zeros((Ho, Wo), np.uint16)
    bgr = np.zeros((Ho, Wo, 3), np.uint8)
    seen = []
    for k, (cam, frame) in enumerate(zip(cams, frames)):
        h_s, w_s = np.shape(frame)[:2]
        C = cam[3]
        D0, D1, Zc, fu, fv = project(cam, n, e, h)
        dh = (-C[2]) - h
        with np.errstate(invalid='ignore'):
            cover = (~np.isnan(h) & (Zc > 0) & (fu >= 0) & (fu <= w_s - 1) & (fv >= 0) & (fv <= h_s - 1) & (dh > 0))
        if boxes is not None:
            c0, r0, c1, r1 = boxes[k]
            inbox = np.zeros((Ho, Wo), bool)
            if c1 >= c0 and r1 >= r0:
                inbox[r0:r1 + 1, c0:c1 + 1] = True
            cover &= inbox
        vis = cover & ~occluded(Z32, x0, y1, gsd, ss, bias, zmax, C, h, dh, cover)
        seen.append(vis)
        count[vis] = np.minimum(count[vis].astype(np.int64) + 1, 65535).astype(np.uint16)
        if best:
            with np.errstate(invalid='ignore', divide='ignore'):
                m = (D0 * D0 + D1 * D1) / (dh * dh)
                win = vis & (m < acc)
            acc[win] = m[win]
            index[win] = k
            val = sample(frame, fu[win], fv[win])
            bgr[win] = np.floor(val + 0.5).astype(np.uint8)
        else:
            fu_, fv_ = fu[vis], fv[vis]
            val = sample(frame, fu_, fv_)
            d = np.minimum(np.minimum(fu_, (w_s - 1) - fu_), np.minimum(fv_, (h_s - 1) - fv_))
            w = np.maximum(d / (0.5 * min(w_s - 1, h_s - 1)), 2.0 ** -20)
            a = acc[vis]
            a[:, :3] = a[:, :3] + w[:, None] * val
            a[:, 3] = a[:, 3] + w
            acc[vis] = a
    if not best:
        on = count > 0
        bgr[on] = np.floor(acc[on][:, :3] / acc[on][:, 3:4] + 0.5).astype(np.uint8)
    return dict(acc=acc, index=index, count=count, bgr=bgr, visible=seen)
