"""numpy restatement of the point undistortion the reference asks of OpenCV,

    cv2.undistortPoints(src, K, dist, P=K)          src float32 [n, 1, 2], dist = (k1, k2, p1, p2, k3)

written from OpenCV's published iteration with its default criteria (five rounds, no early exit).
This is what csrc/chain_geom.hip (iamx_undistort_points, undistort.undistort_points, and the member
loop of iamx_chain_triangulate) is held to BIT FOR BIT: float64 elementwise numpy, no BLAS, every
product and sum rounded on its own in the order written here.

Parity against cv2 itself is UNPINNED, as for CLAHE and the resizes (tests/area_restatement.py,
oracle/image_oracle.py headers): cv2 is not installed where the tests run, so nothing here was ever
compared with its output.

The convention, in float64:
  * x = (u - cx) / fx, y = (v - cy) / fy, x0 = x, y0 = y;
  * exactly five rounds of
        r2 = x*x + y*y
        icdist = 1 / (1 + ((k3*r2 + k2)*r2 + k1)*r2)
        dx = 2*p1*x*y + p2*(r2 + 2*x*x)
        dy = p1*(r2 + 2*y*y) + 2*p2*x*y
        x = (x0 - dx)*icdist,  y = (y0 - dy)*icdist
    a point whose icdist < 0 in any round falls back to x0, y0 and stops;
  * out = x*fx + cx, y*fy + cy, rounded to float32.
"""
import numpy as np


def undistort_points(uv, K, dist):
    """uv: [..., 2] (read as float32); K: 3x3 or (fx, fy, cx, cy); dist: (k1, k2, p1, p2, k3).
    -> float32 array of uv's shape."""
    uv = np.asarray(uv, np.float32)
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.ravel()[:4]
    k1, k2, p1, p2, k3 = [np.float64(v) for v in np.asarray(dist, np.float64).ravel()[:5]]
    u = uv[..., 0].astype(np.float64)
    v = uv[..., 1].astype(np.float64)
    x0 = (u - cx) / fx
    y0 = (v - cy) / fy
    x, y = x0.copy(), y0.copy()
    live = np.ones(x.shape, bool)
    with np.errstate(all='ignore'):
        for _ in range(5):
            r2 = x * x + y * y
            icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            neg = live & (icdist < 0)
            xn = (x0 - dx) * icdist
            yn = (y0 - dy) * icdist
            step = live & ~neg
            x = np.where(step, xn, np.where(neg, x0, x))
            y = np.where(step, yn, np.where(neg, y0, y))
            live = step
    out = np.empty(uv.shape, np.float32)
    out[..., 0] = (x * fx + cx).astype(np.float32)
    out[..., 1] = (y * fy + cy).astype(np.float32)
    return out


def cv2_undistortPoints(src, cameraMatrix, distCoeffs, R=None, P=None):
    """the call shape of cv2.undistortPoints for P = cameraMatrix (what the reference uses)"""
    if R is not None or P is None or not np.array_equal(np.asarray(P), np.asarray(cameraMatrix)):
        raise NotImplementedError("restated for R=None, P=K only")
    src = np.asarray(src, np.float32)
    return undistort_points(src.reshape(-1, 2), cameraMatrix, distCoeffs).reshape(-1, 1, 2)
