"""numpy restatement of the area downscale the texture step asks of OpenCV,

    cv2.resize(src, (0, 0), fx=fx, fy=fy, interpolation=cv2.INTER_AREA)        uint8, 1 or 3 channels

written from OpenCV's published area algorithm for uint8 with a float work type.  This is what
csrc/image_area.hip (iamx_image_resize_area, kernels.resize_area) is held to BIT FOR BIT.

Parity against cv2 itself is UNPINNED, as for CLAHE and the bilinear resize (oracle/image_oracle.py
header): cv2 is on neither the build machine nor the GPU machine, so nothing here was ever compared
with its output.  What is pinned is this restatement against the exact area average (never more
than one level apart, tests/test_textures.py) and the kernel against this restatement.

The convention:
  * size: dw = round-half-even(w * fx), dh likewise (area_dims);
  * per axis scale = 1.0 / f as a double -- not src/dst, the two can differ in the last bit;
  * destination index d, in double: fs1 = d*scale, fs2 = fs1 + scale, cell = min(scale, ssize - fs1),
    s1 = ceil(fs1), s2 = min(floor(fs2), ssize - 1), s1 = min(s1, s2); its taps in this order:
      - if s1 - fs1 > 1e-3: source s1-1, weight float32((s1 - fs1) / cell)
      - sources s1 .. s2-1,  weight float32(1 / cell)
      - if fs2 - s2 > 1e-3: source s2, weight float32(min(min(fs2 - s2, 1), cell) / cell)
  * for every source row that contributes to a destination row, in tap order:
    buf[dx, c] = sum_k src * alpha_k in float32, sequentially from 0, multiply and add rounded
    separately; the first row sets sum = beta*buf, later rows sum += beta*buf (rounded separately);
  * result = sum rounded half to even, saturated to 0..255;
  * both scales integers within DBL_EPSILON: the integer branch -- integer sum over the sx x sy
    block times float32(1/area), rounded half to even; (sum + 2) >> 2 for 2 x 2; a block that
    hangs over the right or bottom edge is float32(sum) / float32(count) over its samples inside.

Departures from cv2.resize, stated:
  * downscale only (1/fx >= 1 and 1/fy >= 1; cv2 switches to its bilinear-style area upscale
    otherwise) and scales up to 4096 per axis; anything else is an argument error;
  * the edge rule of the integer branch tests whole pixels (OpenCV compares an element offset with
    the pixel width for multi-channel images, which looks unintended);
  * OpenCV's SIMD paths are assumed to compute what its scalar code computes.
"""
import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)
MAX_SCALE = 4096.0


def area_dims(h, w, fx, fy):
    """(dh, dw) of cv2.resize(src, (0, 0), fx, fy)"""
    return int(np.rint(np.float64(h) * np.float64(fy))), int(np.rint(np.float64(w) * np.float64(fx)))


def area_taps(dsize, ssize, scale):
    """per destination index: (first source index [dsize], weights float32 [dsize, kmax] padded with
    zeros behind the last tap, tap counts [dsize])"""
    firsts, weights = [], []
    for d in range(dsize):
        fs1 = float(d) * scale
        fs2 = fs1 + scale
        cell = min(scale, ssize - fs1)
        s1 = int(np.ceil(fs1))
        s2 = min(int(np.floor(fs2)), ssize - 1)
        s1 = min(s1, s2)
        wts = []
        first = s1
        if s1 - fs1 > 1e-3:
            first = s1 - 1
            wts.append(np.float32((s1 - fs1) / cell))
        wts.extend([np.float32(1.0 / cell)] * (s2 - s1))
        if fs2 - s2 > 1e-3:
            wts.append(np.float32(min(min(fs2 - s2, 1.0), cell) / cell))
        firsts.append(first)
        weights.append(wts)
    kmax = max(len(x) for x in weights)
    wt = np.zeros((dsize, kmax), np.float32)
    for d, x in enumerate(weights):
        wt[d, :len(x)] = x
    return np.asarray(firsts, np.int64), wt, np.asarray([len(x) for x in weights], np.int64)


def _integer_branch(src, dh, dw, sx, sy):
    h, w, ch = src.shape
    # block sums, with zeros (and a sample count) over the right / bottom edge
    ph, pw = dh * sy, dw * sx
    pad = np.zeros((max(ph, h), max(pw, w), ch), np.int64)
    pad[:h, :w] = src
    inside = np.zeros((max(ph, h), max(pw, w)), np.int64)
    inside[:h, :w] = 1
    total = pad[:ph, :pw].reshape(dh, sy, dw, sx, ch).sum(axis=(1, 3))
    count = inside[:ph, :pw].reshape(dh, sy, dw, sx).sum(axis=(1, 3))[:, :, None]
    full = count == sx * sy
    if sx == 2 and sy == 2:
        whole = (total + 2) >> 2
    else:
        inv = np.float32(1.0) / np.float32(sx * sy)
        whole = np.rint(total.astype(np.float32) * inv)
    edge = np.rint(total.astype(np.float32) / np.maximum(count, 1).astype(np.float32))
    out = np.where(full, whole, edge)
    return np.clip(out, 0, 255).astype(np.uint8)


def resize_area(src, fx, fy):
    """uint8 [h, w] or [h, w, 3] -> uint8 [dh, dw(, 3)]"""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim not in (2, 3):
        raise ValueError("uint8 [h, w] or [h, w, c] expected")
    grey = src.ndim == 2
    img = src[:, :, None] if grey else src
    h, w, ch = img.shape
    if ch not in (1, 3):
        raise ValueError("1 or 3 channels")
    scale_x, scale_y = 1.0 / float(fx), 1.0 / float(fy)
    if not (1.0 <= scale_x <= MAX_SCALE and 1.0 <= scale_y <= MAX_SCALE):
        raise ValueError("area downscale only (1 <= 1/f <= 4096)")
    dh, dw = area_dims(h, w, fx, fy)
    isx, isy = int(np.rint(scale_x)), int(np.rint(scale_y))
    if abs(scale_x - isx) < DBL_EPSILON and abs(scale_y - isy) < DBL_EPSILON:
        out = _integer_branch(img, dh, dw, isx, isy)
        return out[:, :, 0] if grey else out
    xf, xw, _xn = area_taps(dw, w, scale_x)
    yf, yw, _yn = area_taps(dh, h, scale_y)
    # along x, every source row at once: taps in order from 0 (a zero weight behind a pixel's
    # last tap adds +0.0, which changes nothing)
    buf = np.zeros((h, dw, ch), np.float32)
    for k in range(xw.shape[1]):
        idx = np.minimum(xf + k, w - 1)
        buf = buf + img[:, idx, :].astype(np.float32) * xw[None, :, k, None]
    # along y, rows in tap order; 0 + beta*buf == beta*buf, the first row's assignment
    acc = np.zeros((dh, dw, ch), np.float32)
    for k in range(yw.shape[1]):
        idx = np.minimum(yf + k, h - 1)
        acc = acc + yw[:, k, None, None] * buf[idx]
    out = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    return out[:, :, 0] if grey else out


def exact_area_average(src, dh, dw):
    """the exact area average as float64 [dh, dw(, c)]: destination cell d covers the source
    interval [d*ssize/dsize, (d+1)*ssize/dsize); overlaps are rational (integers over dsize)"""
    src = np.asarray(src)
    grey = src.ndim == 2
    img = (src[:, :, None] if grey else src).astype(np.float64)

    def overlap(ssize, dsize):
        m = np.zeros((dsize, ssize), np.float64)
        for d in range(dsize):
            lo, hi = d * ssize, (d + 1) * ssize              # in units of 1/dsize
            for s in range(lo // dsize, min(ssize, -(-hi // dsize))):
                ov = min(hi, (s + 1) * dsize) - max(lo, s * dsize)
                if ov > 0:
                    m[d, s] = ov / float(ssize)
        return m
    my, mx = overlap(img.shape[0], dh), overlap(img.shape[1], dw)
    out = np.einsum('ds,swc->dwc', my, img)
    out = np.einsum('dwc,xw->dxc', out, mx)
    return out[:, :, 0] if grey else out
