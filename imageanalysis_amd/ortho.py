"""Orthomosaic raster of the Step 5 map: what the reference shows only in explorer.py's Panda3D
window (every image's surface grid drawn top-down, no depth test, ordered by distance from the view
centre) written as one georeferenced image, on a machine without a display.

    raster_frame(grids, gsd)                       origin, size, snapped vertices (host)
    compose(grids, uvs, frames, width, height, gsd, mode, bands=)   the rasteriser on ready arrays
    render(proj, group_list, group_index, gsd, ...)           grids, frames and filters of a project
    save(mosaic, analysis_dir, tile, fmt, subdir)  tiles, world files, ortho.json
    compose_dense(...), render_dense(...)          the true orthophoto over the dense DSM (last section)

The rasteriser is csrc/ortho_raster.hip; tests/ortho_restatement.py (mode multiband:
tests/ortho_multiband_restatement.py) restates the rules below in numpy, operation by operation,
and the device result is held to it byte for byte.

THE RULES

Inputs per image of the group: grid_list, ENU vertices [(S+1)^2][3], NaN allowed; distorted_uv,
source pixels [(S+1)^2][2] in the camera's width x height; a BGR uint8 frame of any size
h_s x w_s, source coordinates scaled by w_s / width and h_s / height.

Polygons: the .egg file's.  Cell (j, i) has c = j (S+1) + i and d = c + S + 1; it is USED only if
c, c+1, d, d+1 are all finite (x, y and z).  A used cell is two triangles, (d, d+1, c+1) then
(d, c+1, c), cells in file order (j outer, i inner).  The split of the quad is this package's
convention: Panda3D's own triangulation of a four-vertex polygon is unpinned.  A used vertex is a
vertex of a used cell.

Raster frame (host, float64), over the used vertices of all images:
    x0 = floor(min x / gsd) gsd         y1 = ceil(max y / gsd) gsd
    W = ceil((max x - x0) / gsd)        H = ceil((y1 - min y) / gsd)        (at least 1)
Row 0 is north; pixel (r, c) has its centre at east x0 + (c + 0.5) gsd, north y1 - (r + 0.5) gsd.
A side above 2^20 pixels is refused; a mosaic whose accumulators do not fit the free device
memory is refused with its size in the message (no band splitting).

Coverage is exact.  The host snaps vertices to 1/256 pixel, X = rint((x - x0) / gsd * 256),
Y = rint((y1 - y) / gsd * 256), int32.  The device evaluates int64 edge functions at the pixel
centres (256 c + 128, 256 r + 128).  With area2 = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) for the
triangle (a, b, c): area2 == 0 is skipped, area2 < 0 swaps b and c.  The edge opposite vertex k
(b -> c, c -> a, a -> b) from (Xs, Ys) with (ex, ey) = end - start has the value
    w_k = ex (py - Ys) - ey (px - Xs)
and a centre is inside when every w_k > 0, or w_k == 0 on a top-left edge (ey < 0, or ey == 0 and
ex > 0).  Within one image the first triangle in file order that covers a pixel owns it (this
settles folded cells).  The rule is watertight and never covers a pixel twice.

Texture coordinate and sample (float64, every product and sum rounded on its own), with w_k
converted to double and (u_k, v_k) the distorted_uv of vertex k after the swap:
    u = ((w0 u0 + w1 u1) + w2 u2) / ((w0 + w1) + w2)              v likewise
    fu = min(max(u (w_s / width) - 0.5, 0), w_s - 1)              fv from v, h_s / height, h_s - 1
    x0 = floor(fu), x1 = min(x0 + 1, w_s - 1), tx = fu - x0       y likewise
    top = T[y0][x0] + (T[y0][x1] - T[y0][x0]) tx                  bot on row y1
    sample = top + (bot - top) ty                                 per channel
(the clamp is the explorer's WM_clamp).

Composition, images in group order:
  best      the static form of the explorer's "best" ordering.  Per image, from the tight bounds
            lo, hi of its used vertices (x, y, z): centre = (lo + hi) 0.5, span = |hi - lo|,
            metric(p) = sqrt((cx - px)^2 + (cy - py)^2) + span 0.1 at the pixel's centre p.  The
            covering image with the smallest metric wins, the earlier image on a tie.
            bgr = floor(sample + 0.5); index (int32, -1 where uncovered); count (uint16, the
            covering images, saturating).
  feather   d = min(u, width - u, v, height - v) at the interpolated source coordinate,
            w = max(d / (0.5 min(width, height)), 2^-20), colour = sum w sample / sum w in
            float64, accumulated in group order, bgr = floor(colour + 0.5); count as above.
  multiband Burt-Adelson blending along best's seams (tests/ortho_multiband_restatement.py restates
            it).  Everything above is reused as it is; what follows is float32, every product and
            sum rounded on its own, the one division done in float64 and rounded once (that is the
            correctly rounded float32 quotient, whatever a device does with denormals).
    bands   B, 1 .. 16 (default 5; anything else is a ValueError before any device call).  Level
            sizes H_0 = H, H_(l+1) = (H_l + 1) // 2, W likewise; the levels used are
            L = min(B, 1 + ceil(log2(max(H, W)))): a 1 x 1 mosaic has one.
    owner   before any frame is needed, mode best's index and count for the whole group (geometry
            only): byte for byte what mode best produces.
    layer   of image k, over the mosaic: C_k(p) = the sample above, all three channels, cast to
            float32, wherever image k COVERS p (not only where it wins), 0 elsewhere and outside the
            mosaic; A_k(p) = 1 where index(p) == k, else 0.
    reduce  R, separable, ALONG x FIRST (every row), THEN ALONG y: taps g = (1, 4, 6, 4, 1) / 16 at
            the source positions 2j - 2 .. 2j + 2, outside the level 0, the five terms summed from
            the left:  (((g0 x[2j-2] + g1 x[2j-1]) + g2 x[2j]) + g1 x[2j+1]) + g0 x[2j+2].
    expand  E, to the finer level's size, along x first, then along y; outside is 0:
            even 2m:     ((X[m-1] + 6 X[m]) + X[m+1]) 0.125        odd 2m+1:   (X[m] + X[m+1]) 0.5
    pyramids per image:  GC^0 = C_k, GC^(l+1) = R(GC^l);  GA^0 = A_k, GA^(l+1) = R(GA^l);
            LP^l = GC^l - E(GC^(l+1)) for l < L - 1, LP^(L-1) = GC^(L-1).
    accumulate, images in group order, stream ordered, no atomics:
            N^l = N^l + GA^l LP^l per channel,  D^l = D^l + GA^l.
    resolve Q^l = N^l / D^l where D^l > 0, else 0;  M^(L-1) = Q^(L-1),  M^l = Q^l + E(M^(l+1));
            bgr = floor(min(max(M^0, 0), 255) + 0.5) where count > 0, else 0.
            The Mosaic carries bgr, index, count, mode 'multiband' and bands = L.
    extents the device works, per image, on the region of each level where GA^l or GC^l can be
            non-zero: the pixel box at level 0, and lo .. hi of level l becomes
            ceil((lo - 2) / 2) .. floor((hi + 2) / 2), cut to the level, at level l + 1
            (level_regions()).  Outside it GA^l is 0 and N^l, D^l would receive +-0: no bit changes.
            The restatement computes every level over the whole mosaic; equality checks the extents.
Uncovered pixels are 0.

Memory: best holds 8 + 4 + 2 + 3 = 17 bytes per pixel, feather 32 + 2 + 3 = 37; one image is one
launch that reads and writes only the pixels it covers, plus the frame.  multiband
(multiband_bytes()): 16 bytes per accumulator pixel of every level (at most 16 * 4 / 3 per mosaic
pixel), index 4, count 2, bgr 3; on top the larger of the ownership metric (8 per mosaic pixel,
freed before the first frame) and the layer pyramid of the image with the largest pixel box (16 per
pixel of its regions).  The collapse works in place.  An image costs a layer launch, L - 1 reduces
and L accumulates over its regions; the collapse runs once over every level.

THE TRUE-ORTHO RULES

    compose_dense(surface, cameras, frames, mode, upsample, bias, bands=)   the drape on ready arrays
    render_dense(proj, group_list, group_index, surface, ...)       poses, frames and filters of a project

A true orthophoto over the dense DSM (dense.py; 5e-true-ortho.py): every mosaic pixel is placed at
its DSM height, projected into the frames through the full camera model and coloured only from the
frames that see it.  The kernel is csrc/ortho_dsm.hip; tests/ortho_dense_restatement.py restates
what follows and the device is held to it bit for bit.  Everything is float64, every product and sum
rounded on its own, sums of three from the left.

Inputs.  The surface: Z = float64(dsm) [H][W] with x0, y1, gsd (dense.Surface; fill it first, a NaN
cell is a hole).  The settings: an integer upsample ss, 1 .. 8; bias >= 0, finite, metres; zmax, the
largest finite Z.  Per image k: a BGR uint8 frame h_k x w_k, at least 2 x 2;
K_k = dense.scaled_K(K, width, height, w_k, h_k); dist[5]; R (NED -> camera); C (NED).

Mosaic.  H_o = H ss, W_o = W ss, g = gsd / ss (a side above 2^20 pixels is refused).  Row 0 is north;
pixel (r, c) lies at e = x0 + (c + 0.5) g, n = y1 - (r + 0.5) g.

Height.  gx = min(max((c + 0.5) / ss - 0.5, 0), W - 1), xa = floor(gx), xb = min(xa + 1, W - 1),
tx = gx - xa; y likewise.  top = Z[ya][xa] + (Z[ya][xb] - Z[ya][xa]) tx, and Z[ya][xa] alone when
tx == 0 (the tap of weight zero is not read: a hole beside the pixel does not reach it); bot on row
yb; h = top + (bot - top) ty, and top alone when ty == 0.  Where h is NaN the pixel is uncovered for
every image.  P = (n, e, -h).

Cover.  dense.py's warp from D = Xw - Cn onward with Xw = P: Xn, x, y, r2, rad, xd, yd, then fx_, fy_
with K_k.  Image k covers the pixel iff Xn_2 > 0, 0 <= fx_ <= w_k - 1, 0 <= fy_ <= h_k - 1 (a NaN
fails) and dh = (-C_2) - h > 0.

Visibility, in DSM cell units: px = (c + 0.5) / ss, py = (r + 0.5) / ss; qx = (C_1 - x0) / gsd,
qy = (y1 - C_0) / gsd; dx = qx - px, dy = qy - py, L = max(|dx|, |dy|).  For i = 1, 2, ... while
i <= L and i <= max(H, W):
    t = i / L,  x = px + dx t,  y = py + dy t
    the cell is (floor(y), floor(x)); outside the raster: visible, stop
    hr = h + dh t;  hr > zmax: visible, stop
    Z[cell] > hr + bias: occluded, stop                      (false for a NaN)
When the loop runs out, or L < 1, the pixel is visible.  A step moves one cell along the longer
axis, so the bound max(H, W) is never what ends a march.

Sample: the bilinear formula above at (fx_, fy_) in the frame, per channel.

Composition, images in group order, one stream-ordered launch per image, no atomics; the
accumulators are those of best and feather above (iamx_ortho_clear and iamx_ortho_resolve are reused):
  best      m = (D_0 D_0 + D_1 D_1) / (dh dh), the squared tangent off nadir; the smallest m wins,
            the earlier image on a tie.  bgr = floor(sample + 0.5); index int32, -1 where
            uncovered; count uint16, the images that cover AND see the pixel, saturating.
  feather   d = min(min(fx_, (w_k - 1) - fx_), min(fy_, (h_k - 1) - fy_)),
            w = max(d / (0.5 min(w_k - 1, h_k - 1)), 2^-20); accumulated and resolved as feather above.
  multiband mode='multiband' stays a ValueError over a dense surface; the blend is asked for with
            bands=B, 1 .. 16, beside mode='best' (bands=0, the default, is mode best as above; a
            non-integer, a value outside 0 .. 16 or bands > 0 with mode feather is a ValueError before
            any device call).  It is mode multiband above along mode best's seams HERE, with the two
            passes that its pyramid kernels want from csrc/ortho_dsm.hip
            (tests/ortho_dense_multiband_restatement.py restates it).  Everything not said here is
            the rules of this section (height, cover, visibility, sample, work box) and mode
            multiband's (bands, reduce, expand, pyramids, accumulate, resolve, extents), as written.
    owner   before any layer: index and count of compose_dense(mode='best') on the same surface,
            cameras and frame sizes, byte for byte.  It is geometry only: it needs each frame's
            (h_k, w_k), and through them K_k, but no pixels.  The metric plane (8 bytes per mosaic
            pixel) is freed before the first layer, as in the sparse mode.
    layer   of image k, over its work box: C_k(p) = the bilinear sample in float64, cast to float32,
            wherever image k COVERS p, whether it sees p or not, 0 elsewhere; A_k(p) = 1 where
            index(p) == k, else 0.  Four floats (C_b, C_g, C_r, A) per pixel in the layout
            iamx_ortho_mb_layer writes.  Every pixel of the box is written: the layer buffer is
            reused between images and is not cleared.
            Why covered and not seen: the owner already keeps an occluded view from colouring a pixel
            at full resolution, and what the coarse bands of a neighbour bring across a seam is
            low-frequency colour.  With a zero inside the occlusion shadow the result leaves the range
            of the inputs.  A numpy prototype (the roof scene of tests/test_ortho_dense.py at 96 x 96,
            its first three cameras, flat 400 x 400 frames of 100, 200 and 150 at focal 150 so that
            every camera covers the whole mosaic, bias 0.5) gave blended pixels of 86 .. 222 at 3 bands
            and 98 .. 225 at 5 with a layer of the visible pixels only, and 100 .. 200 at 1, 3, 5 and 8
            bands with the rule above: under it every level of every image is its colour times the
            same border term, so the blend is a convex combination.  On the same scene at 5 bands,
            inside a margin of 8 pixels, the largest step between neighbouring pixels was 5 where mode
            best has 100 (the largest overall, 59, sits in a corner of the mosaic: the zero padding,
            as in the sparse mode), and a single image came out within one grey level of mode best.
    pyramids, accumulate, resolve, extents: the sparse mode's, with the work box in place of the
            pixel box: level_regions(box, sizes).  bgr is 0 where count == 0.  The Mosaic carries
            mode 'multiband', bands = L, surface 'dense', upsample, bias, index and count.

Work box per image (host, float64; work_box()): the undistorted rays (undistort.undistort_points) of
the frame's four corners and of every 32nd border pixel are cut with the horizontal planes at the
smallest and the largest finite DSM height.  If a ray does not descend (or the camera is not above
the higher plane, or a hit is not finite) the box is the whole mosaic.  Otherwise it is the bounds
of the hits in mosaic pixels, floor of the smallest and ceil of the largest, grown on every side by
BOX_MARGIN = 2 pixels plus BOX_GROW = 1/64 of the box's longer side (the bow of a distorted border
between two samples, the float32 of the undistortion and the rounding of h), then cut to the mosaic.
It assumes a distortion model that is monotonic over the frame's cone.  The restatement computes
every image over the whole mosaic; equality checks the box.

Departures, none of them measured on real frames.  Whether the blend's covered-not-seen layer shows
as ghosting on real frames (an occluded view's colour of the roof, where the ground is owned by
another, enters the coarse bands beside the seam) has not been measured.  Occluders are the DSM's cells at their nearest-cell
heights while the point's own height is bilinear: on a slope steeper than bias / gsd per cell a
point can be hidden by the cell it stands in or the next one, which is what bias is for.  bias=None
means 1.0 gsd; no real DSM has been measured against that default.  Memory: the mosaic's
accumulators as above (17 or 37 bytes per pixel; with bands, multiband_bytes(sizes, work boxes)) plus
the DSM.
"""
import ctypes
import json
import os
import time
from math import ceil, floor, sqrt

import numpy as np

from . import _deps
from ._deps import getNode

# a mode's number in iamx_ortho_clear / iamx_ortho_raster_image; multiband has none: it has entry
# points of its own (iamx_ortho_mb_*) and is never forwarded to those two
MODES = {'best': 0, 'feather': 1, 'multiband': None}
MAX_SIDE = 1 << 20
SNAP = 256
# multiband: the pyramid accumulators' upper bound 16 * 4 / 3, index, count, bgr (multiband_bytes() is exact)
BYTES_PER_PIXEL = {'best': 8 + 4 + 2 + 3, 'feather': 32 + 2 + 3, 'multiband': 22 + 4 + 2 + 3}
MAX_BANDS = 16
PREFILTER_BELOW = 0.75         # the frame is shrunk when native / gsd is below this
WORLD_EXT = {'jpg': 'jgw', 'jpeg': 'jgw', 'png': 'pgw', 'tif': 'tfw', 'tiff': 'tfw', 'bmp': 'bpw'}

# the last render(): images, frames rasterised / shrunk, seconds per stage
render_stats = {'images': 0, 'prefiltered': 0, 'seconds': 0.0, 'frames_per_s': 0.0}


def _log(*a):
    _deps.logger().log(*a)


class RasterFrame(object):
    """x0, y1 (metres), W, H (pixels), S, and per image X, Y int32 [N][(S+1)^2] (0 where the vertex
    is not used) and used uint8 [N][S^2]"""
    __slots__ = ('x0', 'y1', 'gsd', 'W', 'H', 'S', 'X', 'Y', 'used')

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class Mosaic(object):
    """device bgr uint8 [H,W,3], index int32 [H,W] (None in mode feather), count uint16 [H,W];
    x0, y1, gsd; mode; names (the group's images, `index` counts into them); bands (multiband: the
    levels used, L; else None); a true orthophoto also carries surface = 'dense', upsample and bias
    (None on every other mosaic)"""
    __slots__ = ('bgr', 'index', 'count', 'x0', 'y1', 'gsd', 'mode', 'names', 'bands', 'surface', 'upsample', 'bias')

    def __init__(self, **kw):
        self.bands = None
        self.surface = self.upsample = self.bias = None
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def shape(self):
        return int(self.bgr.shape[0]), int(self.bgr.shape[1])


def _grids(grids):
    g = np.asarray(grids, np.float64)
    if g.ndim != 3 or g.shape[2] != 3 or g.shape[0] < 1:
        raise ValueError("grids must be [images][(S+1)^2][3]")
    side = int(round(sqrt(g.shape[1])))
    if side * side != g.shape[1] or side < 2:
        raise ValueError("a grid must hold (S+1)^2 vertices, S >= 1 (got %d)" % g.shape[1])
    return g, side - 1


def used_cells(grids):
    """-> (used cells bool [N][S][S], used vertices bool [N][S+1][S+1])"""
    g, S = _grids(grids)
    fin = np.isfinite(g).all(axis=2).reshape(-1, S + 1, S + 1)
    cells = fin[:, :-1, :-1] & fin[:, :-1, 1:] & fin[:, 1:, :-1] & fin[:, 1:, 1:]
    verts = np.zeros_like(fin)
    verts[:, :-1, :-1] |= cells
    verts[:, :-1, 1:] |= cells
    verts[:, 1:, :-1] |= cells
    verts[:, 1:, 1:] |= cells
    return cells, verts


def raster_frame(grids, gsd):
    """The raster frame and the snapped vertices of a group's grids (host, float64)."""
    g, S = _grids(grids)
    gsd = float(gsd)
    if not (gsd > 0.0 and np.isfinite(gsd)):
        raise ValueError("gsd must be a positive number of metres per pixel")
    cells, verts = used_cells(g)
    vm = verts.reshape(len(g), -1)
    if not vm.any():
        raise ValueError("no image of the group has a cell fully on the surface: nothing to rasterise")
    x, y = g[:, :, 0], g[:, :, 1]
    min_x, max_x = float(x[vm].min()), float(x[vm].max())
    min_y, max_y = float(y[vm].min()), float(y[vm].max())
    x0 = floor(min_x / gsd) * gsd
    y1 = ceil(max_y / gsd) * gsd
    W = max(1, int(ceil((max_x - x0) / gsd)))
    H = max(1, int(ceil((y1 - min_y) / gsd)))
    if W > MAX_SIDE or H > MAX_SIDE:
        raise ValueError("a %d x %d pixel raster: a side above 2^20 pixels is refused (gsd %g m)" % (W, H, gsd))
    with np.errstate(invalid='ignore'):
        X = np.where(vm, np.rint((x - x0) / gsd * SNAP), 0.0).astype(np.int32)
        Y = np.where(vm, np.rint((y1 - y) / gsd * SNAP), 0.0).astype(np.int32)
    return RasterFrame(x0=x0, y1=y1, gsd=gsd, W=W, H=H, S=S, X=X, Y=Y,
                       used=np.ascontiguousarray(cells.reshape(len(g), -1), np.uint8))


def image_terms(grid, verts):
    """best: (cx, cy, 0.1 span) from the tight bounds of the image's used vertices; None without one"""
    p = np.asarray(grid, np.float64).reshape(-1, 3)[np.asarray(verts, bool).reshape(-1)]
    if len(p) == 0:
        return None
    lo, hi = p.min(axis=0), p.max(axis=0)
    centre = (lo + hi) * 0.5
    vol = hi - lo
    span = sqrt(vol[0] * vol[0] + vol[1] * vol[1] + vol[2] * vol[2])
    return float(centre[0]), float(centre[1]), span * 0.1


def pixel_box(X, Y, verts, W, H):
    """the inclusive box (c0, r0, c1, r1) of the pixels whose centre can lie in the image's used
    vertices' box, cut to the raster; c1 < c0 when there is none"""
    m = np.asarray(verts, bool).reshape(-1)
    if not m.any():
        return 0, 0, -1, -1
    xs, ys = X[m].astype(np.int64), Y[m].astype(np.int64)
    # centres 256 c + 128 in [min, max]
    c0, c1 = -((128 - int(xs.min())) // SNAP), (int(xs.max()) - 128) // SNAP
    r0, r1 = -((128 - int(ys.min())) // SNAP), (int(ys.max()) - 128) // SNAP
    return max(c0, 0), max(r0, 0), min(c1, W - 1), min(r1, H - 1)


def band_levels(H, W, bands=5):
    """multiband: [(H_l, W_l)] of the L = min(bands, 1 + ceil(log2(max(H, W)))) levels used"""
    bands = int(bands)
    if not 1 <= bands <= MAX_BANDS:
        raise ValueError("bands must be 1 .. %d (got %d)" % (MAX_BANDS, bands))
    L = min(bands, 1 + (max(int(H), int(W)) - 1).bit_length())
    sizes = [(int(H), int(W))]
    while len(sizes) < L:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return sizes


def level_regions(box, sizes):
    """multiband: per level the inclusive region (y0, x0, y1, x1) where an image's layer can be
    non-zero, from its pixel box (c0, r0, c1, r1) of level 0.  Reduced pixel j reads 2j - 2 .. 2j + 2,
    so lo .. hi becomes ceil((lo - 2) / 2) .. floor((hi + 2) / 2), cut to the level."""
    c0, r0, c1, r1 = box
    out = [(r0, c0, r1, c1)]
    for h, w in sizes[1:]:
        y0, x0, y1, x1 = out[-1]
        out.append((max((y0 - 1) // 2, 0), max((x0 - 1) // 2, 0), min((y1 + 2) // 2, h - 1), min((x1 + 2) // 2, w - 1)))
    return out


def _area(region):
    return (region[2] - region[0] + 1) * (region[3] - region[1] + 1)


def multiband_bytes(sizes, boxes):
    """multiband's device memory: (what stays: 16 B per accumulator pixel of every level, index 4,
    count 2, bgr 3 per mosaic pixel; the ownership metric, 8 per mosaic pixel, freed before the first
    frame; the largest image's layer pyramid, 16 B per pixel of its regions).  The peak is the first
    plus the larger of the other two."""
    H, W = sizes[0]
    stay = 16 * sum(h * w for h, w in sizes) + (4 + 2 + 3) * H * W
    temp = 16 * max([sum(_area(r) for r in level_regions(b, sizes)) for b in boxes if b[2] >= b[0] and b[3] >= b[1]]
                    or [0])
    return stay, 8 * H * W, temp


def native_gsd(grid, cells, frame_w, frame_h):
    """sqrt(footprint area of the used cells / (frame_w frame_h)): the metres one frame pixel spans"""
    g = np.asarray(grid, np.float64)
    S = int(round(sqrt(len(g)))) - 1
    p = g[:, :2].reshape(S + 1, S + 1, 2)
    c, c1, d, d1 = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]

    def area(a, b, e):
        return 0.5 * np.abs((b[..., 0] - a[..., 0]) * (e[..., 1] - a[..., 1])
                            - (b[..., 1] - a[..., 1]) * (e[..., 0] - a[..., 0]))
    with np.errstate(invalid='ignore'):
        cell_area = area(d, d1, c1) + area(d, c1, c)
    total = float(cell_area[np.asarray(cells, bool).reshape(S, S)].sum())
    return sqrt(total / (float(frame_w) * float(frame_h)))


def prefilter_factor(grid, cells, frame_w, frame_h, gsd):
    """f = min(1, native / gsd); the frame is shrunk by f in both directions when f < 0.75"""
    return min(1.0, native_gsd(grid, cells, frame_w, frame_h) / float(gsd))


def _check_frame(frame):
    import torch
    if not (isinstance(frame, torch.Tensor) and frame.is_cuda and frame.dtype == torch.uint8
            and frame.dim() == 3 and frame.shape[2] == 3 and frame.numel() > 0):
        raise ValueError("a frame must be a device uint8 tensor [h, w, 3]")
    return frame.contiguous()


class _Pyramids(object):
    """mode multiband's level accumulators and the steps every multiband composer shares: the layer
    pyramid of one image into the accumulators, the collapse.  A composer provides sizes, index, count,
    bgr, dev, mode, _p and _call = (lib, check, stream_ptr), and writes the level-0 layer itself."""

    def _mb_alloc(self, torch, temp_bytes):
        """the accumulators of every level, zeroed, and the layer pyramid's buffer"""
        self.bands = len(self.sizes)
        self.offsets = np.concatenate([[0], np.cumsum([h * w for h, w in self.sizes])]).astype(np.int64)
        self.acc = torch.zeros((int(self.offsets[-1]), 4), dtype=torch.float32, device=self.dev)
        self.temp = torch.empty((max(temp_bytes // 16, 1), 4), dtype=torch.float32, device=self.dev)
        self.finished = False

    def _level(self, l):
        return self.acc[int(self.offsets[l]):int(self.offsets[l + 1])]

    def accumulators(self):
        """multiband, before finish(): per level (N float32 [H_l][W_l][3], D float32 [H_l][W_l]), views"""
        if self.mode != 'multiband' or self.finished:
            raise RuntimeError("accumulators(): mode multiband only, and before finish() (the collapse works in place)")
        out = []
        for l, (h, w) in enumerate(self.sizes):
            a = self._level(l).view(h, w, 4)
            out.append((a[:, :, :3], a[:, :, 3]))
        return out

    def _mb_layers(self, box):
        """(per-level regions, per-level layer buffers) of an image with the level-0 box (c0, r0, c1, r1)"""
        regions = level_regions(box, self.sizes)
        at = np.concatenate([[0], np.cumsum([_area(r) for r in regions])])
        return regions, [self.temp[int(at[l]):int(at[l + 1])] for l in range(len(regions))]

    def _mb_reduce(self, plan):
        """kernel (b): the layer's Gaussian pyramid"""
        L, check, stream_ptr = self._call
        p = self._p
        regions, layers = plan[-2:]
        st = stream_ptr()
        for l in range(len(regions) - 1):
            h, w = self.sizes[l]
            check(L.iamx_ortho_mb_reduce(h, w, p(layers[l]), *regions[l], p(layers[l + 1]), *regions[l + 1], st),
                  'iamx_ortho_mb_reduce')

    def _mb_accumulate(self, plan):
        """kernel (c): every level of the pyramid into the accumulators"""
        L, check, stream_ptr = self._call
        p = self._p
        regions, layers = plan[-2:]
        st = stream_ptr()
        top = len(regions) - 1
        for l in range(top + 1):
            h, w = self.sizes[l]
            coarse, cr = (p(layers[l + 1]), regions[l + 1]) if l < top else (None, (0, 0, 0, 0))
            check(L.iamx_ortho_mb_accumulate(h, w, p(layers[l]), *regions[l], coarse, *cr, p(self._level(l)), st),
                  'iamx_ortho_mb_accumulate')

    def _mb_pyramid(self, plan):
        """kernels (b) and (c): the layer's Gaussian pyramid, then every level into the accumulators"""
        self._mb_reduce(plan)
        self._mb_accumulate(plan)

    def _mb_collapse(self):
        """kernel (d), from the top level down; level 0 ends in bgr"""
        L, check, stream_ptr = self._call
        p = self._p
        top = len(self.sizes) - 1
        for l in range(top, -1, -1):
            h, w = self.sizes[l]
            up = p(self._level(l + 1)) if l < top else None
            count, bgr = (p(self.count), p(self.bgr)) if l == 0 else (None, None)
            check(L.iamx_ortho_mb_collapse(h, w, p(self._level(l)), up, count, bgr, stream_ptr()),
                  'iamx_ortho_mb_collapse')

    def _mb_finish(self):
        if self.finished:
            raise RuntimeError("finish() was called before: the collapse works in place")
        self.finished = True
        self._mb_collapse()
        self.temp = None


class _Composer(_Pyramids):
    """the accumulators of one mosaic and the group's tables on the device; add(k, frame) rasterises
    image k (call it in group order), finish() -> Mosaic"""

    def __init__(self, grids, uvs, width, height, gsd, mode, names=None, bands=5):
        import torch
        from . import kernels
        from ._lib import check, lib, require_gpu, stream_ptr
        if mode not in MODES:
            raise ValueError("mode must be 'best', 'feather' or 'multiband'")
        if mode == 'multiband':
            band_levels(1, 1, bands)                       # (a ValueError before any device call)
        g, S = _grids(grids)
        L = lib()
        if S > int(L.iamx_ortho_max_steps()):
            raise ValueError("grid_steps %d: the rasteriser takes at most %d" % (S, L.iamx_ortho_max_steps()))
        self.g, self.mode, self.names = g, mode, list(names) if names is not None else None
        self.width, self.height = float(width), float(height)
        self.rf = rf = raster_frame(g, gsd)
        self.cells, self.verts = used_cells(g)
        dev = self.dev = require_gpu()
        need = rf.W * rf.H * BYTES_PER_PIXEL[mode]
        if mode == 'multiband':
            self.sizes = band_levels(rf.H, rf.W, bands)
            self.boxes = [pixel_box(rf.X[k], rf.Y[k], self.verts[k], rf.W, rf.H) for k in range(len(g))]
            stay, metric, temp = multiband_bytes(self.sizes, self.boxes)
            need = stay + max(metric, temp)
        free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        if need > free:
            raise MemoryError("a %d x %d pixel mosaic (mode %s) needs %.2f GB of accumulators, %.2f GB of device "
                              "memory are free: use a coarser gsd (band splitting is not implemented)"
                              % (rf.W, rf.H, mode, need / 1e9, free / 1e9))
        uv = np.asarray(uvs, np.float64)
        if uv.ndim == 2:
            uv = np.broadcast_to(uv, (len(g),) + uv.shape)
        if uv.shape != (len(g), g.shape[1], 2) or not np.isfinite(uv).all():
            raise ValueError("uvs must be finite, [(S+1)^2][2] for the group or per image")
        self.shared_uv = all(np.array_equal(uv[0], u) for u in uv[1:])
        self.uv = kernels._dev(uv[:1] if self.shared_uv else uv, kernels.F64)
        self.xy = kernels._dev(np.stack([rf.X, rf.Y], axis=1), kernels.I32)           # [N][2][V]
        self.used = kernels._dev(rf.used, kernels.U8)
        torch.cuda.current_stream().synchronize()          # (the uploads' staging copies have been read)
        n = (rf.H, rf.W)
        self._p = kernels._ptr
        self._call = (L, check, stream_ptr)
        self.done = 0
        if mode == 'multiband':
            self._init_multiband(torch, temp)
            return
        self.acc = torch.empty(n if mode == 'best' else n + (4,), dtype=torch.float64, device=dev)
        self.index = torch.empty(n, dtype=torch.int32, device=dev) if mode == 'best' else None
        self.count = torch.empty(n, dtype=torch.uint16, device=dev)
        self.bgr = torch.empty(n + (3,), dtype=torch.uint8, device=dev)
        check(L.iamx_ortho_clear(MODES[mode], rf.H, rf.W, self._p(self.acc), self._p(self.index),
                                 self._p(self.count), self._p(self.bgr), stream_ptr()), 'iamx_ortho_clear')

    # ---- mode multiband ----
    def _params(self, k):
        terms = image_terms(self.g[k], self.verts[k])
        if terms is None:
            return None
        rf = self.rf
        return (ctypes.c_double * 8)(self.width, self.height, rf.x0, rf.y1, rf.gsd, *terms)

    def _init_multiband(self, torch, temp_bytes):
        """the ownership pass (mode best's index and count, from the geometry alone), then the
        accumulators of every level, zeroed, and the layer pyramid's buffer"""
        L, check, stream_ptr = self._call
        rf, p, dev = self.rf, self._p, self.dev
        n = (rf.H, rf.W)
        self.index = torch.empty(n, dtype=torch.int32, device=dev)
        self.count = torch.empty(n, dtype=torch.uint16, device=dev)
        self.bgr = torch.empty(n + (3,), dtype=torch.uint8, device=dev)
        metric = torch.empty(n, dtype=torch.float64, device=dev)
        check(L.iamx_ortho_clear(MODES['best'], rf.H, rf.W, p(metric), p(self.index), p(self.count), p(self.bgr),
                                 stream_ptr()), 'iamx_ortho_clear')
        for k in range(len(self.g)):
            params = self._params(k)
            if params is None:
                continue
            xy = self.xy[k]
            check(L.iamx_ortho_mb_owner(rf.S, p(xy[0]), p(xy[1]), p(self.used[k]), params, k, *self.boxes[k],
                                        rf.H, rf.W, p(metric), p(self.index), p(self.count), stream_ptr()),
                  'iamx_ortho_mb_owner')
        del metric                                         # (stream ordered: the allocator hands it on in order)
        self._mb_alloc(torch, temp_bytes)

    def _mb_plan(self, k):
        """image k's launch arguments: (params, pixel box, per-level regions, per-level layer buffers);
        None when it has no used cell or covers no pixel centre"""
        params = self._params(k)
        box = self.boxes[k]
        if params is None or box[2] < box[0] or box[3] < box[1]:
            return None
        return (params, box) + self._mb_layers(box)

    def _mb_layer(self, k, frame, plan):
        """kernel (a): C_k and A_k over the image's pixel box"""
        L, check, stream_ptr = self._call
        rf, p = self.rf, self._p
        params, box, _regions, layers = plan
        xy = self.xy[k]
        check(L.iamx_ortho_mb_layer(rf.S, p(xy[0]), p(xy[1]), p(self.uv[0 if self.shared_uv else k]), p(self.used[k]),
                                    p(frame), int(frame.shape[0]), int(frame.shape[1]), params, int(k), *box,
                                    rf.H, rf.W, p(self.index), p(layers[0]), stream_ptr()), 'iamx_ortho_mb_layer')

    def _add_multiband(self, k, frame):
        plan = self._mb_plan(k)
        if plan is not None:
            self._mb_layer(k, frame, plan)
            self._mb_pyramid(plan)

    def _finish_multiband(self):
        rf = self.rf
        self._mb_finish()
        return Mosaic(bgr=self.bgr, index=self.index, count=self.count, x0=rf.x0, y1=rf.y1, gsd=rf.gsd,
                      mode=self.mode, names=self.names, bands=self.bands)

    def add(self, k, frame):
        L, check, stream_ptr = self._call
        rf, p = self.rf, self._p
        frame = _check_frame(frame)
        if self.mode == 'multiband':
            self._add_multiband(k, frame)
            self.done += 1
            return
        terms = image_terms(self.g[k], self.verts[k])
        if terms is None:
            self.done += 1
            return
        c0, r0, c1, r1 = pixel_box(rf.X[k], rf.Y[k], self.verts[k], rf.W, rf.H)
        params = (ctypes.c_double * 8)(self.width, self.height, rf.x0, rf.y1, rf.gsd, *terms)
        xy = self.xy[k]
        check(L.iamx_ortho_raster_image(MODES[self.mode], rf.S, p(xy[0]), p(xy[1]),
                                        p(self.uv[0 if self.shared_uv else k]), p(self.used[k]), p(frame),
                                        int(frame.shape[0]), int(frame.shape[1]), params, int(k), c0, r0, c1, r1,
                                        rf.H, rf.W, p(self.acc), p(self.index), p(self.count), p(self.bgr),
                                        stream_ptr()), 'iamx_ortho_raster_image')
        self.done += 1

    def finish(self):
        L, check, stream_ptr = self._call
        rf, p = self.rf, self._p
        if self.mode == 'multiband':
            return self._finish_multiband()
        if self.mode == 'feather':
            check(L.iamx_ortho_resolve(rf.H, rf.W, p(self.acc), p(self.count), p(self.bgr), stream_ptr()),
                  'iamx_ortho_resolve')
        return Mosaic(bgr=self.bgr, index=self.index, count=self.count, x0=rf.x0, y1=rf.y1, gsd=rf.gsd,
                      mode=self.mode, names=self.names)


def compose(grids, uvs, frames, width, height, gsd, mode='best', names=None, bands=5):
    """The rasteriser on ready arrays: grids [N][(S+1)^2][3] ENU, uvs [(S+1)^2][2] (one for the group)
    or [N][(S+1)^2][2], frames: N device uint8 [h,w,3] tensors, width x height: the camera's image
    size; bands: mode multiband's pyramid levels, 1 .. 16.  -> Mosaic"""
    comp = _Composer(grids, uvs, width, height, gsd, mode, names, bands)
    frames = list(frames)
    if len(frames) != len(comp.g):
        raise ValueError("%d frames for %d grids" % (len(frames), len(comp.g)))
    for k, frame in enumerate(frames):
        comp.add(k, frame)
    return comp.finish()


def _vignette_mask(analysis_dir):
    from . import histogram as _histogram, kernels
    path = os.path.join(analysis_dir, 'models', 'vignette-mask.jpg')
    if not os.path.exists(path):
        raise FileNotFoundError("%s: make it with 99-vignette.py first" % path)
    with open(path, 'rb') as fp, kernels.polite_waits():
        return _histogram._decode_frame(fp.read())


_IDENTITY_LUT = np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def prepare_frame(frame, name, grid, cells, gsd, prefilter=True, histogram=False, mask=None):
    """what render() does to a decoded frame before it is rasterised: histogram.lookup_tables and
    the vignette mask through kernels.colour_lut, then kernels.resize_area by prefilter_factor()
    when that is below 0.75.  -> (frame, shrunk?)"""
    from . import histogram as _histogram, kernels
    frame = _check_frame(frame)
    lut = _histogram.lookup_tables(name) if histogram else None
    if histogram and lut is None:
        _log("histogram: no neighbour template for", name, "(image left as it is)")
    if lut is not None or mask is not None:
        if mask is not None and tuple(mask.shape) != tuple(frame.shape):
            raise ValueError("%s: the frame is %d x %d, the vignette mask %d x %d"
                             % (name, frame.shape[1], frame.shape[0], mask.shape[1], mask.shape[0]))
        frame = kernels.colour_lut(frame, lut if lut is not None else _IDENTITY_LUT, mask)
    if prefilter:
        f = prefilter_factor(grid, cells, frame.shape[1], frame.shape[0], gsd)
        if f < PREFILTER_BELOW and round(frame.shape[0] * f) >= 1 and round(frame.shape[1] * f) >= 1:
            return kernels.resize_area(frame, f, f), True
    return frame, False


def group_grids(proj, group_list, group_index, matches=None):
    """The group's grids from the code that makes the .egg files: render_panda3d.elevation_stats and
    render_panda3d.map_grids (nothing is written).  -> (images, grids [N][(S+1)^2][3], uv)"""
    import pickle
    from . import render_panda3d as rp
    if matches is None:
        with open(os.path.join(proj.analysis_dir, "matches_grouped"), "rb") as f:
            matches = pickle.load(f)
    group = group_list[group_index]
    ref_node = getNode("/config/ned_reference", True)
    ref = [ref_node.getFloat('lat_deg'), ref_node.getFloat('lon_deg'), ref_node.getFloat('alt_m')]
    raw_points, raw_values = rp.elevation_stats(proj, group, group_index, matches)
    images = rp.map_grids(proj, group, raw_points, raw_values, rp.switches(), ref)
    grids = np.array([im.grid_list for im in images], np.float64)
    return images, grids, np.array(images[0].distorted_uv, np.float64)


def render(proj, group_list, group_index, gsd, mode='best', prefilter=True, histogram=False, vignette=False,
           frames=None, matches=None, bands=5):
    """The orthomosaic of one group.  The frames are decoded by histogram.frame_pass (in group
    order, on this thread's stream); frames=: ready device tensors, one per image of the group,
    instead.  histogram / vignette: the explorer's colour tables (histogram.load() must have found
    the project's file; models/vignette-mask.jpg must exist).  bands: mode multiband's pyramid levels.
    -> Mosaic"""
    from . import histogram as _histogram
    t0 = time.perf_counter()
    camera = _deps.camera()
    images, grids, uv = group_grids(proj, group_list, group_index, matches)
    width, height = camera.get_image_params()
    names = [im.name for im in images]
    comp = _Composer(grids, uv, width, height, gsd, mode, names, bands)
    mask = _vignette_mask(proj.analysis_dir) if vignette else None
    state = {'k': 0, 'shrunk': 0}

    def on_frames(batch):
        for frame in batch:
            k = state['k']
            frame, shrunk = prepare_frame(frame, names[k], grids[k], comp.cells[k], gsd, prefilter, histogram, mask)
            comp.add(k, frame)
            state['k'] = k + 1
            state['shrunk'] += 1 if shrunk else 0

    if frames is not None:
        frames = list(frames)
        if len(frames) != len(images):
            raise ValueError("%d frames for the group's %d images" % (len(frames), len(images)))
        on_frames(frames)
    else:
        _histogram.frame_pass(images, want_hist=False, on_frames=on_frames)
    if state['k'] != len(images):
        raise RuntimeError("%d of %d frames arrived" % (state['k'], len(images)))
    mosaic = comp.finish()
    dt = time.perf_counter() - t0
    render_stats.update(images=len(images), prefiltered=state['shrunk'], seconds=dt,
                        frames_per_s=len(images) / dt if dt > 0 else 0.0)
    return mosaic


# ---------------------------------------------------------------------------------------------
# true orthophoto over the dense DSM (THE TRUE-ORTHO RULES)
# ---------------------------------------------------------------------------------------------
DENSE_MODES = ('best', 'feather')
MAX_UPSAMPLE = 8
BOX_STRIDE = 32                # every 32nd border pixel, and the corners
BOX_MARGIN = 2.0               # mosaic pixels
BOX_GROW = 1.0 / 64.0          # of the box's longer side

# the last render_dense(): images, frames shrunk, seconds
render_dense_stats = {'images': 0, 'prefiltered': 0, 'seconds': 0.0, 'frames_per_s': 0.0}


def border_pixels(w, h):
    """(x, y) of the frame's corners and every 32nd pixel of its border -> int64 [n][2]"""
    xs = sorted(set(range(0, w, BOX_STRIDE)) | {w - 1})
    ys = sorted(set(range(0, h, BOX_STRIDE)) | {h - 1})
    pts = [(x, y) for y in (0, h - 1) for x in xs] + [(x, y) for x in (0, w - 1) for y in ys]
    return np.array(sorted(set(pts)), np.int64)


def work_box(K, dist, R, C, w, h, z_lo, z_hi, x0, y1, g, Ho, Wo, rays=None):
    """The work box of one image (THE TRUE-ORTHO RULES): K = (fx, fy, cx, cy) at the frame's size
    w x h, z_lo and z_hi the smallest and the largest finite DSM height, g the mosaic's pixel size.
    rays: the undistorted normalised coordinates [n][2] of border_pixels(w, h) (default:
    undistort.undistort_points, on the device).  -> inclusive (c0, r0, c1, r1) in mosaic pixels"""
    K = np.asarray(K, np.float64).reshape(4)
    R = np.asarray(R, np.float64).reshape(3, 3)
    C = np.asarray(C, np.float64).reshape(3)
    whole = (0, 0, Wo - 1, Ho - 1)
    if rays is None:
        from . import undistort
        und = undistort.undistort_points(border_pixels(w, h).astype(np.float32), K, dist).astype(np.float64)
        rays = np.stack([(und[:, 0] - K[2]) / K[0], (und[:, 1] - K[3]) / K[1]], 1)
    rays = np.asarray(rays, np.float64).reshape(-1, 2)
    d = rays[:, :1] * R[0] + rays[:, 1:] * R[1] + R[2]             # R^T (xn, yn, 1), NED
    if not (np.isfinite(d).all() and (d[:, 2] > 0).all() and -C[2] > z_hi):
        return whole
    cols, rows = [], []
    for z in (z_lo, z_hi):
        t = (-z - C[2]) / d[:, 2]
        cols.append((C[1] + t * d[:, 1] - x0) / g)
        rows.append((y1 - (C[0] + t * d[:, 0])) / g)
    cols, rows = np.concatenate(cols), np.concatenate(rows)
    if not (np.isfinite(cols).all() and np.isfinite(rows).all()):
        return whole
    lo_c, hi_c, lo_r, hi_r = floor(cols.min()), ceil(cols.max()), floor(rows.min()), ceil(rows.max())
    grow = BOX_MARGIN + BOX_GROW * max(hi_c - lo_c, hi_r - lo_r)
    clip = lambda v, n: int(min(max(v, -1.0), float(n)))          # (before int(): a far hit stays a small number)
    return (max(clip(lo_c - grow, Wo), 0), max(clip(lo_r - grow, Ho), 0),
            min(clip(ceil(hi_c + grow), Wo), Wo - 1), min(clip(ceil(hi_r + grow), Ho), Ho - 1))


def _camera_of(cam):
    """a (K, width, height, dist, R, C) tuple or a dense.View-like object (its K is at its plane's
    size) -> (K, width, height, dist [5], R [3, 3], C [3])"""
    if hasattr(cam, 'K') and hasattr(cam, 'R'):
        G = getattr(cam, 'G', None)
        if G is None or len(G.shape) < 2:
            raise ValueError("a view given as a camera carries its plane G [h, w]: its size is the camera's")
        cam = (cam.K, int(G.shape[1]), int(G.shape[0]), cam.dist, cam.R, cam.C)
    if len(cam) != 6:
        raise ValueError("a camera is (K, width, height, dist, R, C)")
    K, width, height, dist, R, C = cam
    dist, R, C = (np.asarray(dist, np.float64).reshape(5), np.asarray(R, np.float64).reshape(3, 3),
                  np.asarray(C, np.float64).reshape(3))
    if not (float(width) >= 1 and float(height) >= 1 and np.isfinite(np.asarray(K, np.float64)).all()
            and np.isfinite(dist).all() and np.isfinite(R).all() and np.isfinite(C).all()):
        raise ValueError("a camera is finite and at least 1 x 1 pixel")
    return np.asarray(K, np.float64), float(width), float(height), dist, R, C


def _check_dense_frame(frame):
    shape = tuple(getattr(frame, 'shape', ()))
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 2 or shape[1] < 2:
        raise ValueError("a frame is uint8 [h, w, 3], at least 2 x 2 (got %r)" % (shape,))


def surface_heights(dsm):
    """(the smallest, the largest, the mean) finite height of a device DSM, as floats"""
    import torch
    finite = dsm[torch.isfinite(dsm)]
    if finite.numel() == 0:
        raise ValueError("the DSM has no finite cell: nothing to drape over")
    return float(finite.min()), float(finite.max()), float(finite.double().mean())


def _check_bands(mode, bands):
    """compose_dense's bands: 0 (no blend) .. 16, an integer; a blend follows mode best's seams"""
    if mode == 'multiband':
        raise ValueError("mode multiband over a dense surface is asked for with bands=: mode='best', bands=1 .. %d"
                         % MAX_BANDS)
    if mode not in DENSE_MODES:
        raise ValueError("mode must be 'best' or 'feather'")
    if isinstance(bands, bool) or not isinstance(bands, (int, np.integer)) or not 0 <= int(bands) <= MAX_BANDS:
        raise ValueError("bands is an integer 0 .. %d (got %r)" % (MAX_BANDS, bands))
    if bands and mode != 'best':
        raise ValueError("bands=%d blends along mode best's seams: mode %s takes bands=0 only" % (bands, mode))
    return int(bands)


class _DenseComposer(_Pyramids):
    """the accumulators of one true orthophoto and the DSM on the device; add(k, camera, frame)
    drapes image k (call it in group order), finish() -> Mosaic.  bands > 0 (mode multiband's blend
    along best's seams) wants every camera and every frame's (h, w) up front (frame_sizes: a list, or
    a function of this composer that returns one): the owner pass runs here, add() then takes the
    frames, each of the size it was announced with."""

    def __init__(self, surface, mode, upsample, bias, names=None, bands=0, cameras=None, frame_sizes=None):
        import torch
        from . import kernels
        from ._lib import check, lib, require_gpu, stream_ptr
        bands = _check_bands(mode, bands)
        if isinstance(upsample, bool) or int(upsample) != upsample or not 1 <= int(upsample) <= MAX_UPSAMPLE:
            raise ValueError("upsample is an integer 1 .. %d (got %r)" % (MAX_UPSAMPLE, upsample))
        gsd = float(surface.gsd)
        if not (gsd > 0.0 and np.isfinite(gsd) and np.isfinite(surface.x0) and np.isfinite(surface.y1)):
            raise ValueError("the surface's frame must be finite, gsd positive")
        bias = 1.0 * gsd if bias is None else float(bias)
        if not (bias >= 0.0 and np.isfinite(bias)):
            raise ValueError("bias is a finite number of metres, at least 0 (got %r)" % bias)
        if len(surface.dsm.shape) != 2 or min(surface.dsm.shape) < 1:
            raise ValueError("a DSM is [H, W]")
        if bands:
            mode = 'multiband'
            if cameras is None or frame_sizes is None:
                raise ValueError("bands > 0 wants every camera and every frame's (h, w) before the first frame")
            cameras = [_camera_of(cam) for cam in cameras]
        self.mode, self.ss, self.bias, self.names = mode, int(upsample), bias, list(names) if names is not None else None
        H, W = (int(v) for v in surface.dsm.shape)
        self.Ho, self.Wo, self.g = H * self.ss, W * self.ss, gsd / self.ss
        if self.Ho > MAX_SIDE or self.Wo > MAX_SIDE:
            raise ValueError("a %d x %d pixel mosaic: a side above 2^20 pixels is refused" % (self.Wo, self.Ho))
        self.x0, self.y1, self.gsd = float(surface.x0), float(surface.y1), gsd
        dev = self.dev = require_gpu()
        need = self.Wo * self.Ho * BYTES_PER_PIXEL[mode]
        if bands:
            # (the boxes want the DSM's heights on the device: first what holds whatever they are)
            self.sizes = band_levels(self.Ho, self.Wo, bands)
            stay, metric, _temp = multiband_bytes(self.sizes, [])
            need = stay + metric + 4 * H * W
        self._fits(torch, need)
        self.dsm = kernels._dev(surface.dsm, torch.float32)
        self.z_lo, self.z_hi, self.z_mean = surface_heights(self.dsm)
        n = (self.Ho, self.Wo)
        self._p, self._kernels = kernels._ptr, kernels
        self._call = (lib(), check, stream_ptr)
        if bands:
            self._init_multiband(torch, cameras, frame_sizes)
            return
        self.acc = torch.empty(n if mode == 'best' else n + (4,), dtype=torch.float64, device=dev)
        self.index = torch.empty(n, dtype=torch.int32, device=dev) if mode == 'best' else None
        self.count = torch.empty(n, dtype=torch.uint16, device=dev)
        self.bgr = torch.empty(n + (3,), dtype=torch.uint8, device=dev)
        L, p = self._call[0], self._p
        check(L.iamx_ortho_clear(MODES[mode], self.Ho, self.Wo, p(self.acc), p(self.index), p(self.count), p(self.bgr),
                                 stream_ptr()), 'iamx_ortho_clear')

    def _fits(self, torch, need):
        free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        if need > free:
            raise MemoryError("a %d x %d pixel mosaic (mode %s) needs %.2f GB of accumulators, %.2f GB of device "
                              "memory are free: use a smaller upsample (band splitting is not implemented)"
                              % (self.Wo, self.Ho, self.mode, need / 1e9, free / 1e9))

    def box(self, K, dist, R, C, w, h):
        return work_box(K, dist, R, C, w, h, self.z_lo, self.z_hi, self.x0, self.y1, self.g, self.Ho, self.Wo)

    def _image(self, camera, h, w):
        """-> (the kernels' parameters, the work box) of a camera with an h x w frame"""
        from . import dense
        K, width, height, dist, R, C = camera
        Ks = dense.scaled_K(K, width, height, w, h)
        params = self._kernels.ortho_dsm_params(self.x0, self.y1, self.gsd, self.bias, self.z_hi, Ks, dist, R, C)
        return params, self.box(Ks, dist, R, C, w, h)

    # ---- bands > 0: mode multiband's blend ----
    def _init_multiband(self, torch, cameras, frame_sizes):
        """the owner pass (mode best's index and count, from the geometry and the frame sizes alone),
        then the accumulators of every level, zeroed, and the layer pyramid's buffer"""
        L, check, stream_ptr = self._call
        p, dev, n = self._p, self.dev, (self.Ho, self.Wo)
        if callable(frame_sizes):                          # (render_dense: they depend on the DSM's mean height)
            frame_sizes = frame_sizes(self)
        self.frame_sizes = frame_sizes = [(int(h), int(w)) for h, w in frame_sizes]
        if len(frame_sizes) != len(cameras) or any(h < 2 or w < 2 for h, w in frame_sizes):
            raise ValueError("one frame size (h, w), at least 2 x 2, per camera")
        self.images = [self._image(cam, h, w) for cam, (h, w) in zip(cameras, frame_sizes)]
        stay, metric_bytes, temp_bytes = multiband_bytes(self.sizes, [box for _params, box in self.images])
        self._fits(torch, stay + max(metric_bytes, temp_bytes))      # (the DSM is allocated by now)
        self.index = torch.empty(n, dtype=torch.int32, device=dev)
        self.count = torch.empty(n, dtype=torch.uint16, device=dev)
        self.bgr = torch.empty(n + (3,), dtype=torch.uint8, device=dev)
        metric = torch.empty(n, dtype=torch.float64, device=dev)
        check(L.iamx_ortho_clear(MODES['best'], self.Ho, self.Wo, p(metric), p(self.index), p(self.count), p(self.bgr),
                                 stream_ptr()), 'iamx_ortho_clear')
        for k, ((params, box), hw) in enumerate(zip(self.images, frame_sizes)):
            self._kernels.ortho_dsm_owner(self.dsm, self.ss, params, hw, k, box, metric, self.index, self.count)
        del metric                                         # (stream ordered: the allocator hands it on in order)
        self._mb_alloc(torch, temp_bytes)

    def _mb_plan(self, k):
        """image k's launch arguments: (params, work box, per-level regions, per-level layer buffers);
        None when its work box is empty"""
        params, box = self.images[k]
        if box[2] < box[0] or box[3] < box[1]:
            return None
        return (params, box) + self._mb_layers(box)

    def _mb_layer(self, k, frame, plan):
        """C_k and A_k over the image's work box"""
        params, box, _regions, layers = plan
        self._kernels.ortho_dsm_layer(self.dsm, self.ss, params, frame, k, box, self.index, layers[0])

    def _add_multiband(self, k, frame):
        if self.finished:
            raise RuntimeError("add() after finish(): the collapse works in place")
        name = self.names[k] if self.names is not None else 'image %d' % k
        if (int(frame.shape[0]), int(frame.shape[1])) != self.frame_sizes[k]:
            raise RuntimeError("%s: a %d x %d frame arrived where the owner pass was told %d x %d (nothing of it "
                               "is accumulated)" % ((name, frame.shape[1], frame.shape[0]) + self.frame_sizes[k][::-1]))
        frame = self._kernels._dev(frame, self._kernels.U8)
        plan = self._mb_plan(k)
        if plan is not None:
            self._mb_layer(k, frame, plan)
            self._mb_pyramid(plan)

    def add(self, k, camera, frame):
        """bands > 0: the camera is the one the owner pass was given for image k, and is not read again"""
        _check_dense_frame(frame)
        if self.mode == 'multiband':
            return self._add_multiband(k, frame)
        frame = self._kernels._dev(frame, self._kernels.U8)
        params, box = self._image(_camera_of(camera), int(frame.shape[0]), int(frame.shape[1]))
        self._kernels.ortho_dsm_image(MODES[self.mode], self.dsm, self.ss, params, frame, k, box, self.acc, self.index,
                                      self.count, self.bgr)

    def finish(self):
        L, check, stream_ptr = self._call
        p = self._p
        extra = {}
        if self.mode == 'multiband':
            self._mb_finish()
            extra['bands'] = self.bands
        if self.mode == 'feather':
            check(L.iamx_ortho_resolve(self.Ho, self.Wo, p(self.acc), p(self.count), p(self.bgr), stream_ptr()),
                  'iamx_ortho_resolve')
        return Mosaic(bgr=self.bgr, index=self.index, count=self.count, x0=self.x0, y1=self.y1, gsd=self.g,
                      mode=self.mode, names=self.names, surface='dense', upsample=self.ss, bias=self.bias, **extra)


def compose_dense(surface, cameras, frames, mode='best', upsample=1, bias=None, names=None, bands=0):
    """The true orthophoto on ready arrays (THE TRUE-ORTHO RULES): surface a dense.Surface (filled:
    dense.fill), cameras a list of (K at camera size, width, height, dist, R NED -> camera, C NED) or
    of dense.View-like objects, frames one BGR uint8 [h, w, 3] per camera (device tensors or numpy),
    of any size at least 2 x 2; upsample: mosaic pixels per DSM cell and side, 1 .. 8; bias: metres a
    DSM cell must stand above the ray to hide the point, None: 1.0 * surface.gsd -- a default no real
    DSM has been measured against; bands: 0, or with mode best 1 .. 16 pyramid levels of mode
    multiband's blend along best's seams.  -> Mosaic (gsd: the mosaic's, surface.gsd / upsample; with
    bands: mode 'multiband', bands the levels used)"""
    cameras, frames = list(cameras), list(frames)
    if len(frames) != len(cameras):
        raise ValueError("%d frames for %d cameras" % (len(frames), len(cameras)))
    if mode not in MODES:
        raise ValueError("mode must be 'best' or 'feather'")
    for cam, frame in zip(cameras, frames):                # (every ValueError before any device call)
        _camera_of(cam)
        _check_dense_frame(frame)
    comp = _DenseComposer(surface, mode, upsample, bias, names, bands, cameras,
                          [tuple(frame.shape[:2]) for frame in frames])
    for k, (cam, frame) in enumerate(zip(cameras, frames)):
        comp.add(k, cam, frame)
    return comp.finish()


def dense_prefilter_factor(K, C, z_mean, g):
    """f = min(1, native / g), native = (-C_2 - mean finite dsm) / sqrt(fx fy) at camera size: the
    metres one frame pixel spans on the mean surface over the mosaic's pixel size"""
    K = np.asarray(K, np.float64)
    fx, fy = (K[0, 0], K[1, 1]) if K.shape == (3, 3) else K.reshape(4)[:2]
    native = (-float(C[2]) - float(z_mean)) / sqrt(fx * fy)
    return min(1.0, native / float(g))


def _colour_frame(frame, name, histogram, mask):
    """prepare_frame's colour step: histogram.lookup_tables and the vignette mask through kernels.colour_lut"""
    from . import histogram as _histogram, kernels
    lut = _histogram.lookup_tables(name) if histogram else None
    if histogram and lut is None:
        _log("histogram: no neighbour template for", name, "(image left as it is)")
    if lut is None and mask is None:
        return frame
    if mask is not None and tuple(mask.shape) != tuple(frame.shape):
        raise ValueError("%s: the frame is %d x %d, the vignette mask %d x %d"
                         % (name, frame.shape[1], frame.shape[0], mask.shape[1], mask.shape[0]))
    return kernels.colour_lut(frame, lut if lut is not None else _IDENTITY_LUT, mask)


def _dense_frame_size(h, w, f, prefilter):
    """render_dense's prefilter decision for an h x w frame with the factor f -> (the size (h, w) the
    frame is draped at, shrunk?)"""
    if prefilter and f < PREFILTER_BELOW and round(h * f) >= 2 and round(w * f) >= 2:
        from . import kernels
        return kernels.resize_area_shape(h, w, f, f), True
    return (int(h), int(w)), False


def render_dense(proj, group_list, group_index, surface, mode='best', upsample=1, bias=None, prefilter=True,
                 histogram=False, vignette=False, frames=None, bands=0):
    """The true orthophoto of one group over `surface` (dense.load, then dense.fill): poses from
    dense.image_pose, the optimised K and distortion as dense.views_from_project takes them, the
    frames decoded by histogram.frame_pass in group order (frames=: ready device tensors instead),
    the colour tables as prepare_frame applies them, and kernels.resize_area by
    dense_prefilter_factor() when that is below 0.75.  bands: compose_dense's; the owner pass then
    runs before the first frame, on the sizes the frames will have (the camera's image size, or the
    tensors' with frames=, after the prefilter decision), and a frame that arrives with another size
    is a RuntimeError naming the image.  -> Mosaic"""
    from . import dense, histogram as _histogram, kernels
    t0 = time.perf_counter()
    camera = _deps.camera()
    K = np.asarray(camera.get_K(optimized=True), np.float64)
    dist = np.array(camera.get_dist_coeffs(optimized=True), np.float64).ravel()[:5]
    width, height = camera.get_image_params()
    group = dense.group_indices(proj, group_list, group_index)
    images = [proj.image_list[i] for i in group]
    names = [im.name for im in images]
    if frames is not None:
        frames = list(frames)
        if len(frames) != len(images):
            raise ValueError("%d frames for the group's %d images" % (len(frames), len(images)))
    cameras = raw = sizes = None
    if _check_bands(mode, bands):
        # the owner pass wants every frame's size before the first frame; the prefilter decision wants
        # the DSM's mean height, which the composer knows once the DSM is on the device
        cameras = [(K, width, height, dist) + tuple(dense.image_pose(im)) for im in images]
        raw = [tuple(int(v) for v in f.shape[:2]) for f in frames] if frames is not None else \
            [(int(height), int(width))] * len(images)

        def sizes(comp):
            return [_dense_frame_size(h, w, dense_prefilter_factor(K, cam[5], comp.z_mean, comp.g), prefilter)[0]
                    for (h, w), cam in zip(raw, cameras)]
    comp = _DenseComposer(surface, mode, upsample, bias, names, bands, cameras, sizes)
    mask = _vignette_mask(proj.analysis_dir) if vignette else None
    state = {'k': 0, 'shrunk': 0}

    def on_frames(batch):
        for frame in batch:
            k = state['k']
            if raw is not None and tuple(int(v) for v in frame.shape[:2]) != raw[k]:
                raise RuntimeError("%s: a %d x %d frame arrived where the owner pass was told %d x %d (nothing of "
                                   "it is accumulated)" % ((names[k], frame.shape[1], frame.shape[0]) + raw[k][::-1]))
            frame = _colour_frame(_check_frame(frame), names[k], histogram, mask)
            R, C = dense.image_pose(images[k])
            if prefilter:
                f = dense_prefilter_factor(K, C, comp.z_mean, comp.g)
                if _dense_frame_size(int(frame.shape[0]), int(frame.shape[1]), f, True)[1]:
                    frame = kernels.resize_area(frame, f, f)
                    state['shrunk'] += 1
            comp.add(k, (K, width, height, dist, R, C), frame)
            state['k'] = k + 1

    if frames is not None:
        on_frames(frames)
    else:
        _histogram.frame_pass(images, want_hist=False, on_frames=on_frames)
    if state['k'] != len(images):
        raise RuntimeError("%d of %d frames arrived" % (state['k'], len(images)))
    mosaic = comp.finish()
    dt = time.perf_counter() - t0
    render_dense_stats.update(images=len(images), prefiltered=state['shrunk'], seconds=dt,
                              frames_per_s=len(images) / dt if dt > 0 else 0.0)
    return mosaic


def world_file_text(gsd, west, north):
    """the six lines of a world file for a north-up tile whose upper-left CORNER is (west, north)"""
    vals = (gsd, 0.0, 0.0, -gsd, west + 0.5 * gsd, north - 0.5 * gsd)
    return "".join("%r\n" % float(v) for v in vals)


def save(mosaic, analysis_dir, tile=4096, fmt='jpg', subdir='ortho'):
    """<analysis_dir>/<subdir>/tile_<row>_<col>.<fmt> through Pillow (jpg: panda3d.encode_jpeg's
    settings), a world file per tile (local ENU metres, the pixel-centre convention) and ortho.json:
    /config/ned_reference, gsd, bounds, mode (multiband: and bands; a true orthophoto: and surface,
    upsample, bias), per-tile bounds, the image names.  -> the json's dict"""
    from PIL import Image as PILImage
    from . import panda3d
    tile = int(tile)
    if tile < 1:
        raise ValueError("tile must be at least 1 pixel")
    fmt = fmt.lower().lstrip('.')
    out_dir = os.path.join(analysis_dir, subdir)
    os.makedirs(out_dir, exist_ok=True)
    H, W = mosaic.shape
    gsd, x0, y1 = float(mosaic.gsd), float(mosaic.x0), float(mosaic.y1)
    ref_node = getNode("/config/ned_reference", True)
    tiles = []
    for tr in range((H + tile - 1) // tile):
        for tc in range((W + tile - 1) // tile):
            r0, c0 = tr * tile, tc * tile
            r1, c1 = min(r0 + tile, H), min(c0 + tile, W)
            pixels = mosaic.bgr[r0:r1, c0:c1].contiguous().cpu().numpy()
            name = 'tile_%d_%d.%s' % (tr, tc, fmt)
            if fmt in ('jpg', 'jpeg'):
                blob = panda3d.encode_jpeg(pixels)
            else:
                import io
                buf = io.BytesIO()
                PILImage.fromarray(np.ascontiguousarray(pixels[:, :, ::-1]), 'RGB').save(
                    buf, format={'tif': 'TIFF'}.get(fmt, fmt.upper()))
                blob = buf.getvalue()
            panda3d._write_atomic(os.path.join(out_dir, name), blob)
            west, north = x0 + c0 * gsd, y1 - r0 * gsd
            world = 'tile_%d_%d.%s' % (tr, tc, WORLD_EXT.get(fmt, 'wld'))
            panda3d._write_atomic(os.path.join(out_dir, world), world_file_text(gsd, west, north).encode())
            tiles.append({'file': name, 'world_file': world, 'row': tr, 'col': tc, 'width': c1 - c0,
                          'height': r1 - r0, 'west': west, 'east': x0 + c1 * gsd, 'north': north,
                          'south': y1 - r1 * gsd})
    info = {'ned_reference': {k: ref_node.getFloat(k) for k in ('lat_deg', 'lon_deg', 'alt_m')},
            'units': 'local ENU metres about ned_reference', 'gsd': gsd, 'mode': mosaic.mode,
            'width': W, 'height': H, 'tile': tile, 'format': fmt,
            'bounds': {'west': x0, 'east': x0 + W * gsd, 'north': y1, 'south': y1 - H * gsd},
            'tiles': tiles, 'images': list(mosaic.names) if mosaic.names is not None else []}
    if mosaic.mode == 'multiband':
        info['bands'] = int(mosaic.bands)
    if getattr(mosaic, 'surface', None) is not None:
        info['surface'] = mosaic.surface
        info['upsample'] = int(mosaic.upsample)
        info['bias'] = float(mosaic.bias)
    panda3d._write_atomic(os.path.join(out_dir, 'ortho.json'), json.dumps(info, indent=1).encode())
    return info
