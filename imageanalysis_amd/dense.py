"""Dense surface: plane-sweep depth maps of a group's images and a DSM raster fused from them, the
third stage beside the Step 5 map and the orthomosaic (the reference has no counterpart: its
surface is the sparse chains' Delaunay triangulation).

    views_from_project(proj, group_list, group_index, matches, scale)   the group's views
    choose_neighbours(matches, group, poses, n=4)        per image, the images to sweep against
    depth_range(matches, group, poses)                   per image, (z_near, z_far) from its chains
    depth_maps(views, neighbours, ranges, planes=64, ...)   sweep every view, cross-check -> DepthMaps
                                                         (regularize='sgm': SEMI-GLOBAL RULES)
    refine_planes(planes, ratio)                         the size T of the next level's plane set
    refine(views, neighbours, ranges, coarse, planes, ratio=4, ...)   one finer level, swept only around
                                                         the coarse depths -> DepthMaps (REFINEMENT RULES)
    fuse(views, depths, gsd, method='mean', ...)         surviving points -> Surface (dsm, count); method=
                                                         'robust': ROBUST FUSION RULES (and support)
    save(surface, analysis_dir, points=None)             dense/dsm.npy, count.npy, dsm.wld, dense.json
    load(analysis_dir)                                   the inverse of save -> Surface
    fill(surface, rounds=8)                              holes closed from their rims -> (Surface, round_of)

The kernels are csrc/dense_sweep.hip; tests/dense_restatement.py restates the rules below in numpy,
operation by operation, and the device result is held to it bit for bit (fill: csrc/ortho_dsm.hip's
iamx_dense_fill, restated by tests/ortho_dense_restatement.py).

THE RULES

View: one image at the sweep scale.  G, a float32 grey plane h x w (the same size for every view of
a call); K = (fx, fy, cx, cy) at that scale; dist, the five OpenCV coefficients (k1, k2, p1, p2, k3),
unchanged by scale; R, NED -> camera, float64 3 x 3; C, the camera centre in NED; rays [h][w][2], the
undistorted normalised coordinates (xn, yn) of the pixel centres (x, y integer), computed on the
device by undistort.undistort_points.

Geometry is float64, every product and sum rounded on its own, sums of three from the left.  Depth is
the reference camera's z.  The planes are fronto-parallel and uniform in inverse depth:
    step = (w_near - w_far) / (D - 1)   (0 for D = 1)      w_d = w_far + d step      z_d = 1 / w_d

Warp of reference pixel q to neighbour n on plane d:
    Xc = (xn z_d, yn z_d, z_d)
    Xw_i = ((Rr[0][i] Xc_0 + Rr[1][i] Xc_1) + Rr[2][i] Xc_2) + Cr_i                 (Rr^T Xc + Cr)
    D = Xw - Cn,  Xn_i = (Rn[i][0] D_0 + Rn[i][1] D_1) + Rn[i][2] D_2
    x = Xn_0 / Xn_2, y = Xn_1 / Xn_2, and synth.project's expressions as Python reads them:
    r2 = x x + y y;  rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
    xd = x rad + 2 p1 x y + p2 (r2 + 2 x x);  yd = y rad + p1 (r2 + 2 y y) + 2 p2 x y
    fx_ = fx xd + cx,  fy_ = fy yd + cy                                          (K of n)
The sample is valid iff Xn_2 > 0 and 0 <= fx_ <= w - 1 and 0 <= fy_ <= h - 1 (comparisons that a NaN
fails: anything not finite on the way is invalid).  Its value is bilinear in float32:
    x0 = floor(fx_), x1 = min(x0 + 1, w - 1), tx = float32(fx_ - x0); y likewise
    top = G[y0][x0] + (G[y0][x1] - G[y0][x0]) tx;  bot on row y1;  Wv = top + (bot - top) ty
It depends on (q, d, n) only: every window that contains q sees the same value.

Score of (p, d, n), float32, over the window of radius r (N = (2r+1)^2 pixels, row-major, every sum
started at the first pixel and taken in that order): invalid when the window leaves the reference
image or one of its warped samples is invalid.  With a the reference's and b the warped values,
    ma = (sum a) / N, mb = (sum b) / N                          correctly rounded quotients
    saa = sum (a - ma)^2, sbb = sum (b - mb)^2, sab = sum (a - ma)(b - mb)
    invalid unless saa >= min_var N                             (float32 product; the texture gate)
    den = float32(sqrt(float64(saa sbb)))                       the product rounded to float32 first
    invalid when den == 0;  s = sab / den, invalid when it is NaN
Aggregate: S_d(p) = (the float32 sum of the valid s in neighbour order) / their count, invalid
without one.

Winner: the largest S_d, the smallest d on a tie; best = -1 where every plane is invalid.  s_0 is
its score, s_m and s_p those of planes best - 1 and best + 1 (NaN where the plane does not exist or
is invalid).  In float32, when s_m and s_p are both valid and den = (s_m - 2 s_0) + s_p < 0:
off = (0.5 (s_m - s_p)) / den clamped to +-0.5, else off = 0.  In float64
    depth = float32(1 / (w_far + (best + off) step))
A pixel is kept iff best >= 0 and s_0 >= min_score; depth is NaN where it is not.  Outputs: plane
int32, score = s_0 (NaN for best = -1), depth, around = (s_m, s_0, s_p).  A NaN is 0x7fc00000.

SEMI-GLOBAL RULES (depth_maps(regularize='sgm'); kernels: csrc/dense_sgm.hip and the emission in
csrc/dense_sweep.hip; restated by tests/dense_sgm_restatement.py).  Between the aggregate scores and
the winner stands a semi-global aggregation (Hirschmueller) of the cost volume; everything but the two
float32 operations of the select is integer arithmetic, so the result does not depend on scheduling.

Cost.  S_d(p) is the aggregate score above, float32, invalid where it is above.  C(p, d) is uint8:
255 where S_d(p) is invalid, otherwise clamp(rint((1.0f - S) 127.0f), 0, 254) -- each float32 operation
rounded on its own, rint half to even, the clamp after the rounding.  The volume is [h][w][planes],
planes contiguous.  The mode takes 2 <= planes <= 64 (IAMX_DENSE_SGM_MAX_PLANES: one plane per lane
of a wave); anything else is a ValueError before any device call.

Working cost.  C'(p, d) = C(p, d) if C < 255, else c_invalid, a parameter in 0 .. 254 that defaults
to 127, which is score 0.

Paths.  The directions (dx, dy) in this order: (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,-1) (1,-1) (-1,1);
paths = 4 takes the first four, paths = 8 all, no other value is allowed.  For direction r and pixel p:
if p - r lies outside the image, L_r(p, d) = C'(p, d); otherwise, with m = min_k L_r(p - r, k),
    L_r(p, d) = C'(p, d) + min(L_r(p-r, d), L_r(p-r, d-1) + P1, L_r(p-r, d+1) + P1, m + P2) - m
where planes d +- 1 outside [0, planes) do not exist.  0 <= P1 <= P2 <= 255.  Hence
L_r <= 254 + P2 <= 509 and T(p, d) = sum_r L_r(p, d) <= 4072 fits a uint16.

Select.  best = argmin_d T(p, d), the smallest d on a tie: always >= 0, also where every raw cost is
255 (a propagated plane).  With T_0 = T(p, best), T_m and T_p at best -+ 1: if 0 < best < planes - 1
and the integer den = (T_m - 2 T_0) + T_p > 0, off = float32(T_m - T_p) / float32(2 den), one float32
division, clamped to +-0.5; otherwise off = 0.  In float64, as in the sweep,
    depth = float32(1 / (w_far + (best + off) step))
A pixel is kept iff its RAW cost satisfies C(p, best) <= q(min_score), q the cost formula above
evaluated on the host in float32; a raw cost of 255 is therefore never kept -- smoothness may move a
winner, it may not invent a measurement.  depth is NaN where the pixel is not kept.  Outputs: plane
int32, cost uint8 (the raw C(p, best)), total uint16 (T_0; carried as int16 bits in torch), depth
float32.  dense_check and everything behind it consume depth unchanged.  The volume and the total of a
depth_maps call take 3 h w planes bytes, allocated once and reused for every view.

REFINEMENT RULES (refine(); kernels: csrc/dense_refine.hip and the guided form of csrc/dense_sweep.hip;
restated by tests/dense_refine_restatement.py).  A coarse level's depth map says where the surface is; the
fine level sweeps, per tile, a window of a larger plane set around it.

Fine plane set.  For a view with range (w_far, w_near), T planes uniform in inverse depth:
    step_f = (w_near - w_far) / (T - 1)      z_d = 1 / (w_far + (double)d step_f)     (the sweep's expression)
refine_planes(planes, ratio) = (planes - 1) ratio + 1, so coarse plane k is fine plane k ratio.
2 <= T <= IAMX_DENSE_GUIDED_MAX_PLANES = 65536 (IAMX_DENSE_MAX_PLANES, the plain sweep's, stays 4096).

Window table.  int32 [tiles_y][tiles_x][2] = (first, count) over the sweep's 32 x 16 tiles in row-major
order, tiles_x = ceil(w / 32), tiles_y = ceil(h / 16).  An entry has 0 <= first, 0 <= count and
first + count <= T; anything else is a ValueError on the host and an error of the C entry, without a launch.

Guided sweep.  For pixel p of tile t, S_d(p) is THE RULES' aggregate for first_t <= d < first_t + count_t;
every other plane is not swept: its score is invalid.  Winner, tie rule, around = (s_m, s_0, s_p) and the
float32 offset are THE RULES' with the global d, so s_m is NaN at best = first_t, s_p is NaN at the window's
last plane, and off = 0 there.  depth = float32(1 / (w_far + (best + off) step_f)) in float64.  A pixel is
kept iff best >= 0, s_0 >= min_score, and (the window-edge rule) neither best = first_t with first_t > 0
nor best = first_t + count_t - 1 with first_t + count_t < T: a winner on a rim of its window that is not a
rim of the plane set may be a clipped peak.  plane, score and around are written for every pixel regardless;
a tile with count = 0 writes plane = -1 and NaN everywhere.  With every entry (0, T) and T <= 4096 the four
outputs are the plain sweep's with planes = T, bit for bit.

Guide.  From the coarse depth map Dc [hc][wc] float32 (NaN: none), the fine size (h, w), (w_far, w_near, T),
the radius r and pad >= 0.  For tile (tx, ty), in integers:
    fine columns    x0 = max(32 tx - r, 0), x1 = min(32 tx + 31 + r, w - 1)        rows: 16 and h
    coarse columns  c0 = max(((2 x0 + 1) wc) div (2 w) - 1, 0)
                    c1 = min(((2 x1 + 1) wc) div (2 w) + 1, wc - 1)                 rows: hc and h
(the coarse pixel under the fine pixel's centre, one more either side; the size ratio need not be 2).  Over
the entries of that box that are finite and > 0, in float64 with every operation rounded on its own:
    wv = 1.0 / (double)Dc,  wmin = min wv,  wmax = max wv         (order-free: no reduction order to fix)
    lo = floor((wmin - w_far) / step_f) - pad,  hi = ceil((wmax - w_far) / step_f) + pad
both clamped into [0, T - 1] (floor and ceil are whole numbers; the pad and the clamp are exact in whatever
arithmetic holds them, so a depth far outside the range lands on an end of the set).  The window is
(lo, hi - lo + 1), and (0, 0) for a box without such an entry.  pad defaults to ratio: one coarse step.

refine.  The guide depth of view i is coarse.depth[i] where coarse.keep[i] != 0 and NaN elsewhere -- the
coarse level's consistency check decides what may guide.  The coarse level may be semi-global; the fine
level is winner-take-all inside its windows.  dense_check runs over the fine maps as above.  A view
without a range or neighbours gets an empty map, and so does one whose coarse map kept nothing (every
window is (0, 0)).  Levels chain: a refine()'s result is the `coarse` of the next with planes = T.

Consistency (dense_check), float64.  A pixel of view i with a depth z becomes the NED point
Ri^T (xn z, yn z, z) + Ci (expressions as above).  For each neighbour j it is projected into j
(as above, with j's K): z' = its depth there, (u, v) its pixel; the neighbour agrees iff z' > 0,
rint(u) and rint(v) (half to even) lie inside the image, j's depth map has a depth z_j there and
|z' - z_j| <= eps z'.  The pixel survives with at least min(min_agree, neighbours of i) agreeing
neighbours; a view without neighbours keeps nothing.

Fusion (dense_splat).  The raster frame follows ortho.raster_frame over the surviving points' ENU
bounds (host): x0 = floor(min east / gsd) gsd, y1 = ceil(max north / gsd) gsd,
W = max(1, ceil((max east - x0) / gsd)), H likewise; a point exactly on the east or south bound
falls outside the last cell and is dropped, as every point outside the frame is.  A point lands in
cell (floor((y1 - north) / gsd), floor((east - x0) / gsd)).  Each cell holds an int32 count and an
int64 sum of rint(up 1024), both kept by integer atomics only: the result does not depend on
scheduling.  dsm = float32(sum / 1024 / count) in float64, NaN where count == 0.

ROBUST FUSION RULES (fuse(method='robust'); kernels: csrc/dense_fuse.hip; restated by
tests/dense_fuse_restatement.py).  The mean above lets one wrong depth pull its cell by metres, and gives a
cell that straddles a roof edge a height that exists nowhere.  This rule finds, per cell, the cluster of
heights to average, from fixed-size histograms: one thread per point, integer atomics only.

Parameters.  bins B, 4 .. 64 (IAMX_DENSE_FUSE_MIN_BINS, _MAX_BINS), default 32: histogram bins per cell.
levels L, 1 .. 4 (IAMX_DENSE_FUSE_MAX_LEVELS), default 2.  band, metres, finite and > 0, default 0.5 gsd: the
least bin width, wmin = max(1, rint(band 1024)) computed on the host, at most 2^40.  share, an integer
1 .. 256, default 256: the first level's acceptance in 256ths of the strongest bin.  Anything else is a
ValueError before any device call, and an error of the C entries without a launch.

Frame and accepted points are the mean's: the frame from frame_of, cell = (floor((y1 - north) / gsd),
floor((east - x0) / gsd)) inside the raster, q = rint(up 1024) as int64 accepted iff |q| <= 1e15 (a NaN
fails every test).  count int32 counts a cell's accepted points: the mean's count, bit for bit.

Range.  Per cell lo = min q, hi = max q over its accepted points (signed 64-bit atomic min and max).

Level l = 1 .. L, for every cell with count > 0, all in int64:
    wb = max(wmin, ceil((hi - lo + 1) / B))                     the integer ceiling
    a point takes part iff lo <= q <= hi; its bin is b = (q - lo) div wb, below B by construction
    hist[b] uint32;  s_b = hist[b-1] + hist[b] + hist[b+1], a bin outside 0 .. B-1 counting 0;  smax = max_b s_b
    b* = the HIGHEST b with s_b 256 >= t smax;  t = share at level 1, 256 at every later level
    lo' = max(lo, lo + (b* - 1) wb),  hi' = min(hi, lo + (b* + 2) wb - 1)      both from the OLD lo
    (lo, hi) = (lo', hi')
So level 1 picks the cluster, the highest one at least share/256 as populous as the strongest (a roof over
the ground it hides, for share < 256); later levels centre on that cluster's mode; the higher bin wins a tie.

Sum and resolve.  support int32 = the cell's accepted points with lo <= q <= hi after level L, sum int64 =
the total of their q, dsm = float32(sum / 1024 / support) in float64 (iamx_dense_resolve as it is), NaN
where count == 0; support >= 1 wherever count >= 1.  window int64 [H][W][2] = the final (lo, hi), (0, 0)
for an empty cell.  lo, hi, the histograms, support and sum are each a minimum, a maximum or a count of
integers: the result depends neither on scheduling nor on the order of the points.

Memory: 4 bins + 16 + 4 + 4 + 8 + 4 bytes per cell (hist, window, count, support, sum, dsm); the size is
checked against the device's free memory on the host.  Passes: 2 + L over the points, L over the cells.

Fill (dense_fill) makes the fused DSM hole-free enough to drape frames over.  Round k = 1 .. rounds
reads the raster as round k - 1 left it (ping-pong, nothing is updated in place).  A NaN cell with at
least one finite value among its 8 neighbours becomes the float32 sum of those values divided by
their count: the neighbours are taken in row-major order, cells outside the raster do not exist, the
sum starts at the first finite neighbour, and the quotient is computed in float64 and rounded once
(the correctly rounded float32 quotient).  Finite cells never change.  round_of, uint8 [H, W], is 0
for a measured cell, k for a cell filled in round k and 255 for a cell still empty.  rounds is
0 .. 254 (0: nothing is filled); an all-NaN raster is a ValueError; count is carried over unchanged.

The grey plane of a project's frame (views_from_project): the decoded BGR frame through
kernels.resize_area at the sweep scale (cv2's INTER_AREA), then the integer luma
Y = (29 B + 150 G + 77 R + 128) >> 8, as float32.  K is scaled with the pixel-centre convention:
sx = w / width, fx' = fx sx, cx' = (cx + 0.5) sx - 0.5, y likewise.
"""
import json
import os
from math import ceil, floor

import numpy as np

from . import _deps
from ._deps import getNode

NEIGHBOUR_RATIO = (0.05, 0.6)          # baseline over median chain depth
RANGE_MARGIN = 0.1
MAX_SIDE = 1 << 20
REGULARIZE = ('none', 'sgm')
FUSIONS = ('mean', 'robust')
SGM_P1, SGM_P2 = 16, 128                 # the defaults of p1 / p2 (the table they come from)


class View(object):
    """One image at the sweep scale (THE RULES).  G and rays numpy or device tensors."""
    __slots__ = ('G', 'K', 'dist', 'R', 'C', 'rays', 'name')

    def __init__(self, G, K, dist, R, C, rays=None, name=None):
        self.G = G
        self.K = np.asarray(K, np.float64).reshape(4)
        self.dist = np.asarray(dist, np.float64).reshape(5)
        self.R = np.asarray(R, np.float64).reshape(3, 3)
        self.C = np.asarray(C, np.float64).reshape(3)
        self.rays = rays
        self.name = name


class DepthMaps(object):
    """depth_maps()'s result, device tensors: plane int32 / score float32 / depth float32 [V, h, w]
    (the sweep's), keep uint8 [V, h, w] (kept and consistent), ned float64 [V, h, w, 3].
    regularize='sgm': plane and depth are the select's, score stays the sweep's winner's, and cost
    uint8 / total int16 [V, h, w] (the raw cost and the summed path cost at the selected plane; 255 and
    0 for a view that was not swept) come with them."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Surface(object):
    """dsm float32 [H, W] (NaN: empty), count int32 [H, W] (device tensors); x0 = west side of
    column 0, y1 = north side of row 0, gsd metres per cell (local ENU about ned_reference).
    fuse(method='robust'): support int32 [H, W], the points behind each height, and fusion, the dict of
    the mode's parameters that save() writes; both None otherwise."""

    def __init__(self, dsm, count, x0, y1, gsd, support=None, fusion=None):
        self.dsm, self.count, self.x0, self.y1, self.gsd = dsm, count, float(x0), float(y1), float(gsd)
        self.support, self.fusion = support, fusion

    @property
    def shape(self):
        return tuple(self.dsm.shape)


# ---------------------------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------------------------
def pixel_rays(K, dist, h, w):
    """rays [h, w, 2] float64 (device): undistort.undistort_points at the pixel centres, (u - cx) / fx"""
    import torch
    from . import kernels, undistort
    K = np.asarray(K, np.float64).reshape(4)
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    und = undistort.undistort_points(np.stack([u, v], 2).reshape(-1, 2), K, dist).astype(np.float64)
    rays = np.stack([(und[:, 0] - K[2]) / K[0], (und[:, 1] - K[3]) / K[1]], 1).reshape(h, w, 2)
    out = kernels._dev(rays, torch.float64)
    torch.cuda.current_stream().synchronize()
    return out


def scaled_K(K, width, height, w, h):
    """(fx, fy, cx, cy) of a width x height camera for its w x h image, pixel centres kept"""
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.reshape(4)
    sx, sy = w / float(width), h / float(height)
    return np.array([fx * sx, fy * sy, (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5])


def grey_plane(frame, scale):
    """device BGR uint8 [H, W, 3] -> float32 [h, w]: kernels.resize_area, then the integer luma"""
    import torch
    from . import kernels
    small = kernels.resize_area(frame, scale, scale) if scale != 1.0 else frame
    s = small.to(torch.int32)
    return ((29 * s[:, :, 0] + 150 * s[:, :, 1] + 77 * s[:, :, 2] + 128) >> 8).to(torch.float32).contiguous()


def image_pose(image):
    """(R NED -> camera, C) of an image's optimised pose"""
    cam2body = image.get_cam2body() if hasattr(image, 'get_cam2body') else \
        np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=float)
    R = np.linalg.inv(cam2body).dot(np.asarray(image.get_body2ned(opt=True), np.float64).T)
    return R, np.asarray(image.get_camera_pose(opt=True)[0], np.float64)


def group_indices(proj, group_list, group_index):
    """the project indices of the group's images, in group order"""
    if not 0 <= group_index < len(group_list):
        raise IndexError("group %d of %d" % (group_index, len(group_list)))
    index = {im.name: i for i, im in enumerate(proj.image_list)}
    return [index[name] for name in group_list[group_index] if name in index]


def views_from_project(proj, group_list, group_index, matches, scale, frames=None):
    """The group's views at `scale` of the camera's size: optimised K, distortion and poses, the grey
    planes from the decoded frames (histogram.frame_pass, in group order; frames=: ready device BGR
    tensors instead).  -> (views, group) with group the images' project indices.  matches is not read
    here: it rides along to choose_neighbours and depth_range."""
    from . import histogram
    camera = _deps.camera()
    K = np.asarray(camera.get_K(optimized=True), np.float64)
    dist = np.array(camera.get_dist_coeffs(optimized=True), np.float64).ravel()[:5]
    width, height = camera.get_image_params()
    group = group_indices(proj, group_list, group_index)
    images = [proj.image_list[i] for i in group]
    planes = []

    def on_frames(batch):
        for frame in batch:
            planes.append(grey_plane(frame, scale))

    if frames is not None:
        on_frames(list(frames))
    else:
        histogram.frame_pass(images, want_hist=False, on_frames=on_frames)
    if len(planes) != len(images):
        raise RuntimeError("%d of %d frames arrived" % (len(planes), len(images)))
    if not planes:
        return [], group
    h, w = planes[0].shape
    Ks = scaled_K(K, width, height, w, h)
    rays = pixel_rays(Ks, dist, h, w)
    views = []
    for im, G in zip(images, planes):
        R, C = image_pose(im)
        views.append(View(G, Ks, dist, R, C, rays=rays, name=im.name))
    return views, group


# ---------------------------------------------------------------------------------------------
# neighbours and depth ranges from the sparse chains (host)
# ---------------------------------------------------------------------------------------------
def _observations(matches, group):
    """the members of the positioned chains that lie in the group -> (chain number, position in
    group, chain NED [n_obs, 3]), one row per (chain, image), an image counted once per chain"""
    pos_of = {int(g): k for k, g in enumerate(group)}
    chain, member, ned = [], [], []
    for c, m in enumerate(matches):
        if m[0] is None:
            continue
        seen = set()
        for p in m[2:]:
            k = pos_of.get(int(p[0]))
            if k is not None and k not in seen:
                seen.add(k)
                chain.append(c)
                member.append(k)
                ned.append(m[0])
    return (np.array(chain, np.int64), np.array(member, np.int64),
            np.array(ned, np.float64).reshape(-1, 3))


def _camera_depth(R, C, X):
    """z of R (X - C), elementwise (no BLAS: the order of the sum is part of the result)"""
    d = X - C
    return (R[2, 0] * d[:, 0] + R[2, 1] * d[:, 1]) + R[2, 2] * d[:, 2]


def choose_neighbours(matches, group, poses, n=4):
    """Per image of the group (project indices; poses[k] = (R, C) of group[k]) the other images
    ranked by the number of positioned chains they share with it (more first, the earlier image on a
    tie), kept only where baseline / (median depth of the shared chains in the image's camera) lies in
    NEIGHBOUR_RATIO, at most n.  -> a list of positions in the group per image."""
    V = len(group)
    if len(poses) != V:
        raise ValueError("one pose per image of the group")
    if n < 1:
        raise ValueError("n is at least 1")
    chain, member, ned = _observations(matches, group)
    out = [[] for _ in range(V)]
    if len(chain) == 0:
        return out
    # every ordered pair (i, j), i != j, of members of one chain
    order = np.argsort(chain, kind='stable')
    chain, member, ned = chain[order], member[order], ned[order]
    start = np.nonzero(np.r_[True, chain[1:] != chain[:-1]])[0]
    length = np.diff(np.r_[start, len(chain)])
    first = np.repeat(start, length)                         # per observation: its chain's first row
    size = np.repeat(length, length)
    a = np.repeat(np.arange(len(chain)), size)               # observation a ...
    b = np.repeat(first, size) + (np.arange(len(a)) - np.repeat(np.cumsum(size) - size, size))   # ... with each b
    sel = a != b
    a, b = a[sel], b[sel]
    i, j = member[a], member[b]
    depth = np.empty(len(a))
    for k in range(V):
        s = i == k
        if s.any():
            depth[s] = _camera_depth(poses[k][0], poses[k][1], ned[a[s]])
    key = i * V + j
    order = np.lexsort((depth, key))
    key, depth = key[order], depth[order]
    start = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0]
    count = np.diff(np.r_[start, len(key)])
    lo, hi = start + (count - 1) // 2, start + count // 2
    median = 0.5 * (depth[lo] + depth[hi])
    pi, pj = key[start] // V, key[start] % V
    Cs = np.array([p[1] for p in poses], np.float64).reshape(V, 3)
    d = Cs[pi] - Cs[pj]
    baseline = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = baseline / median
    ok = (median > 0) & (ratio >= NEIGHBOUR_RATIO[0]) & (ratio <= NEIGHBOUR_RATIO[1])
    for k in range(V):
        s = np.nonzero(ok & (pi == k))[0]
        rank = s[np.lexsort((pj[s], -count[s]))]
        out[k] = [int(x) for x in pj[rank][:n]]
    return out


def depth_range(matches, group, poses):
    """Per image of the group (z_near, z_far): the camera depths of the positioned chains it observes,
    those in front of it, (1 - RANGE_MARGIN) min and (1 + RANGE_MARGIN) max; None without one."""
    V = len(group)
    if len(poses) != V:
        raise ValueError("one pose per image of the group")
    chain, member, ned = _observations(matches, group)
    out = [None] * V
    for k in range(V):
        s = member == k
        if not s.any():
            continue
        z = _camera_depth(poses[k][0], poses[k][1], ned[s])
        z = z[z > 0]
        if len(z):
            out[k] = ((1.0 - RANGE_MARGIN) * float(z.min()), (1.0 + RANGE_MARGIN) * float(z.max()))
    return out


# ---------------------------------------------------------------------------------------------
# depth maps and fusion (device)
# ---------------------------------------------------------------------------------------------
def sgm_max_cost(min_score):
    """q(min_score) of SEMI-GLOBAL RULES: the cost formula in float32 on the host"""
    s = np.float32(min_score)
    if np.isnan(s):
        raise ValueError("min_score is a number")
    c = np.rint((np.float32(1.0) - s) * np.float32(127.0))
    return int(min(max(c, np.float32(0.0)), np.float32(254.0)))


def sgm_parameters(planes, regularize='none', p1=None, p2=None, paths=8, c_invalid=127):
    """the mode and its parameters checked on the host (ValueError) -> None for 'none', else
    (planes, paths, p1, p2, c_invalid) with the defaults filled in"""
    from . import kernels
    if regularize not in REGULARIZE:
        raise ValueError("regularize is one of %s, got %r" % (', '.join(REGULARIZE), regularize))
    if regularize == 'none':
        return None
    return kernels.dense_sgm_check(planes, paths, SGM_P1 if p1 is None else p1, SGM_P2 if p2 is None else p2, c_invalid)


def depth_maps(views, neighbours, ranges, planes=64, radius=3, min_var=4.0, min_score=0.6, eps=0.01,
               min_agree=2, check=True, regularize='none', p1=None, p2=None, paths=8, c_invalid=127):
    """Sweep every view against its neighbours (positions in `views`) over its range (z_near, z_far),
    then the consistency rule over all maps (check=False: every kept pixel survives).  A view without
    neighbours or without a range gets an empty map.  regularize='sgm': SEMI-GLOBAL RULES stand between
    the sweep and the winner (p1 / p2 default to SGM_P1 / SGM_P2, paths 4 or 8, 2 to 64 planes); the
    cost volume and the total, 3 h w planes bytes, are allocated once and reused for every view.
    -> DepthMaps"""
    import torch
    from . import kernels
    views = list(views)
    V = len(views)
    if V == 0:
        raise ValueError("no views")
    if len(neighbours) != V or len(ranges) != V:
        raise ValueError("one neighbour list and one range per view")
    sgm = sgm_parameters(planes, regularize, p1, p2, paths, c_invalid)
    kernels.dense_neighbour_table(neighbours, V)          # (checked before any device call)
    h, w = kernels._dense_size(views)
    for r in ranges:
        if r is not None and not (0.0 < float(r[0]) < float(r[1]) < float('inf')):
            raise ValueError("a range is 0 < z_near < z_far, got %r" % (r,))
    dev = kernels.require_gpu()
    plane = torch.full((V, h, w), -1, dtype=torch.int32, device=dev)
    score = torch.full((V, h, w), float('nan'), dtype=torch.float32, device=dev)
    depth = torch.full((V, h, w), float('nan'), dtype=torch.float32, device=dev)
    around = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    more = {}
    if sgm is not None:
        planes, paths, p1, p2, c_invalid = sgm
        max_cost = sgm_max_cost(min_score)
        volume = torch.empty((h, w, planes), dtype=torch.uint8, device=dev)
        total = torch.empty((h, w, planes), dtype=torch.int16, device=dev)
        wta_plane = torch.empty((h, w), dtype=torch.int32, device=dev)
        wta_depth = torch.empty((h, w), dtype=torch.float32, device=dev)
        more = dict(cost=torch.full((V, h, w), 255, dtype=torch.uint8, device=dev),
                    total=torch.zeros((V, h, w), dtype=torch.int16, device=dev))
    for i, v in enumerate(views):
        if ranges[i] is None or len(neighbours[i]) == 0:
            continue
        w_far, w_near = 1.0 / float(ranges[i][1]), 1.0 / float(ranges[i][0])
        if sgm is None:
            kernels.dense_sweep(v, [views[j] for j in neighbours[i]], w_far, w_near, planes, radius=radius,
                                min_var=min_var, min_score=min_score, out=(plane[i], score[i], depth[i], around))
            continue
        kernels.dense_sweep(v, [views[j] for j in neighbours[i]], w_far, w_near, planes, radius=radius,
                            min_var=min_var, min_score=min_score, out=(wta_plane, score[i], wta_depth, around),
                            volume=volume)
        kernels.dense_sgm_paths(volume, paths, p1, p2, c_invalid, out=(total,))
        kernels.dense_sgm_select(total, volume, w_far, w_near, max_cost,
                                 out=(plane[i], more['cost'][i], more['total'][i], depth[i]))
    keep, ned = kernels.dense_check(depth, views, neighbours, eps=eps, min_agree=min_agree)
    if not check:
        keep = torch.isfinite(depth).to(torch.uint8)
    return DepthMaps(plane=plane, score=score, depth=depth, keep=keep, ned=ned, **more)


def refine_planes(planes, ratio):
    """T of REFINEMENT RULES: the size of the fine plane set whose plane k ratio is coarse plane k"""
    from . import kernels
    planes, ratio = int(planes), int(ratio)
    if planes < 2:
        raise ValueError("a level that is refined has at least 2 planes, got %d" % planes)
    if ratio < 1:
        raise ValueError("ratio is at least 1, got %d" % ratio)
    total = (planes - 1) * ratio + 1
    if total > kernels.DENSE_GUIDED_MAX_PLANES:
        raise ValueError("(%d - 1) %d + 1 = %d planes, above %d" % (planes, ratio, total, kernels.DENSE_GUIDED_MAX_PLANES))
    return total


def refine(views, neighbours, ranges, coarse, planes, ratio=4, pad=None, radius=3, min_var=4.0, min_score=0.6,
           eps=0.01, min_agree=2, check=True):
    """One finer level (REFINEMENT RULES).  views: the fine views, the cameras of the coarse call in its
    order at any larger size; coarse: that call's DepthMaps (depth_maps(), with regularize='sgm' or
    without, or an earlier refine()); planes: its plane count.  Per view the guide turns the coarse
    depths that survived (coarse.keep) into a window per tile of the T = refine_planes(planes, ratio)
    fine planes (pad: planes added either side, default ratio), the guided sweep walks them winner-take-all,
    and the consistency rule runs over the fine maps.  A view without neighbours or a range gets an empty
    map, and so does one whose coarse map kept nothing.  -> DepthMaps with plane (indices in the T planes),
    score, depth, keep, ned, windows int32 [V, tiles_y, tiles_x, 2] and total = T; a valid `coarse`
    of the next level with planes = T."""
    import torch
    from . import kernels
    views = list(views)
    V = len(views)
    if V == 0:
        raise ValueError("no views")
    if len(neighbours) != V or len(ranges) != V:
        raise ValueError("one neighbour list and one range per view")
    total = refine_planes(planes, ratio)
    pad = int(ratio) if pad is None else int(pad)
    if not 0 <= pad <= kernels.DENSE_GUIDED_MAX_PLANES:
        raise ValueError("pad is 0 to %d planes, got %d" % (kernels.DENSE_GUIDED_MAX_PLANES, pad))
    if not 1 <= int(radius) <= kernels.DENSE_MAX_RADIUS:
        raise ValueError("radius is 1 to %d, got %d" % (kernels.DENSE_MAX_RADIUS, radius))
    c_shape, k_shape = tuple(coarse.depth.shape), tuple(coarse.keep.shape)
    if len(c_shape) != 3 or k_shape != c_shape:
        raise ValueError("the coarse level carries depth and keep [V, hc, wc]")
    if c_shape[0] != V:
        raise ValueError("the coarse level has %d views, the fine one %d" % (c_shape[0], V))
    kernels.dense_neighbour_table(neighbours, V)          # (checked before any device call)
    h, w = kernels._dense_size(views)
    for r in ranges:
        if r is not None and not (0.0 < float(r[0]) < float(r[1]) < float('inf')):
            raise ValueError("a range is 0 < z_near < z_far, got %r" % (r,))
    dev = kernels.require_gpu()
    c_depth = kernels._dev(coarse.depth, torch.float32)
    c_keep = kernels._dev(coarse.keep, torch.uint8)
    plane = torch.full((V, h, w), -1, dtype=torch.int32, device=dev)
    score = torch.full((V, h, w), float('nan'), dtype=torch.float32, device=dev)
    depth = torch.full((V, h, w), float('nan'), dtype=torch.float32, device=dev)
    around = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    windows = torch.zeros((V,) + kernels.dense_tiles(h, w) + (2,), dtype=torch.int32, device=dev)
    nan = torch.full(c_shape[1:], float('nan'), dtype=torch.float32, device=dev)
    for i, v in enumerate(views):
        if ranges[i] is None or len(neighbours[i]) == 0:
            continue
        w_far, w_near = 1.0 / float(ranges[i][1]), 1.0 / float(ranges[i][0])
        kernels.dense_guide(torch.where(c_keep[i] != 0, c_depth[i], nan), (h, w), w_far, w_near, total, radius=radius,
                            pad=pad, out=windows[i])
        kernels.dense_sweep_guided(v, [views[j] for j in neighbours[i]], w_far, w_near, total, windows[i], radius=radius,
                                   min_var=min_var, min_score=min_score, out=(plane[i], score[i], depth[i], around))
    keep, ned = kernels.dense_check(depth, views, neighbours, eps=eps, min_agree=min_agree)
    if not check:
        keep = torch.isfinite(depth).to(torch.uint8)
    return DepthMaps(plane=plane, score=score, depth=depth, keep=keep, ned=ned, windows=windows, total=total)


def frame_of(east_min, east_max, north_min, north_max, gsd):
    """ortho.raster_frame's frame for ENU bounds -> (x0, y1, W, H)"""
    gsd = float(gsd)
    if not (gsd > 0.0 and np.isfinite(gsd)):
        raise ValueError("gsd must be a positive number of metres per cell")
    x0 = floor(east_min / gsd) * gsd
    y1 = ceil(north_max / gsd) * gsd
    W = max(1, int(ceil((east_max - x0) / gsd)))
    H = max(1, int(ceil((y1 - north_min) / gsd)))
    if W > MAX_SIDE or H > MAX_SIDE:
        raise ValueError("a %d x %d cell raster: a side above 2^20 cells is refused (gsd %g m)" % (W, H, gsd))
    return x0, y1, W, H


def fusion_parameters(method='mean', bins=32, levels=2, band=None, share=256, gsd=None):
    """the fusion and its parameters checked on the host (ValueError) -> None for 'mean', else the dict
    dense.json carries: fusion, bins, levels, band in metres and share.  band None is 0.5 gsd, and stays
    None where the gsd is not known yet (the command line checks its arguments before there is one)."""
    from . import kernels
    if method not in FUSIONS:
        raise ValueError("method is one of %s, got %r" % (', '.join(FUSIONS), method))
    if method == 'mean':
        return None
    if band is None and gsd is not None:
        band = 0.5 * float(gsd)
    bins, levels, _wmin, share = kernels.dense_fuse_check(bins, levels, 1.0 if band is None else band, share)
    return {'fusion': method, 'bins': bins, 'levels': levels, 'band': None if band is None else float(band), 'share': share}


def fuse(views, depths, gsd, method='mean', bins=32, levels=2, band=None, share=256):
    """The surviving points of depth_maps()'s result into a DSM at `gsd` metres per cell.  method='mean': the
    mean of a cell's points (THE RULES: Fusion); 'robust': ROBUST FUSION RULES with bins, levels, band (None:
    0.5 gsd) and share, the Surface then carries support.  -> Surface"""
    import torch
    from . import kernels
    mode = fusion_parameters(method, bins, levels, band, share, gsd)
    keep = depths.keep.reshape(-1).bool()
    if not bool(keep.any()):
        raise ValueError("no pixel survived: nothing to fuse")
    pts = depths.ned.reshape(-1, 3)[keep]
    lo, hi = pts.amin(dim=0).cpu().numpy(), pts.amax(dim=0).cpu().numpy()
    x0, y1, W, H = frame_of(float(lo[1]), float(hi[1]), float(lo[0]), float(hi[0]), gsd)
    if mode is not None:
        count, support, _total, _window, dsm = kernels.dense_fuse(depths.ned, depths.keep, x0, y1, gsd, W, H, bins=mode['bins'],
                                                                  levels=mode['levels'], band=mode['band'], share=mode['share'])
        return Surface(dsm, count, x0, y1, gsd, support=support, fusion=mode)
    count, _total, dsm = kernels.dense_splat(depths.ned, depths.keep, x0, y1, gsd, W, H)
    return Surface(dsm, count, x0, y1, gsd)


def surface_points(views, depths):
    """the surviving points -> (xyz float32 [n, 3] east, north, up; intensity uint8 [n]) on the host"""
    import torch
    keep = depths.keep.bool()
    ned = depths.ned[keep].cpu().numpy()
    G = torch.stack([v.G if isinstance(v.G, torch.Tensor) else torch.from_numpy(np.asarray(v.G)).to(keep.device)
                     for v in views])
    grey = G[keep].clamp(0, 255).to(torch.uint8).cpu().numpy()
    return np.stack([ned[:, 1], ned[:, 0], -ned[:, 2]], 1).astype(np.float32), grey


def ply_bytes(xyz, intensity):
    """binary little-endian PLY: x, y, z float32 and intensity uchar per vertex"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    intensity = np.asarray(intensity, np.uint8).reshape(-1)
    if len(intensity) != len(xyz):
        raise ValueError("one intensity per point")
    rec = np.empty(len(xyz), dtype=[('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('i', 'u1')])
    rec['x'], rec['y'], rec['z'], rec['i'] = xyz[:, 0], xyz[:, 1], xyz[:, 2], intensity
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar intensity\nend_header\n" % len(xyz))
    return head.encode('ascii') + rec.tobytes()


def save(surface, analysis_dir, points=None, extra=None):
    """<analysis_dir>/dense/dsm.npy (float32, NaN: empty), count.npy (int32), dsm.wld (the world file
    of the raster, local ENU metres, pixel-centre convention), dense.json; points = (xyz, intensity):
    points.ply as well; extra: a dict of further entries of dense.json (the semi-global mode's
    parameters), appended after the others.  A surface with support (fuse(method='robust')): support.npy
    (int32) as well, and dense.json gains points_supporting, fusion, bins, levels, band and share; without
    it the files are the ones written before that mode existed, byte for byte.  -> the json's dict"""
    import io
    from . import ortho, panda3d
    out_dir = os.path.join(analysis_dir, 'dense')
    os.makedirs(out_dir, exist_ok=True)
    H, W = surface.shape
    count = surface.count.cpu().numpy()

    def npy(a):
        buf = io.BytesIO()
        np.save(buf, a)
        return buf.getvalue()

    panda3d._write_atomic(os.path.join(out_dir, 'dsm.npy'), npy(surface.dsm.cpu().numpy()))
    panda3d._write_atomic(os.path.join(out_dir, 'count.npy'), npy(count))
    panda3d._write_atomic(os.path.join(out_dir, 'dsm.wld'),
                          ortho.world_file_text(surface.gsd, surface.x0, surface.y1).encode())
    ref_node = getNode("/config/ned_reference", True)
    info = {'ned_reference': {k: ref_node.getFloat(k) for k in ('lat_deg', 'lon_deg', 'alt_m')},
            'units': 'local ENU metres about ned_reference; dsm is metres up', 'gsd': surface.gsd,
            'width': W, 'height': H, 'cells_filled': int((count > 0).sum()), 'points_fused': int(count.sum()),
            'bounds': {'west': surface.x0, 'east': surface.x0 + W * surface.gsd, 'north': surface.y1,
                       'south': surface.y1 - H * surface.gsd},
            'files': {'dsm': 'dsm.npy', 'count': 'count.npy', 'world_file': 'dsm.wld'}}
    support = getattr(surface, 'support', None)
    if support is not None:
        support = support.cpu().numpy()
        panda3d._write_atomic(os.path.join(out_dir, 'support.npy'), npy(support))
        info['files']['support'] = 'support.npy'
        info['points_supporting'] = int(support.sum())
        info.update(getattr(surface, 'fusion', None) or {'fusion': 'robust'})
    if points is not None:
        panda3d._write_atomic(os.path.join(out_dir, 'points.ply'), ply_bytes(*points))
        info['files']['points'] = 'points.ply'
        info['points'] = int(len(points[0]))
    if extra:
        info.update(extra)
    panda3d._write_atomic(os.path.join(out_dir, 'dense.json'), (json.dumps(info, indent=2) + "\n").encode())
    return info


def load(analysis_dir, device=None):
    """<analysis_dir>/dense/dsm.npy, count.npy and dense.json back into a Surface, the inverse of
    save(); support.npy and the fusion's parameters too where the json names them.  The tensors go to the current HIP device; device=: somewhere else ('cpu': no device
    is needed)."""
    import torch
    out_dir = os.path.join(analysis_dir, 'dense')
    with open(os.path.join(out_dir, 'dense.json')) as f:
        info = json.load(f)
    files = info.get('files', {})
    dsm = np.load(os.path.join(out_dir, files.get('dsm', 'dsm.npy')))
    count = np.load(os.path.join(out_dir, files.get('count', 'count.npy')))
    if dsm.ndim != 2 or dsm.dtype != np.float32 or count.shape != dsm.shape or count.dtype != np.int32:
        raise ValueError("%s: dsm.npy is float32 [H, W] and count.npy int32 of the same shape" % out_dir)
    if dsm.shape != (info['height'], info['width']):
        raise ValueError("%s: dsm.npy is %d x %d cells, dense.json says %d x %d"
                         % (out_dir, dsm.shape[1], dsm.shape[0], info['width'], info['height']))
    support = fusion = None
    if 'support' in files:
        support = np.load(os.path.join(out_dir, files['support']))
        if support.shape != dsm.shape or support.dtype != np.int32:
            raise ValueError("%s: support.npy is int32 of the DSM's shape" % out_dir)
        fusion = {k: info[k] for k in ('fusion', 'bins', 'levels', 'band', 'share') if k in info}
    if device is None:
        from . import kernels
        d, c = kernels._dev(dsm, torch.float32), kernels._dev(count, torch.int32)
        s = kernels._dev(support, torch.int32) if support is not None else None
        torch.cuda.current_stream().synchronize()
    else:
        d, c = torch.from_numpy(dsm).to(device), torch.from_numpy(count).to(device)
        s = torch.from_numpy(support).to(device) if support is not None else None
    return Surface(d, c, info['bounds']['west'], info['bounds']['north'], info['gsd'], support=s, fusion=fusion)


def fill(surface, rounds=8):
    """The fill rule (THE RULES) on a Surface.  -> (Surface with the filled dsm and the same count,
    round_of uint8 [H, W]: 0 measured, k filled in round k, 255 still empty)"""
    import torch
    from . import kernels
    rounds = int(rounds)
    if not 0 <= rounds <= 254:
        raise ValueError("rounds is 0 to 254, got %d" % rounds)
    dsm = surface.dsm if isinstance(surface.dsm, torch.Tensor) else torch.from_numpy(np.asarray(surface.dsm, np.float32))
    if dsm.dim() != 2 or dsm.numel() == 0:
        raise ValueError("a DSM is [H, W]")
    if not bool(torch.isfinite(dsm).any()):
        raise ValueError("the DSM has no measured cell: nothing to fill from")
    filled, round_of = kernels.dense_fill(dsm, rounds)
    return Surface(filled, surface.count, surface.x0, surface.y1, surface.gsd), round_of
