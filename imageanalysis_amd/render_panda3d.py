"""MI355X-native stand-in for the reference's scripts/lib/render_panda3d.py: Step 5, "Create the map".

    build_map(proj, group_list, group_index)                                  render_panda3d.py:80-233

Same effects as the reference: the elevation statistics and per-image z_avg, models/surface.bin, the
Delaunay surface of the optimised points (scipy.spatial.Delaunay on the host: the reference's own
call, so the triangles are identical), image.distorted_uv and image.grid_list for every image of the
group, then panda3d.generate_from_grid (textures and .egg files).

What differs is where the work runs.  The reference casts (grid_steps + 1)^2 rays per image and
intersects each with the surface by a fixed-point iteration of up to 26 single-point
LinearNDInterpolator calls; here all rays of all images of the group are one launch of
kernels.surface_grid (csrc/surface_grid.hip, one thread per ray).  A ray whose walk the kernel would
not answer (step bound, degenerate simplex) is recomputed on the host with scipy and counted in
`grid_stats` -- nothing is silently approximated.  The statistics are computed without a python loop
over observations (np.bincount adds in input order, so the per-image sums are the reference's
sequential float sums bit for bit); pass an array-backed match_cleanup.Chains as `matches` to skip the
matches_grouped pickle altogether.

Not reproduced: intersect2d's `print(" returning high angle nans:", angle)` debug line per culled
ray (the rays are counted in grid_stats['high_angle'] instead).

Use `install(lib.render_panda3d)` to give the reference's module this build_map (drop-in).
"""
import os
import pickle
import time
from math import atan2, pi, sqrt

import numpy as np

from . import _deps, panda3d
from ._deps import getNode

r2d = 180 / pi

# the reference's module switches, names and defaults (render_panda3d.py:18-23)
grid_steps = 8
texture_resolution = 512
use_direct_pose = False
force_ground_elevation_m = None
use_srtm_surface = None
no_extrapolate = False
SWITCHES = ('grid_steps', 'texture_resolution', 'use_direct_pose', 'force_ground_elevation_m',
            'use_srtm_surface', 'no_extrapolate')
_switch_module = None           # install(): the reference's module, where its scripts set the switches


def switches():
    """the six switches as build_map reads them: this module's, or after install() the reference
    module's own (scripts set `render_panda3d.<switch> = ...` on the module they imported)"""
    import sys
    src = _switch_module if _switch_module is not None else sys.modules[__name__]
    return {k: getattr(src, k) for k in SWITCHES}


# the bound on the records one look-up's walk may read before the ray goes to the host (0: the
# kernel's own, the number of triangles + 16).  Not one of the reference's switches.
max_walk_steps = 0

# the last build_map call: rays cast, rays by flag, rays recomputed on the host (fallback), look-ups
# and records read by the walks (steps / lookups = steps per look-up), seconds per stage, and
# `rounds`, the iteration rounds of every ray (int32 [images, rays]; None before the first grid and
# in the SRTM mode)
grid_stats = {'images': 0, 'rays': 0, 'sky': 0, 'high_angle': 0, 'fallback': 0, 'lookups': 0, 'steps': 0,
              'triangles': 0, 'rounds': None,
              'stage_s': {'stats': 0.0, 'delaunay': 0.0, 'transform': 0.0, 'seed': 0.0, 'upload': 0.0,
                          'poses': 0.0, 'kernel': 0.0, 'download': 0.0, 'lists': 0.0}}
# the last interpolate() call: queries, and those recomputed on the host
interp_stats = {'queries': 0, 'fallback': 0}


def _log(*a):
    _deps.logger().log(*a)


def redistort(uv_list, K, dist_coeffs):
    """project.ProjectMgr.redistort (project.py:300-329) on numpy float64 SCALARS, operation by
    operation and in the reference's order -- `x**2`, `r2**2` and `r2**3` stay powers -- so the
    result is the reference's bit for bit (the same scalar routines run in the same order; an array
    form would send the powers through numpy's vector loops, which need not round the same way)."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3 = dist_coeffs
    out = []
    for pt in uv_list:
        x = (pt[0] - cx) / fx
        y = (pt[1] - cy) / fy
        r2 = x**2 + y**2
        r4, r6 = r2**2, r2**3
        dx = 2*p1*x*y + p2*(r2 + 2*x*x)
        dy = p1*(r2 + 2*y*y) + 2*p2*x*y
        Lr = 1.0 + k1*r2 + k2*r4 + k3*r6
        ud = Lr*x + dx
        vd = Lr*y + dy
        out.append([ud * fx + cx, vd * fy + cy])
    return out


def pixel_grid(width, height, steps):
    """the (steps + 1)^2 pixel grid of build_map, v outer, u inner (render_panda3d.py:172-179)"""
    u_list = np.linspace(0, width, steps + 1)
    v_list = np.linspace(0, height, steps + 1)
    return [[u, v] for v in v_list for u in u_list]


def elevation_stats(proj, group, group_index, matches):
    """render_panda3d.py:90-132,148-153: avg / std of the group's points, the 10 std filter, per image
    sum_values / sum_count / min_z / max_z / z_avg, and the surface's points and values.
    `matches`: the loaded matches_grouped (lists), or an untouched match_cleanup.Chains.
    -> (raw_points, raw_values) as the reference's plain lists."""
    from .match_cleanup import Chains
    images = proj.image_list
    arrays = isinstance(matches, Chains) and matches.untouched()
    _log("Computing stats...")
    if arrays:
        rows = np.nonzero(matches.group == group_index)[0]
        ned = np.where(matches.has_ned[rows, None], matches.ned[rows], np.nan)
        ptr, img = matches.ptr, matches.img
    else:
        rows = [m for m in matches if m[1] == group_index]
        ned_list = [m[0] for m in rows]
        ned = np.array(ned_list)
    avg = -np.mean(np.array(ned)[:, 2])
    std = np.std(np.array(ned)[:, 2])
    _log("Average elevation: %.2f" % avg)
    _log("Standard deviation: %.2f" % std)

    _log('Reading feature locations from optimized match points ...')
    keep = np.abs(-ned[:, 2] - avg) < 10*std
    for k in np.nonzero(~keep)[0]:
        if arrays:
            c = int(rows[k])
            a, b = int(ptr[c]), int(ptr[c + 1])
            match = [matches.ned[c].tolist() if matches.has_ned[c] else None, int(matches.group[c])] + \
                [[i, p] for i, p in zip(img[a:b].tolist(), matches.uv[a:b].tolist())]
        else:
            match = rows[k]
        _log("Discarding match with excessive altitude:", match)
    if arrays:
        kept = rows[keep]
        raw_points = ned[keep][:, [1, 0]].tolist()
        raw_values = ned[keep][:, 2].tolist()
        counts = ptr[kept + 1] - ptr[kept]
        first = np.repeat(ptr[kept] - np.concatenate([[0], np.cumsum(counts)[:-1]]), counts)
        obs = first + np.arange(int(counts.sum()))
        obs_img = img[obs].astype(np.int64)
        obs_z = np.repeat(-ned[keep][:, 2], counts)
    else:
        kept_rows = [m for m, k in zip(rows, keep.tolist()) if k]
        raw_points = [[m[0][1], m[0][0]] for m in kept_rows]
        raw_values = [m[0][2] for m in kept_rows]
        counts = np.array([len(m) - 2 for m in kept_rows], np.int64)
        obs_img = np.array([p[0] for m in kept_rows for p in m[2:]], np.int64)
        obs_z = np.repeat(np.array([-m[0][2] for m in kept_rows], np.float64), counts)
    in_group = np.zeros(len(images), bool)
    names = set(group)
    for i, im in enumerate(images):
        in_group[i] = im.name in names
    sel = in_group[obs_img] if len(obs_img) else np.zeros(0, bool)
    obs_img, obs_z = obs_img[sel], obs_z[sel]
    n = len(images)
    # (np.bincount adds its weights in input order: the reference's `sum_values += z`, bit for bit)
    sum_values = np.bincount(obs_img, weights=obs_z, minlength=n)
    sum_count = np.bincount(obs_img, minlength=n)
    min_z = np.full(n, 9999.0)
    max_z = np.full(n, -9999.0)
    np.minimum.at(min_z, obs_img, obs_z)
    np.maximum.at(max_z, obs_img, obs_z)
    for i, im in enumerate(images):
        im.sum_values = float(sum_values[i])
        im.sum_count = float(sum_count[i])
        im.min_z = float(min_z[i])
        im.max_z = float(max_z[i])
        im.z_avg = im.sum_values / float(im.sum_count) if im.sum_count > 0 else 0
    return raw_points, raw_values


def save_surface(analysis_dir, raw_points, raw_values):
    """models/surface.bin: the surface definition as a separate file (render_panda3d.py:134-141)"""
    models_dir = os.path.join(analysis_dir, 'models')
    if not os.path.exists(models_dir):
        _log("Notice: creating models directory =", models_dir)
        os.makedirs(models_dir)
    surface = {'points': raw_points, 'values': raw_values}
    with open(os.path.join(analysis_dir, 'models', 'surface.bin'), "wb") as f:
        pickle.dump(surface, f)


def intersect2d_host(interp, ned, v, avg_ground, no_extrapolate=False):
    """render_panda3d.intersect2d on the host, a scipy call per look-up (the fallback of a ray the
    kernel did not answer; the loop form tools/step5_grid_rate.py times) -> (point, rounds)"""
    p = list(ned)
    if v[2] <= 0.0:
        return p, 0
    tmp = interp([p[1], p[0]])[0]
    surface = tmp if (no_extrapolate or not np.isnan(tmp)) else avg_ground
    error = abs(p[2] - surface)
    count = 0
    while error > 0.01 and count < 25:
        d_proj = -(ned[2] - surface)
        factor = d_proj / v[2]
        p = [ned[0] + v[0] * factor, ned[1] + v[1] * factor, ned[2] + d_proj]
        tmp = interp([p[1], p[0]])[0]
        if no_extrapolate or not np.isnan(tmp):
            surface = tmp
        error = abs(p[2] - surface)
        count += 1
    dy, dx, dz = ned[0] - p[0], ned[1] - p[1], ned[2] - p[2]
    if atan2(-dz, sqrt(dx*dx + dy*dy)) * r2d < 30:
        return [np.nan, np.nan, np.nan], count
    return p, count


def unit_rays(M, grid):
    """project.projectVectors for one image on the host: unit(M . [u, v, 1])"""
    out = []
    for uv in grid:
        proj = M.dot(np.array([uv[0], uv[1], 1.0]))
        out.append(proj / sqrt(np.dot(proj, proj)))
    return out


def interpolate(tri, values, xy, max_steps=0, stats=None):
    """LinearNDInterpolator(tri, values)(xy) through kernels.surface_interp; queries the kernel flags
    (step bound, degenerate simplex) are recomputed with scipy and counted in `interp_stats`.
    -> z float64 [N] (numpy), NaN outside the hull"""
    from . import kernels
    st = stats if stats is not None else interp_stats
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    z, flags = (x.cpu().numpy() for x in kernels.surface_interp(kernels.Surface(tri, values), xy, max_steps=max_steps))
    bad = np.nonzero(flags)[0]
    st['queries'], st['fallback'] = len(xy), len(bad)
    if len(bad):
        import scipy.interpolate
        z[bad] = scipy.interpolate.LinearNDInterpolator(tri, values)(xy[bad])
    return z


def surface_grids(tri, values, M, ned, avg_ground, grid, no_extrapolate=False, ground_m=None, stats=None,
                  max_steps=0):
    """All rays of all images against the surface on the device; rays the kernel flags are
    recomputed with scipy.  tri None: the ground-plane mode.  -> pts float64 [I, n, 3] NED (numpy);
    stats['rounds'] holds every ray's iteration rounds"""
    import torch
    from . import kernels
    st = stats if stats is not None else grid_stats
    stage = st['stage_s']
    clock = time.perf_counter
    uv = np.array(grid, np.float64).reshape(-1, 2)
    surface = None
    if tri is not None:
        t = clock()
        tri.transform           # (scipy computes it on first access; find_simplex below needs it)
        stage['transform'] += clock() - t
        t = clock()
        surface = kernels.Surface(tri, values)
        stage['upload'] += surface.upload_s
        stage['seed'] += clock() - t - surface.upload_s
        st['triangles'] = surface.T
    t = clock()
    pts, rounds, flags, steps = kernels.surface_grid(
        surface, M, ned, avg_ground, uv, no_extrapolate=no_extrapolate,
        ground_m=ground_m if tri is None else None, max_steps=max_steps, with_steps=True)
    torch.cuda.current_stream().synchronize()
    stage['kernel'] += clock() - t
    t = clock()
    pts, rounds, flags, steps = (x.cpu().numpy() for x in (pts, rounds, flags, steps))
    stage['download'] += clock() - t
    st['images'], st['rays'] = int(flags.shape[0]), int(flags.size)
    st['sky'] = int(np.count_nonzero(flags & kernels.SURFACE_SKY))
    st['high_angle'] = int(np.count_nonzero(flags & kernels.SURFACE_HIGH_ANGLE))
    bad = np.argwhere(flags & kernels.SURFACE_FALLBACK)
    st['fallback'] = len(bad)
    st['steps'] = int(steps.sum(dtype=np.int64))
    if len(bad):
        import scipy.interpolate
        interp = scipy.interpolate.LinearNDInterpolator(tri, values)
        Mh, nh, ah = np.asarray(M).reshape(-1, 3, 3), np.asarray(ned).reshape(-1, 3), np.asarray(avg_ground)
        for i, k in bad.tolist():
            v = unit_rays(Mh[i], [uv[k]])[0]
            pts[i, k], rounds[i, k] = intersect2d_host(interp, nh[i].tolist(), v, float(ah[i]), no_extrapolate)
    # (after the recompute: a ray's look-ups are one in front of the loop and one per round)
    st['lookups'] = 0 if tri is None else int((rounds.astype(np.int64) + 1)[(flags & kernels.SURFACE_SKY) == 0].sum())
    st['rounds'] = rounds
    return pts


def map_grids(proj, group, raw_points, raw_values, sw=None, ref=None):
    """build_map between the statistics and the egg files (render_panda3d.py:143-228): the Delaunay
    surface of (raw_points, raw_values), the pixel grid and its distorted twin, every ray of every
    image of `group` against the surface, and image.distorted_uv / image.grid_list (ENU) for each.
    sw: switches(); ref: the NED reference [lat, lon, alt], read in the SRTM mode only.  Needs
    image.z_avg (elevation_stats).  -> the group's images.  ortho.render takes its grids from here,
    so a mosaic and the .egg files of one project show the same polygons."""
    import scipy.spatial
    camera = _deps.camera()
    if sw is None:
        sw = switches()
    clock = time.perf_counter
    stage = grid_stats['stage_s']
    ground = bool(sw['force_ground_elevation_m'])
    srtm_mode = not ground and bool(sw['use_srtm_surface'])
    _log('Generating Delaunay mesh and interpolator ...')
    tri = None
    if not ground and not srtm_mode:        # (the reference builds it in every mode and reads it in this one)
        t = clock()
        tri = scipy.spatial.Delaunay(np.array(raw_points))
        stage['delaunay'] = clock() - t

    # the pixel grid and its distorted twin: the same for every image of the group
    t = clock()
    width, height = camera.get_image_params()
    K = camera.get_K(optimized=True)
    IK = np.linalg.inv(K)
    grid = pixel_grid(width, height, sw['grid_steps'])
    distorted_uv = redistort(grid, K, camera.get_dist_coeffs(True))
    images = [proj.findImageByName(name) for name in group]
    M = np.empty((len(images), 3, 3))
    ned = np.empty((len(images), 3))
    avg_ground = np.empty(len(images))
    for i, image in enumerate(images):
        opt = not sw['use_direct_pose']
        # (left to right, as project.projectVectors multiplies)
        M[i] = image.get_body2ned(opt=True).dot(image.get_cam2body()).dot(IK) if opt else \
            image.get_body2ned().dot(image.get_cam2body()).dot(IK)
        ned[i] = image.get_camera_pose(opt=True)[0] if opt else image.get_camera_pose()[0]
        avg_ground[i] = -image.z_avg
    stage['poses'] = clock() - t

    if srtm_mode:
        # SRTM ground interpolator, as smart.update_srtm_elevations reaches it: lib.srtm's terrain is
        # adopted inside the reference environment, else the mirror builds its own; then every ray of
        # every image in one launch (csrc/terrain.hip)
        from . import srtm as terrain
        srtm = _deps.srtm()
        srtm.initialize(ref, 6000, 6000, 30)
        if srtm is not terrain:
            terrain.adopt(srtm.ned_interp)
        t = clock()
        pts = terrain.intersect(M, ned, np.array(grid, np.float64).reshape(-1, 2))
        stage['kernel'] += clock() - t
    else:
        pts = surface_grids(tri, raw_values, M, ned, avg_ground, grid, no_extrapolate=sw['no_extrapolate'],
                            ground_m=sw['force_ground_elevation_m'] if ground else None,
                            max_steps=max_walk_steps)

    # convert ned to xyz and stash the result for each image
    t = clock()
    enu = np.stack([pts[:, :, 1], pts[:, :, 0], -pts[:, :, 2]], axis=-1)
    for i, image in enumerate(images):
        _log(image.name, image.z_avg)
        image.distorted_uv = distorted_uv
        image.grid_list = enu[i].tolist()
    stage['lists'] = clock() - t
    return images


def build_map(proj, group_list, group_index, matches=None):
    """The reference's build_map.  `matches` (optional, not in the reference's signature): the
    matches_grouped structure already in memory -- an array-backed match_cleanup.Chains is read
    through its arrays -- instead of <analysis_dir>/matches_grouped."""
    sw = switches()
    clock = time.perf_counter
    stage = grid_stats['stage_s']
    for k in stage:
        stage[k] = 0.0
    grid_stats.update(images=0, rays=0, sky=0, high_angle=0, fallback=0, lookups=0, steps=0, triangles=0,
                      rounds=None)
    # lookup ned reference
    ref_node = getNode("/config/ned_reference", True)
    ref = [ref_node.getFloat('lat_deg'), ref_node.getFloat('lon_deg'), ref_node.getFloat('alt_m')]

    _log("Loading optimized match points ...")
    if matches is None:
        with open(os.path.join(proj.analysis_dir, "matches_grouped"), "rb") as f:
            matches = pickle.load(f)
    group = group_list[group_index]

    t = clock()
    raw_points, raw_values = elevation_stats(proj, group, group_index, matches)
    stage['stats'] = clock() - t

    save_surface(proj.analysis_dir, raw_points, raw_values)

    map_grids(proj, group, raw_points, raw_values, sw, ref)

    # generate the panda3d egg models
    dir_node = getNode('/config/directories', True)
    img_src_dir = dir_node.getString('images_source')
    panda3d.generate_from_grid(proj, group_list[group_index], src_dir=img_src_dir,
                               analysis_dir=proj.analysis_dir, resolution=sw['texture_resolution'])


def install(ref_render_module):
    """Give the reference's lib.render_panda3d the device build_map (drop-in).  From then on the
    switches are read from THAT module, where the reference's scripts set them."""
    global _switch_module
    ref_render_module.build_map = build_map
    _switch_module = ref_render_module if all(hasattr(ref_render_module, k) for k in SWITCHES) else None
