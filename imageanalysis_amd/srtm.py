"""The terrain under the survey: the mirror of scripts/lib/srtm.py, with the reference's names and
module-level state (tile_dict, ned_interp).

    initialize(lla_ref, width_m, height_m, step_m)     srtm.py:150-158   process.py Step 2, 3a, 3c, Step 5
    load_tiles / make_interpolator                     srtm.py:160-254
    ned_interp([n, e]) / ned_interp(array [N, 2])      the RegularGridInterpolator of :254 (host)
    interpolate_vector(ned, v)                         srtm.py:277-314, one ray through the same kernel
    interpolate_vectors(ned, v_list)                   srtm.py:319-324, on the device
    heights(points)                                    ned_interp for a batch, on the device
    intersect(M, ned, uv)                              every ray of every image, on the device
    adopt(interp)                                      any RegularGridInterpolator-like object as the terrain

The tile rules are the reference's as written: <cache_dir>/<tile>.hgt.zip (default /var/tmp), member
<tile>.hgt of 1201 x 1201 big-endian UNSIGNED 16-bit words; 65535 and anything above 10000 become 0
(so negative elevations, which read as large unsigned values, become 0 too); stored as
[col, 1200 - row] over linspace(lon, lon + 1, 1201) x linspace(lat, lat + 1, 1201); linear
interpolation with fill value -32768; every loaded tile overwrites the NED nodes it answers above
-10000, nodes still below -10000 become 0.  All of it vectorised.

Nothing here downloads: a tile that is not in the cache directory raises FileNotFoundError naming
the file to put there."""
import os
import zipfile

import numpy as np

from . import _deps
from .hostlib import geodesy

FILL = -32768.0
default_cache_dir = '/var/tmp'


def _log(*args):
    logger = _deps.logger()
    if logger is not None:
        logger.log(*args)
    else:
        print(*args)


def lla_ll_corner(lat_deg, lon_deg):
    """the south-west corner (whole degrees) of the 1 x 1 degree tile that holds the coordinate"""
    return int(np.floor(lat_deg)), int(np.floor(lon_deg))


def make_tile_name(lat, lon):
    """the tile's base name, hemisphere letters and "%2d" / "%03d" degrees as the reference forms it:
    a latitude below 10 gives a name with a space in it ("N 7E012")"""
    south, west = lla_ll_corner(lat, lon)
    return "%s%2d%s%03d" % ("S" if south < 0 else "N", abs(south), "W" if west < 0 else "E", abs(west))


def _interval(a, x):
    """i with a[i] <= x < a[i + 1], clamped to [0, len(a) - 2] (the last interval closed)"""
    return np.clip(np.searchsorted(a, x, side='right') - 1, 0, len(a) - 2)


class GridInterpolator(object):
    """scipy.interpolate.RegularGridInterpolator((axis0, axis1), values, method='linear',
    bounds_error=False, fill_value=-32768), callable like it, with .grid and .values like it.  The
    host copy answers __call__; the device copy (kernels.Terrain) is made on first use."""

    def __init__(self, axes, values, fill_value=FILL):
        self.grid = tuple(np.ascontiguousarray(a, np.float64) for a in axes)
        self.values = np.ascontiguousarray(values, np.float64)
        self.fill_value = fill_value
        if len(self.grid) != 2 or self.values.shape != (len(self.grid[0]), len(self.grid[1])):
            raise ValueError("two axes and a grid of their lengths")
        for a in self.grid:
            if len(a) < 2 or not np.all(np.diff(a) > 0):
                raise ValueError("an axis is strictly ascending with at least 2 nodes")
        self._device = None

    def __call__(self, xi):
        xi = np.asarray(xi, np.float64)
        shape = xi.shape[:-1]
        xi = xi.reshape(-1, 2)
        a0, a1 = self.grid
        x0, x1 = xi[:, 0], xi[:, 1]
        nans = np.isnan(x0) | np.isnan(x1)
        with np.errstate(invalid='ignore'):
            outside = (x0 < a0[0]) | (x0 > a0[-1]) | (x1 < a1[0]) | (x1 > a1[-1])
        q0 = np.where(nans | outside, a0[0], x0)
        q1 = np.where(nans | outside, a1[0], x1)
        i, j = _interval(a0, q0), _interval(a1, q1)
        y0 = (q0 - a0[i]) / (a0[i + 1] - a0[i])
        y1 = (q1 - a1[j]) / (a1[j + 1] - a1[j])
        v = self.values
        out = v[i, j] * (1.0 - y0) * (1.0 - y1) + v[i, j + 1] * (1.0 - y0) * y1 + \
            v[i + 1, j] * y0 * (1.0 - y1) + v[i + 1, j + 1] * y0 * y1
        out[outside] = self.fill_value
        out[nans] = np.nan
        return out.reshape(shape) if len(shape) else out

    def device(self):
        if self._device is None:
            from . import kernels
            self._device = kernels.Terrain(self.grid[0], self.grid[1], self.values)
        return self._device


class SRTM():
    def __init__(self, lat, lon, dict_path=None):
        self.lat, self.lon = lla_ll_corner(lat, lon)
        self.srtm_cache_dir = default_cache_dir       # unless set otherwise
        self.srtm_z = None
        self.lla_interp = None

    # a persistent place where the .hgt.zip files lie
    def set_srtm_cache_dir(self, srtm_cache_dir):
        if not os.path.exists(srtm_cache_dir):
            _log("SRTM: cache path doesn't exist =", srtm_cache_dir)
        else:
            self.srtm_cache_dir = srtm_cache_dir

    def parse(self):
        tilename = make_tile_name(self.lat, self.lon)
        cache_file = self.srtm_cache_dir + '/' + tilename + '.hgt.zip'
        if not os.path.exists(cache_file):
            raise FileNotFoundError(
                "SRTM tile %s is not in the cache directory: put %s.hgt.zip (holding %s.hgt, 1201 x 1201 "
                "big-endian 16-bit words) at %s -- nothing is downloaded here"
                % (tilename, tilename, tilename, cache_file))
        _log("SRTM: parsing .hgt file:", cache_file)
        with zipfile.ZipFile(cache_file) as z:
            with z.open(tilename + '.hgt', 'r') as f:
                contents = f.read()
        # 1,442,401 (1201x1201) big-endian UNSIGNED 16-bit words, as the reference unpacks them (">...H")
        self.srtm_z = np.frombuffer(contents, dtype='>u2', count=1201 * 1201)
        return True

    def make_lla_interpolator(self):
        _log("SRTM: constructing LLA interpolator")
        z = self.srtm_z.astype(np.float64).reshape(1201, 1201)         # [row][col], row 0 = north
        z[(z == 65535) | (z > 10000)] = 0.0
        srtm_pts = np.ascontiguousarray(z[::-1].T)                     # [col, 1200 - row]
        x = np.linspace(self.lon, self.lon + 1, 1201)
        y = np.linspace(self.lat, self.lat + 1, 1201)
        self.lla_interp = GridInterpolator((x, y), srtm_pts)

    def lla_interpolate(self, point_list):
        return self.lla_interp(point_list)


# The module's state, under the reference's names: the tiles loaded by the last initialize() and the
# NED elevation grid made from them.  The grid is regular in NED metres although the tiles are
# regular in degrees, so an area may span tile edges and corners and every look-up stays a regular
# grid look-up.
tile_dict = {}
ned_interp = None


def initialize(lla_ref, width_m, height_m, step_m):
    """srtm.py:150-158: load the tiles under the area and build the NED grid centred at lla_ref"""
    global tile_dict
    again = len(tile_dict) > 0
    _log("Reinitializing SRTM interpolator which is probably not necessary" if again
         else "Initializing the SRTM interpolator")
    tile_dict = {}
    load_tiles(lla_ref, width_m, height_m)
    make_interpolator(lla_ref, width_m, height_m, step_m)


def load_tiles(lla_ref, width_m, height_m):
    """srtm.py:160-177: every tile between the tiles of the area's south-west and north-east corners,
    latitudes outer, longitudes inner (the order in which make_interpolator lets them overwrite)"""
    _log("SRTM: loading DEM tiles")
    half = np.array([[height_m * 0.5, width_m * 0.5, 0.0]])
    sw = geodesy.ned2lla(-half, lla_ref[0], lla_ref[1], lla_ref[2])
    ne = geodesy.ned2lla(half, lla_ref[0], lla_ref[1], lla_ref[2])
    lat1, lon1 = lla_ll_corner(sw[0], sw[1])
    lat2, lon2 = lla_ll_corner(ne[0], ne[1])
    for lat in range(lat1, lat2 + 1):
        for lon in range(lon1, lon2 + 1):
            tile = SRTM(lat, lon)
            tile.parse()
            tile.make_lla_interpolator()
            tile_dict[make_tile_name(lat, lon)] = tile


def make_interpolator(lla_ref, width_m, height_m, step_m):
    _log("SRTM: constructing NED area interpolator")
    rows = int(height_m / step_m) + 1
    cols = int(width_m / step_m) + 1
    n_list = np.linspace(-height_m * 0.5, height_m * 0.5, rows)
    e_list = np.linspace(-width_m * 0.5, width_m * 0.5, cols)
    # the reference's point list: e outer, n inner, so point (r, c) sits at index (rows * c) + r
    ned_pts = np.zeros((cols * rows, 3))
    ned_pts[:, 0] = np.tile(n_list, cols)
    ned_pts[:, 1] = np.repeat(e_list, rows)
    lat, lon, _alt = geodesy.ned2lla(ned_pts, lla_ref[0], lla_ref[1], lla_ref[2])
    ll_pts = np.stack([np.atleast_1d(lon), np.atleast_1d(lat)], axis=1)

    ned_ds = np.full((rows, cols), FILL)
    # every tile overwrites the nodes it answers (tiles in loading order, as the dict iterates)
    for tile in tile_dict:
        zs = tile_dict[tile].lla_interpolate(ll_pts).reshape(cols, rows).T
        good = zs > -10000
        ned_ds[good] = zs[good]

    # quick sanity check (in the reference's order: rows outer, columns inner)
    for r, c in np.argwhere(ned_ds < -10000):
        _log("Problem interpolating elevation for:", ll_pts[(rows * c) + r].tolist())
        ned_ds[r, c] = 0.0

    global ned_interp
    ned_interp = GridInterpolator((n_list, e_list), ned_ds)


def adopt(interp):
    """Take any RegularGridInterpolator-like object (.grid = (n axis, e axis), .values [rows, cols])
    as the terrain: lib.srtm.ned_interp when the reference's module was initialised by process.py."""
    global ned_interp
    if interp is None:
        raise RuntimeError("the terrain to adopt was never initialised (srtm.initialize)")
    ned_interp = interp if isinstance(interp, GridInterpolator) else GridInterpolator(interp.grid, interp.values)
    return ned_interp


def _terrain():
    if ned_interp is None:
        raise RuntimeError("the terrain was never initialised: call srtm.initialize(lla_ref, width_m, "
                           "height_m, step_m) (or srtm.adopt) first")
    return ned_interp.device()


def heights(points):
    """ned_interp for points [N, 2] (n, e) in one launch -> float64 [N] (numpy)"""
    from . import kernels
    return kernels.terrain_heights(_terrain(), np.asarray(points, np.float64).reshape(-1, 2)).cpu().numpy()


def intersect(M, ned, uv, with_stats=False):
    """Every ray unit(M[i] . [u, v, 1]) of every image against the terrain, with the arguments of
    kernels.surface_grid: M [I, 3, 3], ned [I, 3], uv [n, 2] -> pts float64 [I, n, 3] NED (numpy);
    with_stats also iters uint8 [I, n] and flags uint8 [I, n] (kernels.TERRAIN_*)."""
    from . import kernels
    pts, iters, flags = (x.cpu().numpy() for x in kernels.terrain_rays(_terrain(), M, ned, uv=uv))
    return (pts, iters, flags) if with_stats else pts


def interpolate_vectors(ned, v_list):
    """srtm.py:319-324: the ground points of one camera's rays (vectors already in NED orientation),
    one launch for the list -> list of [n, e, d]"""
    from . import kernels
    v = np.array([np.asarray(x, np.float64).flatten() for x in v_list], np.float64).reshape(1, -1, 3)
    if v.shape[1] == 0:
        return []
    pts, _iters, _flags = kernels.terrain_rays(_terrain(), None, np.asarray(ned, np.float64).reshape(1, 3), v=v)
    return pts.cpu().numpy()[0].tolist()


def interpolate_vector(ned, v):
    """srtm.py:277-314 for one ray: the iteration is csrc/terrain.hip's, the same as for a list"""
    return interpolate_vectors(ned, [v])[0]
