"""WGS-84 NED <-> geodetic conversions with navpy's calling convention, as scripts/lib/srtm.py:164-165,
207-216 uses it: degrees and metres, one point or a list of points in, (lat, lon, alt) / ned out.

When navpy is importable its functions are used.  Otherwise the conversions below (numpy, float64)
stand in: ECEF through the reference point's north / east / down axes, and ECEF -> geodetic by the
fixed-point iteration on the latitude run to convergence.  Parity with navpy is UNPINNED (navpy is
not available to test against); tests/test_terrain.py holds these to a 50-digit evaluation instead."""
import numpy as np

try:
    import navpy as _navpy
except ImportError:
    _navpy = None

WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563
WGS84_E2 = WGS84_F * (2.0 - WGS84_F)


def _points(x):
    """one point [3] or points [N, 3] -> float64 [N, 3] and whether one point came in"""
    x = np.asarray(x, np.float64)
    single = x.ndim == 1
    x = x.reshape(-1, 3)
    return x, single or x.shape[0] == 1


def lla2ecef(lat_deg, lon_deg, alt_m):
    lat, lon = np.radians(lat_deg), np.radians(lon_deg)
    s, c = np.sin(lat), np.cos(lat)
    N = WGS84_A / np.sqrt(1.0 - WGS84_E2 * s * s)
    return np.stack([(N + alt_m) * c * np.cos(lon), (N + alt_m) * c * np.sin(lon),
                     (N * (1.0 - WGS84_E2) + alt_m) * s], axis=-1)


def ecef2lla(ecef):
    """ecef [N, 3] -> lat_deg [N], lon_deg [N], alt_m [N]"""
    x, y, z = ecef[:, 0], ecef[:, 1], ecef[:, 2]
    lon = np.arctan2(y, x)
    p = np.hypot(x, y)
    lat = np.arctan2(z, p * (1.0 - WGS84_E2))
    h = np.zeros_like(p)
    for _ in range(12):          # (contracts by ~e^2 = 0.0067 a round: converged far below one ulp)
        s, c = np.sin(lat), np.cos(lat)
        N = WGS84_A / np.sqrt(1.0 - WGS84_E2 * s * s)
        h = p * c + z * s - WGS84_A * np.sqrt(1.0 - WGS84_E2 * s * s)
        lat = np.arctan2(z, p * (1.0 - WGS84_E2 * N / (N + h)))
    return np.degrees(lat), np.degrees(lon), h


def _ned_axes(lat_ref, lon_ref):
    """rows: the north, east and down unit vectors at the reference, in ECEF"""
    lat, lon = np.radians(lat_ref), np.radians(lon_ref)
    sl, cl, so, co = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    return np.array([[-sl * co, -sl * so, cl],
                     [-so, co, 0.0],
                     [-cl * co, -cl * so, -sl]])


def ned2lla(ned, lat_ref, lon_ref, alt_ref):
    """NED metres about (lat_ref, lon_ref, alt_ref) -> (lat_deg, lon_deg, alt_m), each a scalar for
    one point and an array [N] for a list of points"""
    if _navpy is not None:
        return _navpy.ned2lla(ned, lat_ref, lon_ref, alt_ref)
    ned, single = _points(ned)
    ecef = lla2ecef(lat_ref, lon_ref, alt_ref) + ned.dot(_ned_axes(lat_ref, lon_ref))
    lat, lon, alt = ecef2lla(ecef)
    if single:
        return float(lat[0]), float(lon[0]), float(alt[0])
    return lat, lon, alt


def lla2ned(lat, lon, alt, lat_ref, lon_ref, alt_ref):
    """(lat_deg, lon_deg, alt_m), scalars or arrays [N] -> NED metres about the reference: [3] for one
    point, [N, 3] for a list"""
    if _navpy is not None:
        return _navpy.lla2ned(lat, lon, alt, lat_ref, lon_ref, alt_ref)
    lat, lon, alt = (np.asarray(a, np.float64) for a in (lat, lon, alt))
    single = lat.ndim == 0 or lat.size == 1
    d = lla2ecef(lat.reshape(-1), lon.reshape(-1), alt.reshape(-1)) - lla2ecef(lat_ref, lon_ref, alt_ref)
    ned = d.dot(_ned_axes(lat_ref, lon_ref).T)
    return ned[0] if single else ned
