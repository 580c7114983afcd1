"""Shared by tools/gen_terrain_golden.py, tests/test_terrain.py and tests/test_terrain_gpu.py: the
SRTM tiles written from a seed (the goldens store the seeds, not the tiles) and the golden loader."""
import gzip
import os
import pickle
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
_cache = {}


def load(name):
    """tests/golden/terrain_<name>.pkl.gz (read once, shared, not to be changed)"""
    if name not in _cache:
        with gzip.open(os.path.join(GOLD, 'terrain_%s.pkl.gz' % name), 'rb') as f:
            _cache[name] = pickle.load(f)
    return _cache[name]


def tile_words(seed, voids=None):
    """1201 x 1201 uint16 [row][col] (row 0 = the tile's north edge), a relief without any symmetry
    between rows and columns so that a transposed or flipped reading shows.  voids: (row0, row1, col0,
    col1): in that window every 7th cell takes 65535, 10001 or 40000 in turn."""
    rng = np.random.default_rng(seed)
    r = np.arange(1201.0)[:, None]
    c = np.arange(1201.0)[None, :]
    z = 300.0 + 0.11 * r + 0.05 * c + 70.0 * np.sin(r / 97.0 + seed) + 45.0 * np.cos(c / 53.0) + \
        25.0 * np.sin((r + 2.0 * c) / 31.0)
    z = np.round(z + rng.integers(0, 6, (1201, 1201))).astype(np.uint16)
    if voids is not None:
        r0, r1, c0, c1 = voids
        win = z[r0:r1, c0:c1]
        flat = win.reshape(-1).copy()
        flat[::7] = np.resize(np.array([65535, 10001, 40000], np.uint16), len(flat[::7]))
        z[r0:r1, c0:c1] = flat.reshape(win.shape)
    return z


def write_tile(cache_dir, name, seed, voids=None):
    """<cache_dir>/<name>.hgt.zip with the member <name>.hgt: big-endian 16-bit words"""
    path = os.path.join(str(cache_dir), name + '.hgt.zip')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=1) as z:
        z.writestr(name + '.hgt', tile_words(seed, voids).astype('>u2').tobytes())
    return path


# ---- the ray bound: max(16 x the restatement's worst difference from the reference's recorded points,
# measured on the CPU on these goldens, 1e-9 max(1, |ref|)) ------------------------------------------------
CAPPED = 2
MEASURED_WORST = 0.0


def ray_bound(ref):
    return np.maximum(16.0 * MEASURED_WORST, 1e-9 * np.maximum(1.0, np.abs(ref)))


def assert_points(got, ref, flags):
    """non-capped rays within ray_bound, NaN where the reference has NaN"""
    keep = (flags & CAPPED) == 0
    g, r = got[keep], ref[keep]
    assert np.array_equal(np.isnan(g), np.isnan(r))
    ok = ~np.isnan(r)
    assert (np.abs(g[ok] - r[ok]) <= ray_bound(r[ok])).all(), np.abs(g[ok] - r[ok]).max()


# ---- a project of bare poses for the elevation hooks -------------------------------------------------
class _Image(object):
    def __init__(self, name, ned):
        self.name, self.ned = name, ned

    def get_camera_pose(self, opt=False):
        return self.ned, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]


class _Project(object):
    def __init__(self, image_list, analysis_dir):
        self.image_list, self.analysis_dir = image_list, analysis_dir
