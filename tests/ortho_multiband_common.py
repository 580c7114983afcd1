"""Shared by tests/test_ortho_multiband.py and tests/test_ortho_multiband_gpu.py: planted geometry,
the seam and detail scenes, and the restatements' answers (computed once, left read-only)."""
import numpy as np

import ortho_common as oc
import ortho_multiband_restatement as mb
import ortho_restatement as rs

WIDTH, HEIGHT = 960.0, 640.0
GOLDEN_GSD = 3.0               # the recorded 30-image scenes at about 103 x 82 pixels
_cache = {}


def grid(points_px, top):
    """vertices in pixels (x right, y DOWN from the raster's top, which is `top` above y = 0); gsd 1 m"""
    p = np.asarray(points_px, np.float64)
    return np.stack([p[:, 0], top - p[:, 1], np.zeros(len(p))], axis=1)


def uv(S):
    return np.array([[i * WIDTH / S, j * HEIGHT / S] for j in range(S + 1) for i in range(S + 1)])


def lattice(S, x0, y0, x1, y1):
    return [[x0 + (x1 - x0) * i / S, y0 + (y1 - y0) * j / S] for j in range(S + 1) for i in range(S + 1)]


def _freeze(out):
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def restated(key, grids, uvs, frames, gsd, mode, bands=5, width=WIDTH, height=HEIGHT):
    """the restatement's answer for a scene, computed once per key"""
    key = (key, gsd, mode, bands)
    if key not in _cache:
        if mode == 'multiband':
            out = mb.compose(grids, uvs, frames, width, height, gsd, bands)
        else:
            out = rs.compose(grids, uvs, frames, width, height, gsd, mode)
        _cache[key] = _freeze(out)
    return _cache[key]


def golden(scene, mode, bands=5):
    names, grids, guv, width, height = oc.scene_input(scene)
    frames = [oc.hash_frame(k) for k in range(len(grids))]
    return restated(scene, grids, guv, frames, GOLDEN_GSD, mode, bands, width, height)


# ---- two images side by side, 80 x 60 pixels each, 60 columns of overlap; the frames are 60 x 80, so
# every pixel centre of the mosaic (100 x 60) is a texel centre of both ----
PAIR = (grid(lattice(1, 0.0, 0.0, 80.0, 60.0), 60.0), grid(lattice(1, 20.0, 0.0, 100.0, 60.0), 60.0))
OVERLAP = 60
SEAM = 50                      # image 0 owns the columns below it (equal spans: half way between the centres)
ROW = 30


def constant(v):
    return np.full((60, 80, 3), v, np.uint8)


def board(shift):
    """a one-pixel checkerboard, 60 and 180; image 1 starts 20 columns (an even number) to the east,
    so shift 1 puts it one source pixel off image 0's"""
    yy, xx = np.mgrid[0:60, 0:80]
    return np.repeat((60 + 120 * ((xx + yy + shift) & 1)).astype(np.uint8)[:, :, None], 3, axis=2)


SEAM_FRAMES = (constant(100), constant(140))
DETAIL_FRAMES = (board(0), board(1))


def seam_distance():
    """per column, the pixels between it and the seam"""
    cols = np.arange(100)
    return np.where(cols < SEAM, SEAM - 1 - cols, cols - SEAM)


def check_seam(best_bgr, multi_bgr):
    """best steps by the 40 grey levels at the seam; multiband at the default bands shows no
    adjacent step above 20 along the row"""
    step_best = np.abs(np.diff(best_bgr[ROW, :, 0].astype(int)))
    step_multi = np.abs(np.diff(multi_bgr[ROW].astype(int), axis=0))
    print('seam row %d: best steps by %d at column %d, multiband by at most %d'
          % (ROW, step_best.max(), int(step_best.argmax()) + 1, step_multi.max()))
    assert step_best.max() == 40 and int(step_best.argmax()) + 1 == SEAM
    assert step_multi.max() <= 20
    assert (multi_bgr[ROW, :8] == 100).all() and (multi_bgr[ROW, -8:] == 140).all()


def check_detail(best_bgr, multi_bgr, feather_bgr):
    """8 pixels and more from the seam multiband is the winner's pixel within 1 grey level.  Feather
    at t pixels from the seam mixes the two boards with weights (OVERLAP / 2 -+ t) / OVERLAP (its
    border distances), which leaves 2 t / OVERLAP of the amplitude: at most half for
    t <= OVERLAP / 4, so it is looked at on the columns 8 .. OVERLAP / 4 from the seam."""
    t = seam_distance()
    far = t >= 8
    d = np.abs(multi_bgr.astype(int) - best_bgr.astype(int))
    zone = far & (t <= OVERLAP // 4)
    amp_feather = np.abs(feather_bgr[:, zone].astype(int) - 120)
    amp_multi = np.abs(multi_bgr[:, zone].astype(int) - 120)
    print('detail: multiband differs from the winner by at most %d (8 and more from the seam; %d anywhere); '
          'amplitude there of 60: feather at most %d, multiband at least %d'
          % (d[:, far].max(), d.max(), amp_feather.max(), amp_multi.min()))
    assert d[:, far].max() <= 1
    assert amp_feather.max() <= 30 and amp_multi.min() >= 59
