"""Shared by tests/test_ortho.py and tests/test_ortho_gpu.py: the recorded grids of the Step 5
goldens as rasteriser input, the synthetic hash frames, and the restatement's answers (computed
once per scene, gsd and mode, left read-only)."""
import os

import numpy as np

import ortho_restatement as rs
import step5_common as s5

SCENES = ('step5_mid_default', 'step5_mid_tilted', 'step5_dist_default')
FRAME_H, FRAME_W = 64, 96
_ref = {}
_frames = {}


def golden(scene):
    return s5.load(os.path.join(s5.GOLD, scene + '.pkl.gz'))


def scene_input(scene):
    """-> (names, grids [N][81][3], uv [81][2], width, height) of the golden's first group"""
    g = golden(scene)
    names = list(g['groups'][0])
    grids = np.array([g['images'][n]['grid_list'] for n in names], np.float64)
    uv = np.array(g['images'][names[0]]['distorted_uv'], np.float64)
    return names, grids, uv, g['width'], g['height']


def hash_frame(k, h=FRAME_H, w=FRAME_W):
    """uint8 [h][w][3]: an integer hash of (x, y, channel, k) -- no two neighbours alike, so a
    texel off by one shows"""
    key = (k, h, w)
    if key not in _frames:
        y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64),
                              np.arange(3, dtype=np.uint64), indexing='ij')
        z = (x * 0x9E3779B1 + y * 0x85EBCA77 + c * 0xC2B2AE3D + np.uint64(k + 1) * 0x27D4EB2F) & 0xFFFFFFFF
        z ^= z >> 15
        z = (z * 0x2C1B3C6D) & 0xFFFFFFFF
        z ^= z >> 12
        f = (z & 255).astype(np.uint8)
        f.setflags(write=False)
        _frames[key] = f
    return _frames[key]


def reference(scene, gsd, mode):
    key = (scene, gsd, mode)
    if key not in _ref:
        names, grids, uv, width, height = scene_input(scene)
        out = rs.compose(grids, uv, [hash_frame(k) for k in range(len(grids))], width, height, gsd, mode)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ref[key] = out
    return _ref[key]
