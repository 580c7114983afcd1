"""CPU: the host half of the orthomosaic (imageanalysis_amd/ortho.py) against the numpy restatement
of its rules (tests/ortho_restatement.py) on the recorded Step 5 grids, the restatement's own
properties, the tile / world file / ortho.json writer, the C ABI's argument checks and map_grids.
The rasteriser itself is held to the restatement in test_ortho_gpu.py."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest

import ortho_common as oc
import ortho_restatement as rs
import step5_common as s5


@pytest.mark.parametrize('gsd', [0.5, 0.25])
@pytest.mark.parametrize('scene', oc.SCENES)
def test_raster_frame_equals_the_restatement(scene, gsd):
    from imageanalysis_amd import ortho
    _names, grids, _uv, _w, _h = oc.scene_input(scene)
    got, want = ortho.raster_frame(grids, gsd), rs.raster_frame(grids, gsd)
    assert (got.x0, got.y1, got.W, got.H, got.S) == (want['x0'], want['y1'], want['W'], want['H'], want['S'])
    assert got.X.dtype == np.int32 and got.X.tobytes() == want['X'].tobytes()
    assert got.Y.dtype == np.int32 and got.Y.tobytes() == want['Y'].tobytes()
    assert got.used.tobytes() == want['used'].tobytes()
    assert 0 <= got.X.min() and got.X.max() <= 256 * got.W and 0 <= got.Y.min() and got.Y.max() <= 256 * got.H
    if gsd == 0.5 and scene == 'step5_mid_default':
        assert (got.W, got.H) == (617, 492)
    if gsd == 0.5 and scene == 'step5_mid_tilted':
        # 660 x 706 over every finite vertex; one finite vertex there belongs to no used cell, and the
        # frame is over the USED vertices, which end 19 rows further north
        assert got.W == 660 and got.H < 706


def test_raster_frame_refusals():
    from imageanalysis_amd import ortho
    _names, grids, _uv, _w, _h = oc.scene_input('step5_mid_default')
    with pytest.raises(ValueError, match='2\\^20'):
        ortho.raster_frame(grids, 1e-4)
    with pytest.raises(ValueError):
        ortho.raster_frame(grids, 0.0)
    with pytest.raises(ValueError, match='nothing to rasterise'):
        ortho.raster_frame(np.full((2, 81, 3), np.nan), 0.5)
    with pytest.raises(ValueError):
        ortho.raster_frame(np.zeros((2, 80, 3)), 0.5)


@pytest.mark.parametrize('scene', oc.SCENES)
def test_restatement_properties_on_the_golden_scenes(scene):
    """no pixel covered twice by one image, the all-sky image covers nothing, and no pixel's winner
    sits on a decision: the smallest relative gap to the runner-up's metric is at least 1e-9"""
    ref = oc.reference(scene, 0.5, 'best')
    print('%s: %d x %d, up to %d images over a pixel, smallest relative metric gap %.3g'
          % (scene, ref['frame']['W'], ref['frame']['H'], int(ref['count'].max()), ref['gap']))
    assert max(ref['times_max']) == 1 and min(ref['times_max']) in (0, 1)
    assert ref['gap'] >= 1e-9
    assert (ref['index'] >= 0).sum() == (ref['count'] > 0).sum() > 0
    names, grids, _uv, _w, _h = oc.scene_input(scene)
    assert len(names) == (12 if scene == 'step5_dist_default' else 30) and ref['count'].max() <= len(names)
    if scene == 'step5_mid_tilted':
        assert np.isnan(grids).any(axis=2).sum() == 127
        rf = ref['frame']
        flat = []
        for k, g in enumerate(grids):
            cells, _v = rs.used_cells(g)
            tris = rs.triangles(rf['S'], cells)
            X, Y = rf['X'][k].astype(np.int64), rf['Y'][k].astype(np.int64)
            if tris and all((X[b] - X[a]) * (Y[c] - Y[a]) == (Y[b] - Y[a]) * (X[c] - X[a]) for a, b, c in tris):
                flat.append((k, len(tris)))
        assert flat == [(flat[0][0], 128)]                  # every ray "sky": the camera position 81 times
        assert ref['times_max'][flat[0][0]] == 0 and not (ref['index'] == flat[0][0]).any()


def test_restatement_planted_quads_are_watertight():
    """a 2 x 2 mesh with corners on pixel centres in all four vertex orders, and 300 jittered ones:
    no centre is covered twice, and the planted outline's 4 x 4 centres exactly once"""
    rng = np.random.default_rng(5)
    base = np.array([[x, y] for y in (0, 2, 4) for x in (0, 2, 4)], np.float64) * 256 + 128
    orders = [np.arange(9), np.arange(9).reshape(3, 3)[::-1].reshape(-1), np.arange(9).reshape(3, 3)[:, ::-1].reshape(-1),
              np.arange(9).reshape(3, 3).T.reshape(-1)]
    cells = np.ones((2, 2), bool)
    for o in orders:
        p = base[o].astype(np.int32)
        _own, times, _abc, _wk = rs.cover(p[:, 0], p[:, 1], 2, cells, 6, 6)
        assert times.max() == 1 and times.sum() == 16, o      # 4 x 4 centres, the top-left rule's share
    for _ in range(300):
        p = (base + rng.integers(-100, 101, base.shape)).astype(np.int32)      # (0.39 pixel: no triangle can flip)
        _own, times, _abc, _wk = rs.cover(p[:, 0], p[:, 1], 2, cells, 6, 6)
        assert times.max() <= 1


class _HostMosaic(object):
    def __init__(self, bgr, x0, y1, gsd, names):
        import torch
        self.bgr = torch.from_numpy(bgr)
        self.index = self.count = None
        self.x0, self.y1, self.gsd, self.mode, self.names = x0, y1, gsd, 'best', names
        self.shape = bgr.shape[:2]


@pytest.mark.parametrize('fmt', ['png', 'jpg'])
def test_save_round_trip_with_ragged_tiles(tmp_path, fmt):
    from PIL import Image as PILImage
    from imageanalysis_amd import ortho
    from imageanalysis_amd._deps import getNode
    ref = getNode('/config/ned_reference', True)
    ref.setFloat('lat_deg', 44.5)
    ref.setFloat('lon_deg', -93.25)
    ref.setFloat('alt_m', 278.0)
    bgr = oc.hash_frame(3, 70, 100).copy()
    m = _HostMosaic(bgr, -12.5, 40.0, 0.25, ['a.JPG', 'b.JPG'])
    info = ortho.save(m, str(tmp_path), tile=32, fmt=fmt)
    out = tmp_path / 'ortho'
    assert json.loads((out / 'ortho.json').read_text()) == info
    assert info['ned_reference'] == {'lat_deg': 44.5, 'lon_deg': -93.25, 'alt_m': 278.0}
    assert (info['gsd'], info['mode'], info['width'], info['height']) == (0.25, 'best', 100, 70)
    assert info['bounds'] == {'west': -12.5, 'east': 12.5, 'north': 40.0, 'south': 22.5}
    assert info['images'] == ['a.JPG', 'b.JPG'] and len(info['tiles']) == 3 * 4
    assert sorted(os.listdir(str(out))) == sorted([t['file'] for t in info['tiles']]
                                                  + [t['world_file'] for t in info['tiles']] + ['ortho.json'])
    back = np.zeros_like(bgr)
    seen = np.zeros(bgr.shape[:2], int)
    for t in info['tiles']:
        a, rot0, rot1, e, cx, cy = [float(l) for l in (out / t['world_file']).read_text().split()]
        assert (a, rot0, rot1, e) == (0.25, 0.0, 0.0, -0.25)
        c0, r0 = (cx - 0.5 * a - m.x0) / a, (m.y1 - (cy - 0.5 * e)) / a        # centre of the upper-left pixel
        assert c0 == t['col'] * 32 and r0 == t['row'] * 32
        assert (t['west'], t['north']) == (m.x0 + c0 * a, m.y1 - r0 * a)
        assert (t['east'], t['south']) == (t['west'] + t['width'] * a, t['north'] - t['height'] * a)
        with PILImage.open(str(out / t['file'])) as im:
            px = np.asarray(im.convert('RGB'))[:, :, ::-1]
        assert px.shape == (t['height'], t['width'], 3)
        assert t['width'] == (32 if t['col'] < 3 else 4) and t['height'] == (32 if t['row'] < 2 else 6)
        r0, c0 = int(r0), int(c0)
        back[r0:r0 + t['height'], c0:c0 + t['width']] = px
        seen[r0:r0 + t['height'], c0:c0 + t['width']] += 1
    assert (seen == 1).all()
    if fmt == 'png':
        assert back.tobytes() == bgr.tobytes()
    with pytest.raises(ValueError):
        ortho.save(m, str(tmp_path), tile=0)


def test_prefilter_factor_and_pixel_box():
    from imageanalysis_amd import ortho
    S = 2
    xy = np.array([[x, y, 5.0] for y in (20.0, 10.0, 0.0) for x in (0.0, 15.0, 30.0)])
    cells, verts = ortho.used_cells(xy[None])
    assert cells.all() and verts.all() and cells.shape == (1, S, S)
    assert ortho.native_gsd(xy, cells[0], 300, 200) == 0.1                     # 30 m x 20 m over 300 x 200
    assert ortho.prefilter_factor(xy, cells[0], 300, 200, 0.4) == 0.25
    assert ortho.prefilter_factor(xy, cells[0], 300, 200, 0.05) == 1.0
    xy[0] = np.nan                                                             # one cell leaves
    cells, verts = ortho.used_cells(xy[None])
    assert cells.sum() == 3 and verts.sum() == 8
    assert ortho.native_gsd(xy, cells[0], 300, 200) == np.sqrt(450.0 / 60000.0)
    rf = ortho.raster_frame(xy[None], 1.0)
    assert (rf.x0, rf.y1, rf.W, rf.H) == (0.0, 20.0, 30, 20) and rf.X[0, 0] == 0 and rf.Y[0, 0] == 0
    assert ortho.pixel_box(rf.X[0], rf.Y[0], verts[0], rf.W, rf.H) == (0, 0, 29, 19)
    assert ortho.pixel_box(rf.X[0], rf.Y[0], np.zeros(9, bool), rf.W, rf.H) == (0, 0, -1, -1)
    assert ortho.image_terms(xy, verts[0]) == rs.image_terms(xy, verts[0].reshape(-1))


def test_argument_checks_do_not_need_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(256)          # never dereferenced: the checks come before the launch
    odd = ctypes.c_void_p(8)
    par = (ctypes.c_double * 8)(5472, 3648, 0.0, 10.0, 0.5, 1.0, 2.0, 3.0)
    assert L.iamx_ortho_max_steps() == 32
    assert L.iamx_ortho_clear(0, 4, 4, None, one, one, one, None) == -1 and b'null pointer' in L.iamx_last_error()
    assert L.iamx_ortho_clear(0, 4, 4, one, None, one, one, None) == -1              # best needs the index
    assert L.iamx_ortho_clear(2, 4, 4, one, one, one, one, None) == -1 and b'mode' in L.iamx_last_error()
    assert L.iamx_ortho_clear(0, 0, 4, one, one, one, one, None) == -1
    assert L.iamx_ortho_clear(0, 4, (1 << 20) + 1, one, one, one, one, None) == -1
    assert b'sides out of range' in L.iamx_last_error()
    assert L.iamx_ortho_clear(1, 4, 4, odd, None, one, one, None) == -1 and b'aligned' in L.iamx_last_error()

    def raster(mode=0, S=8, X=one, frame=one, h_s=64, w_s=96, params=par, box=(0, 0, 3, 3), H=4, W=4, acc=one,
               index=one):
        return L.iamx_ortho_raster_image(mode, S, X, one, one, one, frame, h_s, w_s, params, 0, *box, H, W, acc,
                                         index, one, one, None)
    assert raster(X=None) == -1 and b'null pointer' in L.iamx_last_error()
    assert raster(frame=None) == -1 and raster(params=None) == -1 and raster(index=None) == -1
    assert raster(S=0) == -1 and b'grid steps' in L.iamx_last_error()
    assert raster(S=33) == -1
    assert raster(h_s=0) == -1 and b'empty frame' in L.iamx_last_error()
    assert raster(H=0) == -1 and raster(W=(1 << 20) + 1) == -1 and b'sides out of range' in L.iamx_last_error()
    assert raster(box=(0, 0, 4, 3)) == -1 and b'leaves the raster' in L.iamx_last_error()
    assert raster(box=(-1, 0, 3, 3)) == -1
    assert raster(mode=3) == -1
    assert raster(mode=1, acc=odd, index=None) == -1 and b'aligned' in L.iamx_last_error()
    bad = (ctypes.c_double * 8)(5472, 3648, 0.0, 10.0, 0.0, 1.0, 2.0, 3.0)
    assert raster(params=bad) == -1 and b'not finite' in L.iamx_last_error()
    assert raster(box=(2, 0, 1, 3)) == 0                                         # covers nothing: no launch
    assert L.iamx_ortho_resolve(4, 4, None, one, one, None) == -1 and b'null pointer' in L.iamx_last_error()
    assert L.iamx_ortho_resolve(4, 0, one, one, one, None) == -1
    assert L.iamx_ortho_resolve(4, 4, odd, one, one, None) == -1


def test_map_grids_gives_build_maps_grids(tmp_path, monkeypatch):
    """build_map and ortho.group_grids go through one map_grids: with the device stage answered from
    the golden, both leave the recorded grid_list and distorted_uv on the images"""
    from imageanalysis_amd import ortho, panda3d, render_panda3d as rp
    g = oc.golden('step5_mid_tilted')
    names = list(g['groups'][0])
    enu = np.array([g['images'][n]['grid_list'] for n in names], np.float64)
    ned = np.stack([enu[:, :, 1], enu[:, :, 0], -enu[:, :, 2]], axis=-1)
    calls = []
    monkeypatch.setattr(rp, 'surface_grids', lambda *a, **k: calls.append(len(a[2])) or ned.copy())
    monkeypatch.setattr(panda3d, 'generate_from_grid', lambda *a, **k: calls.append('eggs'))

    def recorded(proj):
        for n in names:
            im, want = proj.findImageByName(n), g['images'][n]
            assert np.array(im.grid_list, np.float64).tobytes() == want['grid_list'].tobytes(), n
            assert np.array(im.distorted_uv, np.float64).tobytes() == want['distorted_uv'].tobytes(), n
            assert im.z_avg == want['z_avg']
    s5.set_switches(rp, g)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            proj = s5.project(g, str(tmp_path))
            (tmp_path / 'matches_grouped').write_bytes(g['matches_in'])
            rp.build_map(proj, g['groups'], 0)
            recorded(proj)
            assert calls == [30, 'eggs']
            proj = s5.project(g, str(tmp_path))
            images, grids, uv = ortho.group_grids(proj, g['groups'], 0)
            recorded(proj)
    finally:
        s5.reset_switches(rp)
    assert calls == [30, 'eggs', 30] and [im.name for im in images] == names
    assert grids.tobytes() == enu.tobytes() and uv.tobytes() == g['images'][names[0]]['distorted_uv'].tobytes()
    assert not os.path.exists(str(tmp_path / 'ortho'))          # (group_grids writes nothing of its own)
