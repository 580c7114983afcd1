"""GPU: csrc/terrain.hip through the C ABI against the goldens of tools/gen_terrain_golden.py, and the
paths that read it (srtm.heights / intersect / interpolate_vectors, render_panda3d.map_grids in SRTM
mode, the elevation hooks).

Tolerances as in tests/test_terrain.py: heights 1e-9 m absolute, fill values and NaN bit-equal; ray hits
max(16 x 0.0, 1e-9 max(1, |ref|)) -- the restatement's worst difference from the reference's recorded
points, measured on the CPU on these goldens, is 0.0; iters and flags equal for every ray; rays that end
at the cap of 25 rounds compared by iters and flags only."""
import numpy as np
import pytest

import terrain_common as tc
import terrain_restatement as tr
from terrain_common import _Image, _Project, assert_points, ray_bound

pytestmark = pytest.mark.gpu


@pytest.fixture
def srtm(monkeypatch):
    from imageanalysis_amd import srtm as mod
    monkeypatch.setattr(mod, 'tile_dict', {})
    monkeypatch.setattr(mod, 'ned_interp', None)
    return mod


def _terrain(axis_n, axis_e, grid):
    from imageanalysis_amd import kernels
    return kernels.Terrain(axis_n, axis_e, grid)


def test_constants_match_the_header():
    from imageanalysis_amd import kernels
    assert (kernels.TERRAIN_SKY, kernels.TERRAIN_CAPPED, kernels.TERRAIN_LEFT_GRID) == (tr.SKY, tr.CAPPED, tr.LEFT_GRID)


def test_heights_against_the_reference():
    from imageanalysis_amd import kernels
    q = tc.load('queries')
    T = _terrain(q['axis_n'], q['axis_e'], q['grid'])
    for name, (pts, z) in q['groups'].items():
        got = kernels.terrain_heights(T, pts).cpu().numpy()
        special = ~np.isfinite(z) | (z == tr.FILL)
        assert np.array_equal(got[special], z[special], equal_nan=True), name     # fill and NaN: bit-equal
        assert (np.abs(got[~special] - z[~special]) <= 1e-9).all(), name
    # a two-node axis, and axes that are not uniform at all
    T2 = _terrain([0.0, 1.0], [0.0, 0.5, 4.0, 4.25, 100.0], np.arange(10.0).reshape(2, 5) ** 2)
    pts = np.array([[0.5, 0.25], [1.0, 100.0], [0.0, 0.0], [0.25, 4.1], [0.75, 50.0], [1.0000001, 1.0], [0.3, -1e-12]])
    ref = tr.heights(np.array([0.0, 1.0]), np.array([0.0, 0.5, 4.0, 4.25, 100.0]), np.arange(10.0).reshape(2, 5) ** 2, pts)
    assert np.array_equal(kernels.terrain_heights(T2, pts).cpu().numpy(), ref)
    assert kernels.terrain_heights(T2, np.zeros((0, 2))).shape == (0,)


@pytest.mark.parametrize('scene', ['smooth', 'n1', 'n63', 'n64', 'n65', 'edge', 'steep'])
def test_rays_against_the_reference(scene):
    from imageanalysis_amd import kernels
    R = tc.load('rays')
    s = [x for x in R['scenes'] if x['name'] == scene][0]
    T = _terrain(R['axis_n'], R['axis_e'], R['terrains'][s['terrain']])
    pts, iters, flags = (x.cpu().numpy() for x in kernels.terrain_rays(T, None, s['ned'], v=s['v']))
    assert np.array_equal(iters, s['iters']) and np.array_equal(flags, s['flags'])
    assert_points(pts, s['pts'], s['flags'])
    sky = (s['flags'] & tr.SKY) != 0
    assert np.array_equal(pts[sky], np.broadcast_to(s['ned'][:, None, :], pts.shape)[sky])
    # a batched launch equals per-image launches bit for bit
    for i in range(len(s['ned'])):
        one = [x.cpu().numpy() for x in kernels.terrain_rays(T, None, s['ned'][i:i + 1], v=s['v'][i:i + 1])]
        assert np.array_equal(one[0][0], pts[i], equal_nan=True)
        assert np.array_equal(one[1][0], iters[i]) and np.array_equal(one[2][0], flags[i])
    if s['M'] is not None:
        # the entry that forms the rays itself: unit(M . [u, v, 1])
        p2, i2, f2 = (x.cpu().numpy() for x in kernels.terrain_rays(T, s['M'], s['ned'], uv=s['uv']))
        assert np.array_equal(i2, s['iters']) and np.array_equal(f2, s['flags'])
        assert_points(p2, s['pts'], s['flags'])
        for i in range(len(s['ned'])):
            one = [x.cpu().numpy() for x in kernels.terrain_rays(T, s['M'][i:i + 1], s['ned'][i:i + 1], uv=s['uv'])]
            assert np.array_equal(one[0][0], p2[i], equal_nan=True)
            assert np.array_equal(one[1][0], i2[i]) and np.array_equal(one[2][0], f2[i])


def test_intersect_equals_interpolate_vectors_of_unit_rays(srtm):
    from imageanalysis_amd.render_panda3d import unit_rays
    R = tc.load('rays')
    s = [x for x in R['scenes'] if x['name'] == 'n65'][0]
    srtm.adopt(srtm.GridInterpolator((R['axis_n'], R['axis_e']), R['terrains'][s['terrain']]))
    pts, iters, flags = srtm.intersect(s['M'], s['ned'], s['uv'], with_stats=True)
    assert np.array_equal(srtm.intersect(s['M'], s['ned'], s['uv']), pts)
    for i in range(len(s['ned'])):
        ref = np.array(srtm.interpolate_vectors(s['ned'][i].tolist(), unit_rays(s['M'][i], s['uv'])))
        assert (np.abs(pts[i] - ref) <= ray_bound(ref)).all()
    assert (iters > 0).all() and (flags == 0).all()
    one = srtm.interpolate_vector(s['ned'][0].tolist(), s['v'][0, 7])
    assert isinstance(one, list) and (np.abs(np.array(one) - s['pts'][0, 7]) <= ray_bound(s['pts'][0, 7])).all()
    h = srtm.heights(s['ned'][:, :2])
    assert np.array_equal(h, srtm.ned_interp(s['ned'][:, :2]))
    with pytest.raises(Exception):
        srtm.adopt(None)


def test_terrain_must_be_initialised(srtm):
    with pytest.raises(RuntimeError, match='never initialised'):
        srtm.heights([[0.0, 0.0]])
    with pytest.raises(RuntimeError, match='never initialised'):
        srtm.interpolate_vectors([0.0, 0.0, -100.0], [np.array([0.0, 0.0, 1.0])])


def test_map_grids_in_srtm_mode_on_the_mid_scene(srtm, monkeypatch):
    import step5_common as s5
    from imageanalysis_amd import _deps, render_panda3d
    m = tc.load('mid')
    monkeypatch.setitem(_deps._resolved, 'srtm', srtm)
    g = dict(names=m['names'], poses=m['poses'], poses_opt=m['poses'], width=m['width'], height=m['height'],
             camera=dict(K=m['K'], K_opt=m['K'], dist=m['dist'], dist_opt=m['dist']))
    proj = s5.project(g)
    for im in proj.image_list:
        im.z_avg = 0.0
    inits = []

    def initialize(ref, width_m, height_m, step_m):
        # (the golden terrain in the place of tiles: what process.py's own initialize would have left)
        inits.append((list(ref), width_m, height_m, step_m))
        srtm.adopt(srtm.GridInterpolator((m['axis_n'], m['axis_e']), m['grid']))
    monkeypatch.setattr(srtm, 'initialize', initialize)
    sw = dict(grid_steps=m['grid_steps'], texture_resolution=512, use_direct_pose=True,
              force_ground_elevation_m=None, use_srtm_surface=True, no_extrapolate=False)
    images = render_panda3d.map_grids(proj, m['group'], None, None, sw, [45.0, -93.0, 280.0])
    assert inits == [([45.0, -93.0, 280.0], 6000, 6000, 30)]
    assert [im.name for im in images] == m['group']
    for i, im in enumerate(images):
        enu = np.array(im.grid_list, np.float64)
        ned = np.stack([enu[:, 1], enu[:, 0], -enu[:, 2]], 1)
        assert ned.shape == m['pts'][i].shape == (81, 3)
        assert (np.abs(ned - m['pts'][i]) <= ray_bound(m['pts'][i])).all(), (i, np.abs(ned - m['pts'][i]).max())


def test_elevation_hooks_on_the_device(srtm, tmp_path, monkeypatch):
    from imageanalysis_amd import _deps, match_cleanup, smart
    monkeypatch.setitem(_deps._resolved, 'srtm', srtm)
    q = tc.load('queries')
    srtm.adopt(srtm.GridInterpolator((q['axis_n'], q['axis_e']), q['grid']))
    images = [_Image('terrain_hook_gpu_%02d' % i, [30.0 * i - 100.0, 17.0 * i, -400.0 if i != 2 else -200.0]) for i in range(6)]
    proj = _Project(images, str(tmp_path))
    expect = [srtm.ned_interp([im.ned[0], im.ned[1]])[0] for im in images]
    smart.update_srtm_elevations(proj)
    for im, z in zip(images, expect):
        assert smart.smart_node.getChild(im.name, True).getFloat('srtm_surface_m') == float('%.1f' % z)
    base = match_cleanup._base_elevations(proj)
    assert np.allclose(base, [min(z, -im.ned[2] - 1) for im, z in zip(images, expect)], rtol=0, atol=1e-9)
