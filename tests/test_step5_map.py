"""CPU: the host half of Step 5 ("Create the map") against the reference's own runs
(tests/golden/step5_*.pkl.gz, tools/gen_step5_golden.py): the elevation statistics and surface.bin,
the redistort restatement, the .egg writer, the host's seed grid, the new C ABI's argument checks and
install().  The kernels themselves are held to scipy and to the goldens in test_step5_map_gpu.py."""
import contextlib
import io
import os
import pickle
import types

import numpy as np
import pytest

import step5_common as s5

IDS = [os.path.basename(p)[6:-7] for p in s5.CASES]


def test_goldens_are_all_there_and_off_every_decision():
    assert len(s5.CASES) == 12
    for path in s5.CASES:
        g = s5.load(path)
        assert g['margin'] >= 1e-6, path
    tilted = s5.load(os.path.join(s5.GOLD, 'step5_mid_tilted.pkl.gz'))
    grid = np.array([v['grid_list'] for v in tilted['images'].values()])
    n_look = np.diff(tilted['lookups']['ray_ptr'])
    assert np.isnan(grid).any() and np.isnan(tilted['lookups']['z']).any()      # < 30 degrees; left the hull
    assert (n_look == 0).any() and len(tilted['removed']) == 1                  # above the horizon; an egg removed
    out = s5.load(os.path.join(s5.GOLD, 'step5_dist_outlier.pkl.gz'))
    assert 'Discarding match with excessive altitude:' in out['stdout']


@pytest.mark.parametrize('form', ['lists', 'arrays'])
@pytest.mark.parametrize('path', s5.CASES, ids=IDS)
def test_statistics_and_surface_bin(path, form, tmp_path):
    """z_avg of every image and the surface.bin bytes are the reference's, from the loaded pickle
    and from the array-backed Chains (np.bincount adds in input order: the same float sums)"""
    from imageanalysis_amd import render_panda3d as rp
    from imageanalysis_amd.match_cleanup import Chains
    g = s5.load(path)
    proj = s5.project(g, str(tmp_path))
    matches = pickle.loads(g['matches_in'])
    if form == 'arrays':
        matches = Chains.from_lists(matches)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        pts, vals = rp.elevation_stats(proj, g['groups'][0], 0, matches)
        rp.save_surface(proj.analysis_dir, pts, vals)
    if form == 'arrays':
        assert matches.untouched()                       # read through the arrays, no lists were built
    for name, want in g['images'].items():
        im = proj.findImageByName(name)
        assert im.z_avg == want['z_avg'] and type(im.z_avg) is type(want['z_avg']), name
    with open(os.path.join(str(tmp_path), 'models', 'surface.bin'), 'rb') as f:
        assert f.read() == g['surface_bin']
    ours, theirs = s5.log_lines(out.getvalue()), s5.log_lines(g['stdout'])
    assert ours == theirs[1:1 + len(ours)]               # (their first line: "Loading optimized match points ...")
    assert sum(l.startswith('Discarding match') for l in ours) == (1 if g['case'] == 'outlier' else 0)


@pytest.mark.parametrize('path', s5.CASES, ids=IDS)
def test_redistort_is_the_reference_bit_for_bit(path):
    """Bit for bit, not within an ulp: redistort() runs the reference's expressions on numpy float64
    scalars in the reference's order (powers as powers), so the same scalar routines round the same."""
    from imageanalysis_amd import render_panda3d as rp
    from imageanalysis_amd.hostlib import camera
    g = s5.load(path)
    s5.project(g)
    grid = rp.pixel_grid(g['width'], g['height'], 8)
    got = np.array(rp.redistort(grid, camera.get_K(True), camera.get_dist_coeffs(True)), np.float64)
    for want in g['images'].values():
        assert got.tobytes() == np.ascontiguousarray(want['distorted_uv'], np.float64).tobytes()


@pytest.mark.parametrize('path', s5.CASES, ids=IDS)
def test_eggs_byte_for_byte(path, tmp_path, monkeypatch):
    from imageanalysis_amd import panda3d
    g = s5.load(path)
    proj = s5.project(g, str(tmp_path))
    group = g['groups'][0]
    shared_uv = None
    for name in group:
        im = proj.findImageByName(name)
        im.grid_list = g['images'][name]['grid_list'].tolist()
        if shared_uv is None:
            shared_uv = g['images'][name]['distorted_uv'].tolist()
        im.distorted_uv = shared_uv
    proj.findImageByName(g['groups'][1][0]).grid_list = []          # never asked for: not in the group
    calls = []
    monkeypatch.setattr(panda3d, 'make_textures_opencv', lambda *a, **k: calls.append((a, k)))
    models = tmp_path / 'models'
    models.mkdir()
    for name in g['removed']:
        (models / name).write_text('left over from an earlier run')
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        panda3d.generate_from_grid(proj, group, src_dir='/nonexistent', analysis_dir=str(tmp_path), resolution=512)
    assert calls == [(('/nonexistent', str(tmp_path), proj.image_list, 512), {})]
    assert sorted(os.listdir(str(models))) == sorted(g['eggs'])
    for name, want in g['eggs'].items():
        assert (models / name).read_bytes() == want, name
    ours = s5.log_lines(out.getvalue())
    theirs = [l for l in s5.log_lines(g['stdout']) if l.startswith(('EGG file name:', 'Warning: no polygons'))]
    assert ours == theirs
    assert sum(l.startswith('Warning: no polygons') for l in ours) == len(g['removed'])


def test_empty_grid_list_is_skipped(tmp_path, monkeypatch):
    from imageanalysis_amd import panda3d
    g = s5.load(s5.CASES[0])
    proj = s5.project(g, str(tmp_path))
    monkeypatch.setattr(panda3d, 'make_textures_opencv', lambda *a, **k: None)
    (tmp_path / 'models').mkdir()
    name = g['groups'][0][0]
    im = proj.findImageByName(name)
    im.grid_list, im.distorted_uv = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        panda3d.generate_from_grid(proj, [name], analysis_dir=str(tmp_path))
    assert os.listdir(str(tmp_path / 'models')) == []


def test_seed_grid_cells_outside_the_hull_take_a_real_triangle():
    import scipy.spatial
    from imageanalysis_amd import kernels
    rng = np.random.default_rng(3)
    r, a = np.sqrt(rng.random(400)), rng.random(400) * 2 * np.pi
    tri = scipy.spatial.Delaunay(np.stack([r * np.cos(a), r * np.sin(a)], 1))        # a disc: corners outside
    seed, bbox = kernels.surface_seed_grid(tri, 64)
    assert seed.shape == (64, 64) and seed.dtype == np.int32
    assert seed.min() >= 0 and seed.max() < len(tri.simplices)
    assert tri.find_simplex(np.array([[bbox[0], bbox[1]]]))[0] == -1                 # the corner is outside
    with pytest.raises(ValueError):
        kernels.surface_seed_grid(tri, 0)


def test_argument_checks_do_not_need_a_gpu():
    import ctypes
    from imageanalysis_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(128)          # never dereferenced: the checks come before the launch
    odd = ctypes.c_void_p(64)
    bbox = (ctypes.c_double * 4)(0, 0, 1, 1)
    assert L.iamx_surface_pack(None, None, None, 4, None, None) == -1
    assert b'null pointer' in L.iamx_last_error()
    assert L.iamx_surface_pack(one, one, one, 0, one, None) == -1
    assert L.iamx_surface_pack(one, one, one, 4, odd, None) == -1 and b'aligned' in L.iamx_last_error()
    assert L.iamx_surface_interp(None, 4, None, 4, None, 1, None, None, 8, 0, None, None, None, None) == -1
    assert b'null pointer' in L.iamx_last_error()
    assert L.iamx_surface_interp(one, 0, one, 4, one, 1, bbox, one, 8, 0, one, one, None, None) == -1
    assert L.iamx_surface_interp(one, 4, one, 2, one, 1, bbox, one, 8, 0, one, one, None, None) == -1
    assert L.iamx_surface_interp(one, 4, one, 4, one, 0, bbox, one, 8, 0, one, one, None, None) == -1
    assert b'seed grid' in L.iamx_last_error()
    assert L.iamx_surface_interp(one, 4, one, 4, one, 1, bbox, one, -1, 0, one, one, None, None) == -1
    assert L.iamx_surface_interp(odd, 4, one, 4, one, 1, bbox, one, 8, 0, one, one, None, None) == -1
    grid = lambda *a: L.iamx_surface_grid(*a)                                      # noqa: E731
    assert grid(one, 4, one, 4, one, 1, bbox, None, None, one, 1, None, 81, 0, 0, 0.0, 0, None, None, None,
                None, None) == -1 and b'null pointer' in L.iamx_last_error()
    assert grid(None, 0, None, 0, None, 0, None, one, one, one, 1, one, 81, 0, 0, 0.0, 0, one, one, one,
                None, None) == -1                        # no triangulation, and not the ground-plane mode
    assert grid(one, 4, one, 4, one, 1, bbox, one, one, one, 1, one, 0, 0, 0, 0.0, 0, one, one, one,
                None, None) == -1 and b'bad size' in L.iamx_last_error()
    assert grid(one, 4, one, 4, one, 1, bbox, one, one, one, 1 << 30, one, 81, 0, 0, 0.0, 0, one, one, one,
                None, None) == -1 and b'too many rays' in L.iamx_last_error()
    # nothing to do is not an error, and launches nothing
    assert L.iamx_surface_interp(one, 4, one, 4, one, 1, bbox, one, 0, 0, one, one, None, None) == 0
    assert grid(None, 0, None, 0, None, 0, None, one, one, one, 0, one, 81, 0, 1, 3.0, 0, one, one, one,
                None, None) == 0


def test_install_replaces_build_map_and_reads_the_reference_modules_switches():
    from imageanalysis_amd import render_panda3d as rp
    assert rp.switches() == dict(grid_steps=8, texture_resolution=512, use_direct_pose=False,
                                 force_ground_elevation_m=None, use_srtm_surface=None, no_extrapolate=False)
    ref = types.ModuleType('render_panda3d')
    ref.build_map = lambda *a, **k: 'reference'
    ref.intersect2d = 'untouched'
    for k, v in rp.switches().items():
        setattr(ref, k, v)
    try:
        rp.install(ref)
        assert ref.build_map is rp.build_map and ref.intersect2d == 'untouched'
        ref.grid_steps, ref.no_extrapolate = 4, True
        assert rp.switches()['grid_steps'] == 4 and rp.switches()['no_extrapolate'] is True
        assert rp.grid_steps == 8
    finally:
        rp._switch_module = None
