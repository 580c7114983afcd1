"""CPU: the terrain module (imageanalysis_amd/srtm.py, hostlib/geodesy.py) and the numpy restatement of
csrc/terrain.hip against the goldens of tools/gen_terrain_golden.py (the reference's own lib/srtm.py).

Tolerances.  Heights: 1e-9 m absolute (values <= 1e4 m, four products and one rounding each: <= 1e-11 m).
Ray hits: the worst difference between tests/terrain_restatement.py and the reference's recorded points,
measured on these goldens on the CPU, is 0.0 (the restatement follows scipy's and lib/srtm.py's order of
operations and equals them bit for bit), so the bound max(16 x that, 1e-9 max(1, |ref|)) is its second
term, the figure iamx_triangulate_ground is held to.  Rays that end at the cap of 25 rounds are compared
by iters and flags only."""
import os

import numpy as np
import pytest

import terrain_common as tc
import terrain_restatement as tr
from terrain_common import _Image, _Project, assert_points

@pytest.fixture
def srtm(monkeypatch):
    """the mirror with its module state put back afterwards"""
    from imageanalysis_amd import srtm as mod
    monkeypatch.setattr(mod, 'tile_dict', {})
    monkeypatch.setattr(mod, 'ned_interp', None)
    return mod


# ---- the restatement against the goldens -------------------------------------------------------------
def test_restated_heights_equal_the_reference():
    q = tc.load('queries')
    for name, (pts, z) in q['groups'].items():
        got = tr.heights(q['axis_n'], q['axis_e'], q['grid'], pts)
        special = ~np.isfinite(z) | (z == tr.FILL)
        assert np.array_equal(got[special], z[special], equal_nan=True), name     # fill and NaN: bit-equal
        assert (np.abs(got[~special] - z[~special]) <= 1e-9).all(), name
    assert (q['groups']['outside'][1] == tr.FILL).all() and np.isnan(q['groups']['nan'][1]).all()
    assert not (q['groups']['border'][1] == tr.FILL).any()


@pytest.mark.parametrize('scene', ['smooth', 'n1', 'n63', 'n64', 'n65', 'edge', 'steep'])
def test_restated_rays_equal_the_reference(scene):
    R = tc.load('rays')
    s = [x for x in R['scenes'] if x['name'] == scene][0]
    errors = []
    pts, iters, flags = tr.rays(R['axis_n'], R['axis_e'], R['terrains'][s['terrain']], s['ned'], s['v'], errors)
    assert np.array_equal(iters, s['iters']) and np.array_equal(flags, s['flags'])
    assert_points(pts, s['pts'], s['flags'])
    capped = (s['flags'] & tr.CAPPED) != 0
    assert capped.mean() <= (0.05 if scene == 'steep' else 0.0)
    # every iteration's error of every ray that does not end at the cap
    ptr = s['err_ptr']
    ray = 0
    for i in range(s['v'].shape[0]):
        for k in range(s['v'].shape[1]):
            ref = s['errors'][ptr[ray]:ptr[ray + 1]]
            flat = i * s['v'].shape[1] + k
            got = [e[flat] for m, e in errors if m[flat]]
            ray += 1
            if capped[i, k]:
                continue
            assert len(got) == len(ref)
            assert np.allclose(got, ref, rtol=0, atol=1e-9, equal_nan=True)
    if s['M'] is not None:
        assert np.abs(tr.unit_rays(s['M'], s['uv']) - s['v']).max() <= 4 * np.finfo(float).eps


def test_the_scenes_hold_what_they_were_built_for():
    R = tc.load('rays')
    by = {s['name']: s for s in R['scenes']}
    assert [by[k]['v'].shape[1] for k in ('smooth', 'n1', 'n63', 'n64', 'n65')] == [257, 1, 63, 64, 65]
    assert all(by[k]['v'].shape[0] == 3 for k in by)
    e = by['edge']
    assert (e['iters'][0] == 0).all()                                    # the camera on the ground
    assert (e['flags'][0, 5:7] == tr.SKY).all() and e['v'][0, 5, 2] == 0 and e['v'][0, 6, 2] < 0
    assert np.array_equal(e['pts'][0, 5], e['ned'][0])
    assert ((e['flags'][1] & tr.LEFT_GRID) != 0).all()                  # the camera outside the grid
    assert np.isnan(e['pts'][1, 4, 0]) and np.isnan(e['v'][1, 5, 2]) and np.isnan(e['pts'][1, 5, :2]).all()
    assert ((e['flags'][2] & tr.LEFT_GRID) != 0).sum() >= 8            # rays that leave during the iteration
    assert ((by['steep']['flags'] & tr.CAPPED) != 0).any() and (by['steep']['iters'].max() == 25)
    for s in R['scenes']:
        assert min(s['margins'].values()) >= 1e-6


# ---- the mirror's tile handling ----------------------------------------------------------------------
@pytest.mark.parametrize('case', ['one', 'corner', 'voids'])
def test_tiles_give_the_reference_grid(case, srtm, tmp_path, monkeypatch):
    g = [c for c in tc.load('tiles')['cases'] if c['name'] == case][0]
    for tile, (seed, voids) in g['tiles'].items():
        tc.write_tile(tmp_path, tile, seed, voids)
    monkeypatch.setattr(srtm, 'default_cache_dir', str(tmp_path))
    srtm.initialize(g['ref'], g['width_m'], g['height_m'], g['step_m'])
    assert list(srtm.tile_dict) == g['tile_order']
    assert np.array_equal(srtm.ned_interp.grid[0], g['axis_n']) and np.array_equal(srtm.ned_interp.grid[1], g['axis_e'])
    assert srtm.ned_interp.values.shape == g['grid'].shape == (51, 81)
    # the tiles' words are whole metres: the NED nodes are blends of them, 1e-9 m like every height
    assert np.abs(srtm.ned_interp.values - g['grid']).max() <= 1e-9
    for tile, (q, z) in g['probes'].items():
        got = srtm.tile_dict[tile].lla_interpolate(q)
        special = z == srtm.FILL
        assert np.array_equal(got[special], z[special]) and np.abs(got - z).max() <= 1e-9
    if case == 'voids':
        words = tc.tile_words(*g['tiles']['N45W094'])
        assert {65535, 10001, 40000} <= set(np.unique(words).tolist())
        assert srtm.tile_dict['N45W094'].srtm_z.max() == 65535
        assert srtm.tile_dict['N45W094'].lla_interp.values.max() <= 10000
    # ned_interp is callable like the reference's
    one = srtm.ned_interp([12.5, -40.25])
    many = srtm.ned_interp(np.array([[12.5, -40.25], [1e6, 0.0], [np.nan, 0.0]]))
    assert one.shape == (1,) and many.shape == (3,) and one[0] == many[0]
    assert many[1] == srtm.FILL and np.isnan(many[2])


def test_host_ned_interp_equals_the_reference(srtm):
    q = tc.load('queries')
    f = srtm.GridInterpolator((q['axis_n'], q['axis_e']), q['grid'])
    for name, (pts, z) in q['groups'].items():
        assert np.allclose(f(pts), z, rtol=0, atol=1e-9, equal_nan=True), name


def test_make_tile_name():
    from imageanalysis_amd.srtm import lla_ll_corner, make_tile_name
    assert make_tile_name(45.2, -93.1) == 'N45W094'
    assert make_tile_name(45.0, -93.0) == 'N45W093'
    assert make_tile_name(-33.9, 151.2) == 'S34E151'
    assert make_tile_name(7.5, 12.2) == 'N 7E012'            # "%2d" as written: a space below 10
    assert make_tile_name(-0.5, -0.5) == 'S 1W001'
    assert lla_ll_corner(-0.5, 10.0) == (-1, 10)


def test_a_missing_tile_names_the_file_to_provide(srtm, tmp_path, monkeypatch):
    monkeypatch.setattr(srtm, 'default_cache_dir', str(tmp_path))
    with pytest.raises(FileNotFoundError) as e:
        srtm.initialize([45.3, -93.6, 280.0], 2400, 1500, 30)
    assert os.path.join(str(tmp_path), 'N45W094.hgt.zip') in str(e.value)
    assert not hasattr(srtm, 'download_srtm') and not hasattr(srtm.SRTM, 'download_srtm')
    t = srtm.SRTM(45.3, -93.6)
    assert t.srtm_cache_dir == str(tmp_path)
    t.set_srtm_cache_dir(str(tmp_path / 'nowhere'))
    assert t.srtm_cache_dir == str(tmp_path)
    monkeypatch.setattr(srtm, 'default_cache_dir', '/var/tmp')
    assert srtm.SRTM(0, 0).srtm_cache_dir == '/var/tmp'


# ---- geodesy against 50 digits -------------------------------------------------------------------------
def _mp_ned2lla(ned, ref):
    import mpmath as mp
    mp.mp.dps = 50
    a = mp.mpf(6378137)
    f = 1 / mp.mpf('298.257223563')
    e2 = f * (2 - f)

    def ecef(lat, lon, h):
        s, c = mp.sin(lat), mp.cos(lat)
        N = a / mp.sqrt(1 - e2 * s * s)
        return [(N + h) * c * mp.cos(lon), (N + h) * c * mp.sin(lon), (N * (1 - e2) + h) * s]
    lat0, lon0, h0 = mp.radians(mp.mpf(ref[0])), mp.radians(mp.mpf(ref[1])), mp.mpf(ref[2])
    n, e, d = (mp.mpf(float(x)) for x in ned)
    sl, cl, so, co = mp.sin(lat0), mp.cos(lat0), mp.sin(lon0), mp.cos(lon0)
    x0 = ecef(lat0, lon0, h0)
    x = x0[0] + (-sl * co) * n + (-so) * e + (-cl * co) * d
    y = x0[1] + (-sl * so) * n + co * e + (-cl * so) * d
    z = x0[2] + cl * n + (-sl) * d
    # ECEF -> geodetic: Newton on g(lat) = p tan(lat) - z - e2 N(lat) sin(lat)
    p = mp.sqrt(x * x + y * y)
    g = lambda t: p * mp.tan(t) - z - e2 * a * mp.sin(t) / mp.sqrt(1 - e2 * mp.sin(t) ** 2)   # noqa: E731
    lat = mp.findroot(g, mp.atan2(z, p * (1 - e2)), tol=mp.mpf(10) ** -45)
    N = a / mp.sqrt(1 - e2 * mp.sin(lat) ** 2)
    h = p * mp.cos(lat) + z * mp.sin(lat) - a * mp.sqrt(1 - e2 * mp.sin(lat) ** 2)
    assert abs(p / mp.cos(lat) - N - h) < mp.mpf(10) ** -30
    return float(mp.degrees(lat)), float(mp.degrees(mp.atan2(y, x))), float(h)


@pytest.mark.parametrize('lat_ref', [0.0, 45.0, -33.0, 89.0])
def test_geodesy_against_fifty_digits(lat_ref):
    from imageanalysis_amd.hostlib import geodesy
    ref = [lat_ref, -93.25 if lat_ref >= 0 else 151.2, 287.5]
    rng = np.random.default_rng(int(lat_ref) + 100)
    ned = np.vstack([rng.uniform(-3000, 3000, (12, 3)), [[0, 0, 0], [3000, 3000, -3000], [-3000, 3000, 3000]]])
    lat, lon, alt = geodesy.ned2lla(ned, *ref)
    assert lat.shape == lon.shape == alt.shape == (len(ned),)
    for k in range(len(ned)):
        rl, ro, ra = _mp_ned2lla(ned[k], ref)
        assert abs(lat[k] - rl) <= 1e-9 and abs(lon[k] - ro) <= 1e-9 and abs(alt[k] - ra) <= 1e-6
    back = geodesy.lla2ned(lat, lon, alt, *ref)
    assert back.shape == ned.shape and np.abs(back - ned).max() <= 1e-6
    # one point in: scalars out, and [3] back
    one = geodesy.ned2lla(ned[3].tolist(), *ref)
    assert all(np.ndim(x) == 0 for x in one) and one == (lat[3], lon[3], alt[3])
    row = geodesy.ned2lla(ned[3:4], *ref)
    assert float(row[0]) == lat[3]
    assert np.abs(geodesy.lla2ned(*one, *ref) - ned[3]).max() <= 1e-6


# ---- wiring ------------------------------------------------------------------------------------------
def test_deps_gives_the_mirror_outside_the_reference_tree(monkeypatch):
    from imageanalysis_amd import _deps, srtm as mirror
    monkeypatch.setattr(_deps, 'HAVE_PROPS', False)               # (no reference environment: no lib.srtm)
    monkeypatch.delitem(_deps._resolved, 'srtm', raising=False)
    assert _deps.srtm() is mirror
    assert 'srtm' not in _deps.REPLACED


def _host_heights(monkeypatch):
    """kernels.terrain_heights needs the device; here the launch is replaced by its restatement so that
    the wiring around it runs (tests/test_terrain_gpu.py runs the same wiring on the kernel)"""
    from imageanalysis_amd import srtm as mod
    calls = []

    def heights(points):
        calls.append(len(points))
        f = mod.ned_interp
        return tr.heights(f.grid[0], f.grid[1], f.values, points)
    monkeypatch.setattr(mod, 'heights', heights)
    return calls


def test_elevation_hooks_read_the_initialised_terrain(srtm, tmp_path, monkeypatch):
    from imageanalysis_amd import _deps, match_cleanup, smart
    monkeypatch.setitem(_deps._resolved, 'srtm', srtm)
    q = tc.load('queries')
    images = [_Image('terrain_hook_%02d' % i, [30.0 * i - 100.0, 17.0 * i, -400.0 if i != 2 else -200.0]) for i in range(6)]
    images.append(_Image('terrain_hook_outside', [1e5, 0.0, -400.0]))
    proj = _Project(images, str(tmp_path))
    with pytest.raises(RuntimeError, match='never initialised'):
        smart.update_srtm_elevations(proj)
    with pytest.raises(RuntimeError, match='never initialised'):
        match_cleanup._base_elevations(proj)
    srtm.adopt(srtm.GridInterpolator((q['axis_n'], q['axis_e']), q['grid']))
    calls = _host_heights(monkeypatch)
    expect = [srtm.ned_interp([im.ned[0], im.ned[1]])[0] for im in images]
    smart.update_srtm_elevations(proj)
    assert calls == [len(images)]                                   # one look-up for all cameras
    for im, z in zip(images, expect):
        assert smart.smart_node.getChild(im.name, True).getFloat('srtm_surface_m') == float('%.1f' % z)
    base = match_cleanup._base_elevations(proj)
    assert calls == [len(images), len(images)]
    want = [min(z, -im.ned[2] - 1) for im, z in zip(images, expect)]
    assert np.allclose(base, want, rtol=0, atol=1e-9)
    assert base[2] == 199.0 and base[-1] == srtm.FILL             # the clamp; outside the grid as the reference
