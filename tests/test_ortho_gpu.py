"""The orthomosaic rasteriser on the device (csrc/ortho_raster.hip through imageanalysis_amd/ortho.py)
against the numpy restatement of its rules (tests/ortho_restatement.py): bgr, index and count byte
for byte, on the recorded Step 5 grids and on planted geometry.  Frames are synthetic hash patterns
handed over as device tensors."""
import contextlib
import io

import numpy as np
import pytest

import ortho_common as oc
import ortho_restatement as rs
import step5_common as s5

pytestmark = pytest.mark.gpu

MODES = ('best', 'feather')


def _dev(frames):
    import torch
    return [torch.from_numpy(np.array(f)).cuda() for f in frames]


def _equal(m, ref, what):
    """the device mosaic against the restatement's dict, byte for byte"""
    bgr, count = m.bgr.cpu().numpy(), m.count.cpu().numpy()
    assert bgr.shape == ref['bgr'].shape, what
    print('%s: %d x %d, covered %d, bgr bytes differing %d, count differing %d'
          % (what, bgr.shape[1], bgr.shape[0], int((ref['count'] > 0).sum()), int((bgr != ref['bgr']).sum()),
             int((count != ref['count']).sum())))
    assert count.dtype == np.uint16 and count.tobytes() == ref['count'].tobytes(), what
    if m.mode == 'best':
        index = m.index.cpu().numpy()
        assert index.dtype == np.int32 and index.tobytes() == ref['index'].tobytes(), what
    else:
        assert m.index is None
    assert bgr.tobytes() == ref['bgr'].tobytes(), what
    assert (m.x0, m.y1, m.gsd) == (ref['frame']['x0'], ref['frame']['y1'], ref['frame']['gsd'])


def _both(grids, uv, frames, width, height, gsd, what, modes=MODES):
    """compose on the device and in numpy, both modes; -> the restatement's dicts"""
    from imageanalysis_amd import ortho
    out = {}
    dev = _dev(frames)
    for mode in modes:
        ref = rs.compose(grids, uv, frames, width, height, gsd, mode)
        _equal(ortho.compose(grids, uv, dev, width, height, gsd, mode), ref, '%s %s' % (what, mode))
        out[mode] = ref
    return out


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scene', ['step5_mid_default', 'step5_mid_tilted'])
def test_recorded_grids_equal_the_restatement(scene, mode):
    """30 images, up to 20 over one pixel, 0.5 m; mid_tilted: 127 NaN vertices and the all-sky image"""
    from imageanalysis_amd import ortho
    names, grids, uv, width, height = oc.scene_input(scene)
    ref = oc.reference(scene, 0.5, mode)
    frames = _dev([oc.hash_frame(k) for k in range(len(grids))])
    m = ortho.compose(grids, uv, frames, width, height, 0.5, mode, names=names)
    _equal(m, ref, scene + ' ' + mode)
    assert m.names == names and ref['count'].max() >= 15
    again = ortho.compose(grids, uv, frames, width, height, 0.5, mode, names=names)      # the same call twice
    assert again.bgr.cpu().numpy().tobytes() == m.bgr.cpu().numpy().tobytes()
    assert again.count.cpu().numpy().tobytes() == m.count.cpu().numpy().tobytes()
    if mode == 'best':
        assert again.index.cpu().numpy().tobytes() == m.index.cpu().numpy().tobytes()


# ---- planted geometry: pixel coordinates (x right, y DOWN from the raster's top) -> an ENU grid ----
WIDTH, HEIGHT = 960.0, 640.0


def _grid(points_px, top):
    """vertices in pixels of a raster whose row 0 starts `top` pixels above y = 0; gsd 1 m"""
    p = np.asarray(points_px, np.float64)
    return np.stack([p[:, 0], top - p[:, 1], np.zeros(len(p))], axis=1)


def _uv(S):
    return np.array([[i * WIDTH / S, j * HEIGHT / S] for j in range(S + 1) for i in range(S + 1)])


def _lattice(S, x0, y0, x1, y1):
    return [[x0 + (x1 - x0) * i / S, y0 + (y1 - y0) * j / S] for j in range(S + 1) for i in range(S + 1)]


def _orders(S):
    a = np.arange((S + 1) ** 2).reshape(S + 1, S + 1)
    return {'as is': a.reshape(-1), 'rows reversed': a[::-1].reshape(-1), 'columns reversed': a[:, ::-1].reshape(-1),
            'transposed': a.T.reshape(-1)}


@pytest.mark.parametrize('S', [1, 2])
def test_corners_on_pixel_centres_in_all_four_vertex_orders(S):
    """every vertex on a pixel centre: edges through centres in both axis directions and along the
    cells' diagonals, so w == 0 occurs on owned and on unowned edges; the mirrored orders put
    u == 0, u == width, v == 0 and v == height on owned pixels"""
    pts = np.array(_lattice(S, 0.5, 0.5, 8.5, 6.5))
    seen_u, seen_v = set(), set()
    for name, order in _orders(S).items():
        grid = _grid(pts[order], 7.0)
        out = _both([grid], _uv(S), [oc.hash_frame(1)], WIDTH, HEIGHT, 1.0, 'centres S=%d %s' % (S, name))
        ref = out['best']
        assert ref['bgr'].shape == (7, 9, 3) and int((ref['count'] > 0).sum()) == 8 * 6, name
        rf = ref['frame']
        cells, _v = rs.used_cells(grid)
        owner, times, abc, wk = rs.cover(rf['X'][0], rf['Y'][0], S, cells, rf['W'], rf['H'])
        assert times.max() == 1 and (wk[owner >= 0] == 0).any()
        u, v = rs.texture_uv(abc[owner >= 0], wk[owner >= 0], _uv(S))
        seen_u |= set(u[(u == 0.0) | (u == WIDTH)].tolist())
        seen_v |= set(v[(v == 0.0) | (v == HEIGHT)].tolist())
    assert seen_u == {0.0, WIDTH} and seen_v == {0.0, HEIGHT}


def test_two_images_sharing_an_edge_cover_each_edge_pixel_once():
    for S in (1, 2):
        left = _grid(_lattice(S, 0.5, 0.5, 5.5, 9.5), 10.0)
        right = _grid(_lattice(S, 5.5, 0.5, 12.5, 9.5), 10.0)
        out = _both([left, right], _uv(S), [oc.hash_frame(1), oc.hash_frame(2)], WIDTH, HEIGHT, 1.0, 'shared edge')
        for ref in out.values():
            assert ref['count'].max() == 1 and int(ref['count'].sum()) == 12 * 9
            assert (ref['count'][:9, 5] == 1).all()                              # the shared column of centres
        assert (out['best']['index'][:9, :5] == 0).all() and (out['best']['index'][:9, 5:12] == 1).all()


def test_twin_images_the_lower_index_wins():
    grid = _grid(_lattice(2, 0.25, 0.25, 20.75, 18.75), 19.0)
    out = _both([grid, grid.copy()], _uv(2), [oc.hash_frame(1), oc.hash_frame(2)], WIDTH, HEIGHT, 1.0, 'twins')
    ref = out['best']
    covered = ref['count'] > 0
    assert covered.sum() > 300 and (ref['count'][covered] == 2).all() and (ref['index'][covered] == 0).all()
    assert ref['gap'] == 0.0                                 # (a tie on purpose: the rule, not a margin, decides)


def test_bow_tie_thin_triangle_and_nan_corner():
    # a bow-tie: the top row's two vertices swapped; the cell's triangles overlap and re-orient
    pts = _lattice(1, 0.3, 0.3, 20.6, 17.7)
    pts[0], pts[1] = pts[1], pts[0]
    grid = _grid(pts, 18.0)
    ref = _both([grid], _uv(1), [oc.hash_frame(4)], WIDTH, HEIGHT, 1.0, 'bow-tie')['best']
    rf = ref['frame']
    _o, times, _a, _w = rs.cover(rf['X'][0], rf['Y'][0], 1, np.ones((1, 1), bool), rf['W'], rf['H'])
    assert times.max() == 2 and 0 < (ref['count'] > 0).sum() < rf['W'] * rf['H']      # folded: the first triangle owns
    # a cell thinner than a pixel beside a proper one (S = 2, the middle column 0.2 pixel wide)
    pts = [[x, y] for y in (0.0, 8.0, 16.0) for x in (0.0, 11.4, 11.6)]
    ref = _both([_grid(pts, 16.0)], _uv(2), [oc.hash_frame(5)], WIDTH, HEIGHT, 1.0, 'thin')['best']
    assert (ref['count'][:, :11] == 1).all() and ref['count'][:, 11].sum() == 16          # centre 11.5 is in it
    pts = [[x, y] for y in (0.0, 8.0, 16.0) for x in (0.0, 11.6, 11.9)]
    ref = _both([_grid(pts, 16.0)], _uv(2), [oc.hash_frame(5)], WIDTH, HEIGHT, 1.0, 'thin, no centre')['best']
    rf = ref['frame']
    owner, _t, _a, _w = rs.cover(rf['X'][0], rf['Y'][0], 2, np.ones((2, 2), bool), rf['W'], rf['H'])
    assert owner.shape == (16, 12) and set(owner.reshape(-1).tolist()) == {0, 1, 4, 5}    # the thin cells own nothing
    # a NaN corner: S = 2, the cell that touches it is left out, three stay
    grid = _grid(_lattice(2, 0.0, 0.0, 20.0, 20.0), 20.0)
    grid[8] = np.nan
    ref = _both([grid, _grid(_lattice(2, 3.0, 3.0, 9.0, 9.0), 20.0)], _uv(2), [oc.hash_frame(6), oc.hash_frame(7)],
                WIDTH, HEIGHT, 1.0, 'NaN corner')['best']
    assert (ref['count'][10:, 10:] == 0).all() and (ref['count'][:10, :] >= 1).all() and ref['count'].max() == 2
    assert (ref['index'][10:, 10:] == -1).all() and (ref['bgr'][10:, 10:] == 0).all()


@pytest.mark.parametrize('size', [(1, 1), (15, 17), (16, 16), (17, 33)])
def test_mosaic_sizes_around_the_block(size):
    W, H = size
    for S in (1, 2):
        grid = _grid(_lattice(S, 0.0, 0.0, float(W), float(H)), float(H))
        ref = _both([grid], _uv(S), [oc.hash_frame(8)], WIDTH, HEIGHT, 1.0, '%d x %d S=%d' % (W, H, S))['best']
        assert ref['bgr'].shape == (H, W, 3) and (ref['count'] == 1).all()


@pytest.mark.parametrize('shape', [(1, 1), (2, 3), (64, 96)])
def test_sampling_on_texel_centres_and_small_frames(shape):
    """a raster of exactly the frame's size under a grid that maps it one to one: every pixel centre is
    a texel centre and the mosaic IS the frame; then the same grid at 4 pixels per texel"""
    from imageanalysis_amd import ortho
    h, w = shape
    frame = oc.hash_frame(9, h, w)
    grid = _grid(_lattice(1, 0.0, 0.0, float(w), float(h)), float(h))
    out = _both([grid], _uv(1), [frame], WIDTH, HEIGHT, 1.0, 'texel centres %d x %d' % (h, w))
    for ref in out.values():
        assert ref['bgr'].tobytes() == frame.tobytes()
    _both([grid], _uv(1), [frame], WIDTH, HEIGHT, 0.25, 'four per texel %d x %d' % (h, w))
    with pytest.raises(ValueError):
        ortho.compose([grid], _uv(1), [np.array(frame)], WIDTH, HEIGHT, 1.0)       # not a device tensor


def test_refusals_on_the_device_path():
    from imageanalysis_amd import ortho
    grid = _grid(_lattice(1, 0.0, 0.0, 8.0, 8.0), 8.0)
    frames = _dev([oc.hash_frame(1)])
    with pytest.raises(ValueError, match='mode'):
        ortho.compose([grid], _uv(1), frames, WIDTH, HEIGHT, 1.0, 'nearest')
    with pytest.raises(ValueError, match='frames'):
        ortho.compose([grid, grid], _uv(1), frames, WIDTH, HEIGHT, 1.0)
    with pytest.raises(MemoryError, match='GB of accumulators'):
        ortho.compose([grid], _uv(1), frames, WIDTH, HEIGHT, 1.0 / 100000)          # 800 000 pixels a side
    big = _grid(_lattice(33, 0.0, 0.0, 8.0, 8.0), 8.0)
    with pytest.raises(ValueError, match='at most 32'):
        ortho.compose([big], _uv(33), frames, WIDTH, HEIGHT, 1.0)


# ---- render(): a project's grids, frames=, and the three frame filters ----
@pytest.fixture(scope='module')
def project(tmp_path_factory):
    """the mid_default golden as a stand-in project with its matches_grouped on disk"""
    from imageanalysis_amd import render_panda3d as rp
    from imageanalysis_amd._deps import getNode
    directory = tmp_path_factory.mktemp('ortho_project')
    g = oc.golden('step5_mid_default')
    proj = s5.project(g, str(directory))
    (directory / 'matches_grouped').write_bytes(g['matches_in'])
    ref = getNode('/config/ned_reference', True)
    for k, v in (('lat_deg', 45.0), ('lon_deg', -93.0), ('alt_m', 280.0)):
        ref.setFloat(k, v)
    s5.set_switches(rp, g)
    yield proj, g
    s5.reset_switches(rp)


def _render(proj, g, **kw):
    from imageanalysis_amd import ortho
    with contextlib.redirect_stdout(io.StringIO()):
        return ortho.render(proj, g['groups'], 0, 0.5, **kw)


def test_render_a_project_end_to_end_and_save(project, tmp_path):
    """grids from map_grids on the device (within 1e-8 m of the recorded ones), frames through
    frames=; held to the restatement of the grids the call left on the images; tiles written"""
    import json
    from imageanalysis_amd import ortho
    proj, g = project
    names = list(g['groups'][0])
    frames = [oc.hash_frame(k) for k in range(len(names))]
    m = _render(proj, g, frames=_dev(frames), prefilter=False)
    grids = np.array([proj.findImageByName(n).grid_list for n in names], np.float64)
    assert np.abs(grids - oc.scene_input('step5_mid_default')[1]).max() <= 1e-8
    uv = np.array(proj.findImageByName(names[0]).distorted_uv, np.float64)
    _equal(m, rs.compose(grids, uv, frames, g['width'], g['height'], 0.5, 'best'), 'render mid_default')
    assert m.names == names and ortho.render_stats['images'] == 30 and ortho.render_stats['prefiltered'] == 0
    info = ortho.save(m, str(tmp_path), tile=256, fmt='png')
    assert len(info['tiles']) == 3 * 2 and info['images'] == names
    assert json.loads((tmp_path / 'ortho' / 'ortho.json').read_text())['bounds'] == info['bounds']
    with pytest.raises(ValueError, match='frames'):
        _render(proj, g, frames=_dev(frames[:3]))


@pytest.mark.parametrize('mode', MODES)
def test_prefilter_equals_rasterising_the_shrunk_frame(project, mode):
    from imageanalysis_amd import kernels, ortho
    proj, g = project
    names = list(g['groups'][0])
    _n, grids, _uv, _w, _h = oc.scene_input('step5_mid_default')
    frames = _dev([oc.hash_frame(k, 400, 600) for k in range(len(names))])
    got = _render(proj, g, frames=frames, mode=mode)                             # prefilter is the default
    assert ortho.render_stats['prefiltered'] == 30
    grids = np.array([proj.findImageByName(n).grid_list for n in names], np.float64)
    cells, _v = ortho.used_cells(grids)
    shrunk = []
    for k, f in enumerate(frames):
        fac = ortho.prefilter_factor(grids[k], cells[k], 600, 400, 0.5)
        assert fac < 0.75
        shrunk.append(kernels.resize_area(f, fac, fac))
    want = _render(proj, g, frames=shrunk, mode=mode, prefilter=False)
    assert ortho.render_stats['prefiltered'] == 0
    assert got.bgr.cpu().numpy().tobytes() == want.bgr.cpu().numpy().tobytes() and int(got.count.cpu().numpy().max()) >= 15
    plain = _render(proj, g, frames=frames, mode=mode, prefilter=False)
    assert plain.bgr.cpu().numpy().tobytes() != got.bgr.cpu().numpy().tobytes()     # (the filter did something)


def test_histogram_and_vignette_equal_rasterising_the_corrected_frame(project):
    from imageanalysis_amd import histogram, kernels, panda3d
    proj, g = project
    names = list(g['groups'][0])
    host = [oc.hash_frame(k) // 2 + 20 for k in range(len(names))]                 # (room for the mask below 255)
    frames = _dev(host)
    saved = histogram.histograms, histogram.templates
    try:
        histogram.histograms, histogram.templates = {}, {}
        for k, n in enumerate(names):
            h = [np.bincount(host[k][:, :, c].reshape(-1), minlength=256).astype(np.float32) for c in range(3)]
            histogram.histograms[n] = tuple(h)
            t = [np.cumsum(np.roll(x, 40 + k)) for x in h]
            histogram.templates[n] = tuple(x / x[-1] for x in t)
        histogram.templates[names[3]] = tuple(np.full(256, np.nan, np.float32) for _ in range(3))   # no neighbour
        want_frames = [f if k == 3 else kernels.colour_lut(f, histogram.lookup_tables(n))
                       for k, (f, n) in enumerate(zip(frames, names))]
        got = _render(proj, g, frames=frames, histogram=True, prefilter=False)
    finally:
        histogram.histograms, histogram.templates = saved
    want = _render(proj, g, frames=want_frames, prefilter=False)
    plain = _render(proj, g, frames=frames, prefilter=False).bgr.cpu().numpy().tobytes()
    assert got.bgr.cpu().numpy().tobytes() == want.bgr.cpu().numpy().tobytes() != plain

    import os
    models = os.path.join(proj.analysis_dir, 'models')
    os.makedirs(models, exist_ok=True)
    yy, xx = np.mgrid[0:oc.FRAME_H, 0:oc.FRAME_W]
    ramp = ((xx - 48) ** 2 + (yy - 32) ** 2) // 40
    mask_file = os.path.join(models, 'vignette-mask.jpg')
    with open(mask_file, 'wb') as fp:
        fp.write(panda3d.encode_jpeg(np.stack([ramp, ramp + 3, ramp + 6], 2).astype(np.uint8)))
    try:
        with open(mask_file, 'rb') as fp:
            mask = histogram._decode_frame(fp.read())
        identity = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
        want_frames = [kernels.colour_lut(f, identity, mask) for f in frames]
        got = _render(proj, g, frames=frames, vignette=True, prefilter=False)
    finally:
        os.remove(mask_file)
    want = _render(proj, g, frames=want_frames, prefilter=False)
    assert got.bgr.cpu().numpy().tobytes() == want.bgr.cpu().numpy().tobytes() != plain
    with pytest.raises(FileNotFoundError):
        _render(proj, g, frames=frames, vignette=True)


# ---- the command line: scripts/5c-ortho.py on a stand-in for the reference's lib package ----
LIB_STANDIN = {
    '__init__.py': '',
    'project.py': '''\
import os
import ortho_common as oc
import step5_common as s5
class ProjectMgr(object):
    """stand-in: the mid_default golden's poses and camera, frames under <project>/images"""
    def __init__(self, project_dir):
        self.project_dir = project_dir
        self.analysis_dir = os.path.join(project_dir, 'ImageAnalysis')
    def load_images_info(self):
        proj = s5.project(oc.golden('step5_mid_default'), self.analysis_dir)
        for im in proj.image_list:
            im.image_file = os.path.join(self.project_dir, 'images', im.name + '.JPG')
        self.image_list, self.findImageByName = proj.image_list, proj.findImageByName
''',
    'groups.py': '''\
import ortho_common as oc
def load(analysis_dir):
    return oc.golden('step5_mid_default')['groups']
''',
}


def test_script_writes_tiles_and_ortho_json(project, tmp_path):
    """5c-ortho.py in a process of its own: frames decoded from files by histogram.frame_pass; its
    tiles are the mosaic render() makes in this process from the same decoded frames"""
    import json
    import os
    import subprocess
    import sys
    from PIL import Image
    from imageanalysis_amd import image, panda3d
    proj, g = project
    names = list(g['groups'][0])
    lib = tmp_path / 'standin' / 'lib'
    lib.mkdir(parents=True)
    for name, text in LIB_STANDIN.items():
        (lib / name).write_text(text)
    pdir = tmp_path / 'project'
    (pdir / 'images').mkdir(parents=True)
    (pdir / 'ImageAnalysis').mkdir()
    (pdir / 'ImageAnalysis' / 'matches_grouped').write_bytes(g['matches_in'])
    decoded = []
    for k, n in enumerate(names):
        path = str(pdir / 'images' / (n + '.JPG'))
        with open(path, 'wb') as fp:
            fp.write(panda3d.encode_jpeg(np.array(oc.hash_frame(k))))
        decoded.append(image._decode_bgr(path))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / 'standin'), s5.REPO,
                                                       os.path.join(s5.REPO, 'tests')]))
    script = os.path.join(s5.REPO, 'imageanalysis_amd', 'scripts', '5c-ortho.py')
    cmd = ['timeout', '-k', '10', '120', sys.executable, script, str(pdir), '--gsd', '0.5', '--mode', 'feather',
           '--tile', '256', '--format', 'png']
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Mosaic: 617 x 492 pixels at 0.500 m, 30 images' in p.stdout and 'Wrote 6 tiles' in p.stdout
    out = pdir / 'ImageAnalysis' / 'ortho'
    info = json.loads((out / 'ortho.json').read_text())
    assert (info['mode'], info['gsd'], info['width'], info['height'], info['images']) == ('feather', 0.5, 617, 492, names)
    want = _render(proj, g, frames=_dev(decoded), mode='feather').bgr.cpu().numpy()
    assert (want.sum(axis=2) > 0).mean() > 0.5
    for t in info['tiles']:
        with Image.open(str(out / t['file'])) as im:
            px = np.asarray(im.convert('RGB'))[:, :, ::-1]
        r0, c0 = t['row'] * 256, t['col'] * 256
        assert px.tobytes() == want[r0:r0 + t['height'], c0:c0 + t['width']].tobytes(), t['file']
        assert (out / t['world_file']).is_file()
