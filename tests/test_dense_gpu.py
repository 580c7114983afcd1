"""GPU: csrc/dense_sweep.hip against tests/dense_restatement.py, bit for bit.  Outputs start
poison-filled with guard elements behind them, NaN sits behind every input plane."""
import functools

import numpy as np
import pytest
import torch

import dense_common as dc
import dense_restatement as dr
from imageanalysis_amd import dense, kernels

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = {torch.int32: 0x5a5a5a5a, torch.int64: 0x5a5a5a5a5a5a5a5a, torch.uint8: 0x5a, torch.float32: -12345.5,
          torch.float64: -12345.5}


def behind_nan(a):
    """numpy float array -> its device copy with GUARD NaNs behind it"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1)).cuda()
    buf = torch.full((t.numel() + GUARD,), float('nan'), dtype=t.dtype, device='cuda')
    buf[:t.numel()] = t
    return buf[:t.numel()].view(a.shape)


def device_views(views):
    """the views on the device: the grey planes consecutive in one buffer, NaN behind it and the rays"""
    G = behind_nan(np.stack([np.asarray(v.G, np.float32) for v in views]))
    return [dense.View(G[k], v.K, v.dist, v.R, v.C, rays=behind_nan(v.rays), name=v.name)
            for k, v in enumerate(views)]


class Guarded(object):
    """poison-filled output tensors, each with GUARD poison elements behind it"""

    def __init__(self, *specs):
        self.bufs, self.out = [], []
        for shape, dtype in specs:
            n = int(np.prod(shape))
            buf = torch.full((n + GUARD,), POISON[dtype], dtype=dtype, device='cuda')
            self.bufs.append(buf)
            self.out.append(buf[:n].view(shape))

    def check(self):
        for buf, t in zip(self.bufs, self.out):
            tail = buf[t.numel():]
            assert bool((tail == POISON[buf.dtype]).all()), "a guard element was written"
        return [t.cpu().numpy() for t in self.out]


def sweep_outputs(h, w):
    return Guarded(((h, w), torch.int32), ((h, w), torch.float32), ((h, w), torch.float32), ((h, w, 3), torch.float32))


def assert_same_sweep(got, want):
    for name, g, e in zip(('plane', 'score', 'depth', 'around'), got, want):
        assert g.dtype == e.dtype and g.shape == e.shape, name
        bad = np.nonzero(dc.bits(g) != dc.bits(e))
        assert len(bad[0]) == 0, "%s differs at %d places, first %s: %r != %r" % (
            name, len(bad[0]), tuple(int(b[0]) for b in bad), g[tuple(b[0] for b in bad)], e[tuple(b[0] for b in bad)])


def run_sweep(ref, nbs, planes, radius, **kw):
    views = device_views([ref] + list(nbs))
    h, w = ref.G.shape
    out = sweep_outputs(h, w)
    kernels.dense_sweep(views[0], views[1:], dc.W_FAR, dc.W_NEAR, planes, radius=radius, out=out.out, **kw)
    return out.check()


TILE_W, TILE_H = kernels.DENSE_TILE


def test_constants_match_the_header():
    import re
    from imageanalysis_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    d = dict((k, int(v)) for k, v in re.findall(r'#define IAMX_DENSE_(\w+) (\d+)', text))
    assert (d['TILE_W'], d['TILE_H']) == kernels.DENSE_TILE
    assert (d['MAX_RADIUS'], d['MAX_PLANES'], d['MAX_NEIGHBOURS'], d['MAX_SIDE']) == (
        kernels.DENSE_MAX_RADIUS, kernels.DENSE_MAX_PLANES, kernels.DENSE_MAX_NEIGHBOURS, kernels.DENSE_MAX_SIDE)
    assert d['CAM_DOUBLES'] == len(kernels.dense_camera(dc.scene('slope')[0][0]))


@pytest.mark.parametrize('surface, w, h, radius, planes, n_nbr', [
    ('slope', 64, 48, 3, 13, 3),
    ('roof', 64, 48, 3, 13, 3),
    ('roof', 64, 48, 2, 13, 1),
    ('slope', 64, 48, 2, 1, 3),
    ('slope', 37, 29, 3, 2, 3),
    ('roof', 37, 29, 2, 13, 1),
    ('roof', 37, 29, 3, 1, 1),
    ('slope', TILE_W + 1, TILE_H + 1, 3, 13, 3),
    ('roof', TILE_W + 1, TILE_H + 1, 2, 2, 1),
])
def test_sweep_against_the_restatement(surface, w, h, radius, planes, n_nbr):
    views, _ = dc.scene(surface, h, w)
    ref, nbs = views[0], views[1:1 + n_nbr]
    want = dr.sweep(ref, nbs, dc.W_FAR, dc.W_NEAR, planes, radius=radius)
    assert (want[0] >= 0).any() and np.isfinite(want[2]).any()
    assert_same_sweep(run_sweep(ref, nbs, planes, radius), want)


@pytest.mark.parametrize('radius', [1, 4, 5, 6, 7])
def test_every_radius_has_its_kernel(radius):
    views, _ = dc.scene('roof', 37, 29)
    want = dr.sweep(views[0], views[1:3], dc.W_FAR, dc.W_NEAR, 3, radius=radius)
    assert (want[0] >= 0).any()
    assert_same_sweep(run_sweep(views[0], views[1:3], 3, radius), want)


def test_thresholds_are_parameters():
    views, _ = dc.scene('roof')
    kw = dict(min_var=60.0, min_score=0.9)
    want = dr.sweep(views[0], views[1:], dc.W_FAR, dc.W_NEAR, 5, radius=2, **kw)
    base = dr.sweep(views[0], views[1:], dc.W_FAR, dc.W_NEAR, 5, radius=2)
    assert (want[0] < 0).sum() > (base[0] < 0).sum() and np.isnan(want[2]).sum() > np.isnan(base[2]).sum()
    assert_same_sweep(run_sweep(views[0], views[1:], 5, 2, **kw), want)


def test_out_of_view_neighbour():
    """a neighbour 75 m to the east: about half of the warps leave its image, so validity changes
    inside windows, inside tiles and along the image's edge"""
    views, _ = dc.scene('slope')
    far, _ = dc.make_view('slope', 1, centre=(0.0, 75.0))
    for nbs in ([far], [views[2], far]):
        want = dr.sweep(views[0], nbs, dc.W_FAR, dc.W_NEAR, dc.PLANES, radius=3)
        if len(nbs) == 1:
            valid = int((want[0] >= 0).sum())
            assert 0.25 * dc.W * dc.H < valid < 0.75 * dc.interior(dc.H, dc.W, 3).sum()
        assert_same_sweep(run_sweep(views[0], nbs, dc.PLANES, 3), want)


def test_tie_goes_to_the_first_plane():
    """A neighbour with the reference's own pose and image warps to the same samples on every plane:
    every valid score is the same and plane 0 wins.  (The samples of the image's outermost pixels
    lie on the validity bound, 0 or w - 1 up to a rounding, so the windows that hold them -- the
    outermost ring of valid pixels -- are valid on some planes only; the tie is asserted inside it.)"""
    views, _ = dc.scene('roof')
    ref = views[0]
    want = dr.sweep(ref, [ref], dc.W_FAR, dc.W_NEAR, dc.PLANES, radius=3)
    got = run_sweep(ref, [ref], dc.PLANES, 3)
    assert_same_sweep(got, want)
    plane, score, depth, around = got
    inner = dc.interior(dc.H, dc.W, 4) & (plane >= 0)
    assert inner.sum() > 0.8 * dc.interior(dc.H, dc.W, 4).sum()
    assert (plane[inner] == 0).all()
    assert np.array_equal(around[inner][:, 1], around[inner][:, 2]) and np.isnan(around[inner][:, 0]).all()
    assert np.array_equal(dc.bits(depth[inner]), dc.bits(np.full(int(inner.sum()), dc.Z_FAR, np.float32)))


def test_flat_grey_reference():
    views, _ = dc.scene('slope')
    flat = dense.View(np.full((dc.H, dc.W), 128.0, np.float32), views[0].K, views[0].dist, views[0].R, views[0].C,
                      rays=views[0].rays)
    plane, score, depth, around = run_sweep(flat, views[1:], dc.PLANES, 3)
    assert (plane == -1).all() and np.isnan(depth).all() and np.isnan(score).all() and np.isnan(around).all()
    assert_same_sweep((plane, score, depth, around), dr.sweep(flat, views[1:], dc.W_FAR, dc.W_NEAR, dc.PLANES, radius=3))


# ---- consistency and fusion ----
NEIGHBOURS = [[1, 2, 3], [0, 2, 3], [0, 1], [0]]


@functools.lru_cache(maxsize=None)
def restated_maps(surface):
    """the restatement's depth maps of the four views, each against NEIGHBOURS -> (views, depths)"""
    views, _ = dc.scene(surface)
    depths = np.stack([dr.sweep(views[i], [views[j] for j in NEIGHBOURS[i]], dc.W_FAR, dc.W_NEAR, dc.PLANES)[2]
                       for i in range(len(views))])
    return views, depths


@pytest.mark.parametrize('surface, eps, min_agree', [('roof', 0.01, 2), ('slope', 0.01, 2), ('roof', 0.002, 1),
                                                     ('slope', 0.05, 3)])
def test_check_against_the_restatement(surface, eps, min_agree):
    views, depths = restated_maps(surface)
    want_keep, want_ned = dr.check(depths, views, NEIGHBOURS, eps, min_agree)
    assert 0 < want_keep.sum() < np.isfinite(depths).sum()
    assert want_keep[3].any()                              # (one neighbour: one agreement is enough)
    dviews = device_views(views)
    d_depths = behind_nan(depths)
    runs = []
    for _ in range(2):
        out = Guarded((depths.shape, torch.uint8), (depths.shape + (3,), torch.float64))
        kernels.dense_check(d_depths, dviews, NEIGHBOURS, eps=eps, min_agree=min_agree, out=out.out)
        runs.append(out.check())
    for keep, ned in runs:
        assert np.array_equal(keep, want_keep)
        assert np.array_equal(dc.bits(ned), dc.bits(want_ned))


def test_check_without_neighbours_keeps_nothing():
    views, depths = restated_maps('slope')
    keep, _ = kernels.dense_check(depths[:2], device_views(views[:2]), [[1], []])
    want, _ = dr.check(depths[:2], views[:2], [[1], []])
    assert np.array_equal(keep.cpu().numpy(), want) and not want[1].any() and want[0].any()


def _splat_cases():
    rng = np.random.default_rng(3)
    x0, y1, gsd, W, H = -4.0, 6.0, 0.5, 20, 12
    crowd = np.stack([rng.uniform(1.0, 1.5, 5000), rng.uniform(2.0, 2.5, 5000), rng.normal(-3, 5, 5000)], 1)
    c, r = np.meshgrid(np.arange(-1, W + 2), np.arange(-1, H + 2))
    edges = np.stack([(y1 - r * gsd).ravel(), (x0 + c * gsd).ravel(), -np.linspace(0, 9, c.size)], 1)
    cloud = np.stack([rng.uniform(-3, 9, 3000), rng.uniform(-8, 10, 3000), rng.normal(-50, 20, 3000)], 1)
    odd = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, 0, -np.inf], [0, 0, 1e14],
                    [1e300, 1e300, 0], [-1e300, -1e300, 0], [0.25, 0.25, -7.0004883]])
    frame = (x0, y1, gsd, W, H)
    return [('crowd', crowd, None, frame), ('edges', edges, None, frame),
            ('outside', np.concatenate([cloud, odd]), None, frame),
            ('kept', cloud, (rng.uniform(size=3000) < 0.4).astype(np.uint8), frame),
            ('one cell', crowd, None, (2.0, 1.5, 0.75, 1, 1))]


@pytest.mark.parametrize('case', _splat_cases(), ids=lambda c: c[0])
def test_splat_against_the_restatement(case):
    _name, pts, keep, (x0, y1, gsd, W, H) = case
    want = dr.splat(pts, keep, x0, y1, gsd, W, H)
    assert want[0].sum() > 0
    if _name == 'crowd':
        assert want[0].max() == 5000
    if _name in ('edges', 'outside'):
        assert want[0].sum() < len(pts)
    d_pts = behind_nan(pts)
    runs = []
    for _ in range(2):
        out = Guarded(((H, W), torch.int32), ((H, W), torch.int64), ((H, W), torch.float32))
        kernels.dense_splat(d_pts, keep, x0, y1, gsd, W, H, out=out.out)
        runs.append(out.check())
    for count, total, dsm in runs:
        assert np.array_equal(count, want[0]) and np.array_equal(total, want[1])
        assert np.array_equal(dc.bits(dsm), dc.bits(want[2]))


def test_depth_maps_and_fuse_on_the_slope():
    views, want_depths = restated_maps('slope')
    ranges = [(dc.Z_NEAR, dc.Z_FAR)] * len(views)
    maps = dense.depth_maps(device_views(views), NEIGHBOURS, ranges, planes=dc.PLANES)
    assert np.array_equal(dc.bits(maps.depth.cpu().numpy()), dc.bits(want_depths))
    keep, ned = dr.check(want_depths, views, NEIGHBOURS)
    assert np.array_equal(maps.keep.cpu().numpy(), keep)
    gsd = 2.0
    surface = dense.fuse(views, maps, gsd)
    alive = ned[keep != 0]
    x0, y1, W, H = dense.frame_of(alive[:, 1].min(), alive[:, 1].max(), alive[:, 0].min(), alive[:, 0].max(), gsd)
    count, _total, dsm = dr.splat(ned, keep, x0, y1, gsd, W, H)
    assert (surface.x0, surface.y1, surface.gsd, surface.shape) == (x0, y1, gsd, (H, W))
    got = surface.dsm.cpu().numpy()
    assert np.array_equal(surface.count.cpu().numpy(), count) and np.array_equal(dc.bits(got), dc.bits(dsm))
    # the height one plane step spans at the surface's depth under a nadir camera: z^2 step
    filled = count > 0
    assert filled.sum() > 0.5 * filled.size
    r, c = np.nonzero(filled)
    north, east = y1 - (r + 0.5) * gsd, x0 + (c + 0.5) * gsd
    up = -(0.15 * north + 0.1 * east)
    bound = dr.plane_step(dc.W_FAR, dc.W_NEAR, dc.PLANES) * (dc.ALTITUDE - up) ** 2
    err = np.abs(got[filled] - up)
    print('dsm: %d of %d cells, worst error %.2f m of a bound of %.2f m, median %.2f m'
          % (filled.sum(), filled.size, err.max(), bound[err.argmax()], np.median(err)))
    assert (err <= bound).all()


def test_save_writes_the_raster(tmp_path):
    views, depths = restated_maps('slope')
    keep, ned = dr.check(depths, views, NEIGHBOURS)
    maps = dense.DepthMaps(depth=torch.from_numpy(depths).cuda(), keep=torch.from_numpy(keep).cuda(),
                           ned=torch.from_numpy(ned).cuda())
    surface = dense.fuse(views, maps, 2.5)
    info = dense.save(surface, str(tmp_path), points=dense.surface_points(views, maps))
    out = tmp_path / 'dense'
    dsm, count = np.load(out / 'dsm.npy'), np.load(out / 'count.npy')
    assert dsm.dtype == np.float32 and count.dtype == np.int32 and dsm.shape == count.shape == surface.shape
    assert np.array_equal(np.isnan(dsm), count == 0) and info['points'] == int(keep.sum()) == int(count.sum())
    lines = (out / 'dsm.wld').read_text().split()
    assert [float(x) for x in lines] == [2.5, 0.0, 0.0, -2.5, surface.x0 + 1.25, surface.y1 - 1.25]
    blob = (out / 'points.ply').read_bytes()
    assert len(blob.split(b'end_header\n', 1)[1]) == 13 * info['points']
    assert (out / 'dense.json').exists()


# ---- a project: views_from_project, neighbours and ranges from its chains, the command line ----
@pytest.fixture(scope='module')
def project(tmp_path_factory):
    directory = tmp_path_factory.mktemp('dense_project')
    proj = dc.standin_project(str(directory))
    return proj, dc.project_frames(proj), dc.project_matches(proj)


def _pipeline(proj, frames, matches):
    views, group = dense.views_from_project(proj, [dc.NAMES], 0, matches, 1.0 / dc.FULL,
                                            frames=[torch.from_numpy(f).cuda() for f in frames])
    poses = [(v.R, v.C) for v in views]
    neighbours = dense.choose_neighbours(matches, group, poses, n=3)
    ranges = dense.depth_range(matches, group, poses)
    maps = dense.depth_maps(views, neighbours, ranges, planes=dc.PLANES)
    return views, neighbours, ranges, maps, dense.fuse(views, maps, 2.0)


def test_views_from_project_and_the_surface(project):
    proj, frames, matches = project
    views, neighbours, ranges, maps, surface = _pipeline(proj, frames, matches)
    assert [v.name for v in views] == dc.NAMES and all(tuple(v.G.shape) == (dc.H, dc.W) for v in views)
    assert np.allclose(views[0].K, [dc.FOCAL, dc.FOCAL, (dc.W - 1) / 2.0, (dc.H - 1) / 2.0], rtol=0, atol=1e-12)
    for v, im, f in zip(views, proj.image_list, frames):
        R, C = dense.image_pose(im)
        assert np.array_equal(v.R, R) and np.array_equal(v.C, C) and abs(np.linalg.det(R) - 1) < 1e-12
        assert R[2, 2] > 0.99                                  # (the camera looks down)
        blocks = f[:, :, 0].astype(np.float64).reshape(dc.H, dc.FULL, dc.W, dc.FULL).mean(axis=(1, 3))
        G = v.G.cpu().numpy()
        assert G.dtype == np.float32 and np.array_equal(G, np.rint(G)) and np.abs(G - blocks).max() <= 0.5 + 1e-9
    assert np.abs(views[0].rays.cpu().numpy() - dc.host_rays(views[0].K, dc.DIST, dc.H, dc.W)).max() < 1e-5
    assert all(len(n) >= 2 and i not in n for i, n in enumerate(neighbours))
    assert all(r is not None and 70.0 < r[0] < 95.0 and 105.0 < r[1] < 135.0 for r in ranges)
    # the restatement on the same views
    host = [dense.View(v.G.cpu().numpy(), v.K, v.dist, v.R, v.C, rays=v.rays.cpu().numpy()) for v in views]
    depths = np.stack([dr.sweep(host[i], [host[j] for j in neighbours[i]], 1.0 / ranges[i][1], 1.0 / ranges[i][0],
                                dc.PLANES)[2] for i in range(len(host))])
    assert np.array_equal(dc.bits(maps.depth.cpu().numpy()), dc.bits(depths))
    keep, ned = dr.check(depths, host, neighbours)
    alive = ned[keep != 0]
    x0, y1, W, H = dense.frame_of(alive[:, 1].min(), alive[:, 1].max(), alive[:, 0].min(), alive[:, 0].max(), 2.0)
    count, _total, dsm = dr.splat(ned, keep, x0, y1, 2.0, W, H)
    got = surface.dsm.cpu().numpy()
    assert surface.shape == (H, W) and np.array_equal(dc.bits(got), dc.bits(dsm))
    filled = count > 0
    r, c = np.nonzero(filled)
    up = -(0.15 * (y1 - (r + 0.5) * 2.0) + 0.1 * (x0 + (c + 0.5) * 2.0))
    step = max(dr.plane_step(1.0 / zf, 1.0 / zn, dc.PLANES) for zn, zf in ranges)
    err = np.abs(got[filled] - up)
    print('project dsm: %d of %d cells, worst error %.2f m, median %.2f m' % (filled.sum(), filled.size, err.max(), np.median(err)))
    assert filled.sum() > 0.3 * filled.size and (err <= step * (dc.ALTITUDE - up) ** 2).all()


LIB_STANDIN = {
    '__init__.py': '',
    'project.py': '''\
import os
import dense_common as dc
class ProjectMgr(object):
    """stand-in: the four cameras over the slope, frames under <project>/images"""
    def __init__(self, project_dir):
        self.project_dir = project_dir
        self.analysis_dir = os.path.join(project_dir, 'ImageAnalysis')
    def load_images_info(self):
        proj = dc.standin_project(self.analysis_dir, os.path.join(self.project_dir, 'images'))
        self.image_list = proj.image_list
''',
    'groups.py': '''\
import dense_common as dc
def load(analysis_dir):
    return [list(dc.NAMES)]
''',
}


def test_script_writes_the_surface(project, tmp_path):
    """5d-dense-surface.py in a process of its own, frames decoded from files by histogram.frame_pass;
    its raster is the one this process makes from the same decoded frames"""
    import json
    import os
    import pickle
    import subprocess
    import sys
    from conftest import REPO
    from imageanalysis_amd import image, panda3d
    proj, frames, matches = project
    lib = tmp_path / 'standin' / 'lib'
    lib.mkdir(parents=True)
    for name, text in LIB_STANDIN.items():
        (lib / name).write_text(text)
    pdir = tmp_path / 'project'
    (pdir / 'images').mkdir(parents=True)
    (pdir / 'ImageAnalysis').mkdir()
    with open(str(pdir / 'ImageAnalysis' / 'matches_grouped'), 'wb') as fp:
        pickle.dump(matches, fp)
    decoded = []
    for n, f in zip(dc.NAMES, frames):
        path = str(pdir / 'images' / (n + '.JPG'))
        with open(path, 'wb') as fp:
            fp.write(panda3d.encode_jpeg(f))
        decoded.append(image._decode_bgr(path))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / 'standin'), REPO, os.path.join(REPO, 'tests')]))
    script = os.path.join(REPO, 'imageanalysis_amd', 'scripts', '5d-dense-surface.py')
    cmd = ['timeout', '-k', '10', '120', sys.executable, script, str(pdir), '--planes', str(dc.PLANES), '--neighbors', '3',
           '--gsd', '2.0', '--ply']
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Views: 4 of 64 x 48 pixels, 4 with neighbours' in p.stdout and 'Wrote' in p.stdout
    out = pdir / 'ImageAnalysis' / 'dense'
    info = json.loads((out / 'dense.json').read_text())
    *_rest, maps, surface = _pipeline(proj, decoded, matches)
    want = surface.dsm.cpu().numpy()
    assert (info['gsd'], info['height'], info['width']) == (2.0,) + want.shape
    assert np.array_equal(dc.bits(np.load(str(out / 'dsm.npy'))), dc.bits(want))
    assert np.array_equal(np.load(str(out / 'count.npy')), surface.count.cpu().numpy())
    assert info['points'] == int(maps.keep.sum()) > 1000 and (out / 'points.ply').is_file() and (out / 'dsm.wld').is_file()
