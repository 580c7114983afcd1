"""GPU: csrc/dense_refine.hip and the guided form of csrc/dense_sweep.hip against
tests/dense_refine_restatement.py, bit for bit.  Outputs start poison-filled with guard elements behind
them, NaN sits behind every input plane."""
import numpy as np
import pytest
import torch

import dense_common as dc
import dense_refine_common as rc
import dense_refine_restatement as rr
import dense_restatement as dr
import dense_sgm_common as sc
from imageanalysis_amd import dense, kernels

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = {torch.int32: 0x5a5a5a5a, torch.float32: -12345.5}
SWEEP_NAMES = ('plane', 'score', 'depth', 'around')


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
            assert bool((buf[t.numel():] == POISON[buf.dtype]).all()), "a guard element was written"
        return [t.cpu().numpy() for t in self.out]


def behind_nan(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1)).cuda()
    buf = torch.full((t.numel() + GUARD,), float('nan'), dtype=t.dtype, device='cuda')
    buf[:t.numel()] = t
    return buf[:t.numel()].view(a.shape)


def device_views(views):
    G = behind_nan(np.stack([np.asarray(v.G, np.float32) for v in views]))
    return [dense.View(G[k], v.K, v.dist, v.R, v.C, rays=behind_nan(v.rays), name=v.name) for k, v in enumerate(views)]


def same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    bad = np.nonzero(dc.bits(got) != dc.bits(want))
    assert len(bad[0]) == 0, "%s differs at %d places, first %s: %r != %r" % (
        name, len(bad[0]), tuple(int(b[0]) for b in bad), got[tuple(b[0] for b in bad)], want[tuple(b[0] for b in bad)])


def sweep_outputs(h, w):
    return Guarded(((h, w), torch.int32), ((h, w), torch.float32), ((h, w), torch.float32), ((h, w, 3), torch.float32))


def run_guided(ref, nbs, total, windows, radius, **kw):
    views = device_views([ref] + list(nbs))
    h, w = ref.G.shape
    out = sweep_outputs(h, w)
    kernels.dense_sweep_guided(views[0], views[1:], dc.W_FAR, dc.W_NEAR, total, windows, radius=radius, out=out.out, **kw)
    return out.check()


def test_constant_matches_the_header():
    import re
    from imageanalysis_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r'#define IAMX_DENSE_GUIDED_MAX_PLANES (\d+)', text).group(1)) == kernels.DENSE_GUIDED_MAX_PLANES
    assert kernels.dense_tiles(17, 33) == rr.tiles(17, 33) == (2, 2)


@pytest.mark.parametrize('case', rc.guide_cases(), ids=lambda c: c[0])
def test_guide_against_the_restatement(case):
    _name, Dc, fine_hw, T, r, pad = case
    want = rr.guide(Dc, fine_hw, dc.W_FAR, dc.W_NEAR, T, radius=r, pad=pad)
    out = Guarded((want.shape, torch.int32))
    kernels.dense_guide(behind_nan(Dc), fine_hw, dc.W_FAR, dc.W_NEAR, T, radius=r, pad=pad, out=out.out[0])
    got, = out.check()
    assert np.array_equal(got, want)


def test_guided_sweep_on_the_roof_at_ratio_8():
    """128 x 96, r = 3, three neighbours, the table the guide makes of the coarse sweep, T = 97"""
    fv, _ = rc.scene('roof')
    windows, want = rc.guided('roof', 8)
    assert len(set(map(tuple, windows.reshape(-1, 2)))) > 4 and (want[0] >= 0).any()
    got = run_guided(fv[0], fv[1:], 97, windows, 3)
    for name, g, e in zip(SWEEP_NAMES, got, want):
        same(name, g, e)


@pytest.mark.parametrize('surface, w, h, focal, radius, n_nbr, total, pad', [
    ('slope', 70, 50, 47.0, 2, 1, 49, 4),
    ('roof', kernels.DENSE_TILE[0] + 1, kernels.DENSE_TILE[1] + 1, 22.0, 3, 3, 13, 1),
])
def test_guided_sweep_on_partial_tiles(surface, w, h, focal, radius, n_nbr, total, pad):
    """the table comes from the guide over the true depths at half the size (odd sizes: the coarse map is
    ceil(size / 2), which the guide's rule takes like any other)"""
    fv, truth = rc.scene(surface, h, w, focal)
    coarse = truth[0][::2, ::2].astype(np.float32)
    windows = rr.guide(coarse, (h, w), dc.W_FAR, dc.W_NEAR, total, radius=radius, pad=pad)
    assert (windows[..., 1] > 0).all() and (windows[..., 1] < total).any()
    want = rr.sweep_guided(fv[0], fv[1:1 + n_nbr], dc.W_FAR, dc.W_NEAR, total, windows, radius=radius)
    assert (want[0] >= 0).any() and np.isfinite(want[2]).any()
    got = run_guided(fv[0], fv[1:1 + n_nbr], total, windows, radius)
    for name, g, e in zip(SWEEP_NAMES, got, want):
        same(name, g, e)


def test_hand_made_table_and_the_window_edge_rule():
    """70 x 50 is 3 x 4 tiles.  Adjacent tiles hold: no plane; one plane; a window from 0; a window up to T;
    all T planes; two windows that do not overlap.  The slope's winners lie around planes 10 - 18 of 49, so the
    windows that stop inside that band clip peaks on both rims, and the rule drops them; the rims of the
    plane set itself are spared."""
    T = 49
    fv, _ = rc.scene('slope', 50, 70, 47.0)
    full = dr.sweep(fv[0], fv[1:3], dc.W_FAR, dc.W_NEAR, T, radius=2)
    won = full[0][np.isfinite(full[2])]
    lo, hi = int(np.percentile(won, 10)), int(np.percentile(won, 90))      # (10 and 18; the winners span 0 .. 21)
    mid = (lo + hi) // 2
    assert 2 < lo < mid < hi < T - 4
    windows = np.array([[(0, 0), (mid, 1), (0, mid + 1)],
                        [(mid, T - mid), (0, T), (lo - 2, mid - lo + 2)],
                        [(0, mid), (mid, hi + 3 - mid), (5, 0)],
                        [(0, mid), (mid, T - mid), (T - 1, 1)]], np.int32)
    assert windows.shape == rr.tiles(50, 70) + (2,)
    want = rr.sweep_guided(fv[0], fv[1:3], dc.W_FAR, dc.W_NEAR, T, windows, radius=2)
    got = run_guided(fv[0], fv[1:3], T, windows, 2)
    for name, g, e in zip(SWEEP_NAMES, got, want):
        same(name, g, e)
    plane, score, depth, around = got
    first, end = rr.per_pixel(windows, 50, 70)
    swept = plane >= 0
    assert ((plane >= first) & (plane < end))[swept].all()
    empty = end == first
    assert (plane[empty] == -1).all() and np.isnan(score[empty]).all() and np.isnan(around[empty]).all()
    with np.errstate(invalid='ignore'):
        good = swept & (score >= np.float32(0.6))
    on_low, on_high = good & (plane == first), good & (plane == end - 1)
    dropped_low, dropped_high = on_low & (first > 0), on_high & (end < T)
    assert dropped_low.sum() > 0 and dropped_high.sum() > 0
    assert np.isnan(depth[dropped_low | dropped_high]).all()
    spared = (on_low & (first == 0) & ~dropped_high) | (on_high & (end == T) & ~dropped_low)
    assert spared.sum() > 0 and np.isfinite(depth[spared]).all()
    assert np.isfinite(depth[good & ~dropped_low & ~dropped_high]).all()
    assert np.isnan(around[:, :, 0][swept & (plane == first)]).all()
    assert np.isnan(around[:, :, 2][swept & (plane == end - 1)]).all()
    # the one-plane tile: every swept pixel won on its only plane, a rim on both sides
    one = (end - first) == 1
    assert (plane[one & swept] == first[one & swept]).all() and np.isnan(depth[one & (first == mid)]).all()


@pytest.mark.parametrize('radius', [1, 7])
@pytest.mark.parametrize('T', [13, 2])
def test_full_windows_are_the_plain_sweep_on_the_device(radius, T):
    views, _ = dc.scene('roof', 29, 37)
    dv = device_views(views[:3])
    want = [t.cpu().numpy() for t in kernels.dense_sweep(dv[0], dv[1:], dc.W_FAR, dc.W_NEAR, T, radius=radius)]
    assert (want[0] >= 0).any()
    windows = np.zeros(rr.tiles(29, 37) + (2,), np.int32)
    windows[..., 1] = T
    got = run_guided(views[0], views[1:3], T, windows, radius)
    for name, g, e in zip(SWEEP_NAMES, got, want):
        same(name, g, e)


def test_the_entry_refuses_a_bad_table():
    """the C entry reads the table back and launches nothing: the poisoned outputs stay as they were"""
    from imageanalysis_amd import _lib
    views, _ = dc.scene('roof', 29, 37)
    dv = device_views(views[:2])
    pose = kernels._dev(kernels.dense_camera(dv[0])[:12], torch.float64)
    cam = kernels._dev(kernels.dense_camera(dv[1])[None], torch.float64)
    P = kernels._ptr
    for entry in ((0, 14), (-1, 3), (3, -1), (13, 1)):
        tab = np.zeros(rr.tiles(29, 37) + (2,), np.int32)
        tab[..., 1] = 13
        tab[1, 1] = entry
        d_tab = torch.from_numpy(tab).cuda()
        out = sweep_outputs(29, 37)
        rc_ = _lib.lib().iamx_dense_sweep_guided(P(dv[0].G), P(dv[0].rays), P(dv[1].G), P(pose), P(cam), 37, 29, 1, 13,
                                                 dc.W_FAR, dc.W_NEAR, 3, 4.0, 0.6, P(d_tab), *([P(t) for t in out.out] +
                                                                                             [_lib.stream_ptr()]))
        torch.cuda.synchronize()
        assert rc_ == -1 and b'window' in _lib.lib().iamx_last_error()
        for t in out.out:
            assert bool((t == POISON[t.dtype]).all())
        with pytest.raises(ValueError, match='window'):
            kernels.dense_sweep_guided(dv[0], dv[1:], dc.W_FAR, dc.W_NEAR, 13, d_tab)


# ---- dense.refine ----
@pytest.mark.parametrize('regularize', ['none', 'sgm'])
def test_refine_against_the_restatements(regularize):
    """the four views: depth_maps at 64 x 48, refine at 128 x 96 with ratio 4 -- against the same pipeline
    through the restatements, fed the device's coarse maps (which their own tests hold to their restatements)"""
    fv = rc.scene('roof')[0]
    cv = rc.coarse_scene('roof')
    ranges = [(dc.Z_NEAR, dc.Z_FAR)] * 4
    coarse = dense.depth_maps(device_views(cv), rc.NEIGHBOURS, ranges, planes=rc.COARSE_PLANES, regularize=regularize)
    assert bool(coarse.keep.any())
    maps = dense.refine(device_views(fv), rc.NEIGHBOURS, ranges, coarse, rc.COARSE_PLANES)
    want = rr.refine(fv, rc.NEIGHBOURS, ranges, coarse.depth.cpu().numpy(), coarse.keep.cpu().numpy(), rc.COARSE_PLANES)
    assert maps.total == want['total'] == 49
    assert np.array_equal(maps.windows.cpu().numpy(), want['windows'])
    count = want['windows'][..., 1]
    # (a tile on the image's border may be empty: the coarse check needs the neighbours to see it)
    assert (count[:, 1:-1, 1:-1] > 0).all() and count.mean() < 49 / 2.0
    for name in ('plane', 'score', 'depth', 'ned'):
        same(name, getattr(maps, name).cpu().numpy(), want[name])
    assert np.array_equal(maps.keep.cpu().numpy(), want['keep'])
    assert want['keep'].sum() > 0.5 * 4 * dc.interior(rc.H, rc.W, 3).sum()
    surface = dense.fuse(fv, maps, 1.0)
    assert int(surface.count.sum()) > 0 and bool(torch.isfinite(surface.dsm).any())
    xyz, grey = dense.surface_points(fv, maps)
    assert len(xyz) == len(grey) == int(want['keep'].sum())


def test_refine_chains_and_skips_views():
    """a second level from the first one's result; a view without neighbours, one without a range and one
    whose coarse map kept nothing get empty maps"""
    fv = rc.scene('slope')[0]
    cv = rc.coarse_scene('slope')
    nb = [[1], [0], [], [0]]
    ranges = [(dc.Z_NEAR, dc.Z_FAR)] * 3 + [None]
    coarse = dense.depth_maps(device_views(cv), nb, ranges, planes=rc.COARSE_PLANES)
    dfv = device_views(fv)
    one = dense.refine(dfv, nb, ranges, coarse, rc.COARSE_PLANES, ratio=3)
    assert one.total == 37 and bool(one.keep[0].any()) and bool(one.keep[1].any())

    def is_empty(maps, i):
        return (not maps.windows[i].any() and bool((maps.plane[i] == -1).all()) and bool(torch.isnan(maps.depth[i]).all())
                and bool(torch.isnan(maps.score[i]).all()) and not maps.keep[i].any())

    assert is_empty(one, 2) and is_empty(one, 3)
    two = dense.refine(dfv, nb, ranges, one, one.total, ratio=2, check=False)
    want = rr.refine(fv, nb, ranges, one.depth.cpu().numpy(), one.keep.cpu().numpy(), 37, ratio=2)
    assert two.total == 73 and np.array_equal(two.windows.cpu().numpy(), want['windows'])
    same('depth', two.depth.cpu().numpy(), want['depth'])
    assert np.isfinite(want['depth'][:2]).any() and is_empty(two, 2) and is_empty(two, 3)
    assert np.array_equal(two.keep.cpu().numpy(), np.isfinite(want['depth']).astype(np.uint8))
    blind = dense.DepthMaps(depth=coarse.depth, keep=coarse.keep.clone())
    blind.keep[1] = 0
    three = dense.refine(dfv, nb, ranges, blind, rc.COARSE_PLANES, ratio=3)
    assert is_empty(three, 1) and bool(torch.isfinite(three.depth[0]).any()) and not three.keep[0].any()


# ---- the command line ----
@pytest.fixture(scope='module')
def script_project(tmp_path_factory):
    """the stand-in project on disk -> (proj, matches, decoded frames, the script's command, its environment, cwd)"""
    import os
    import pickle
    import sys
    from conftest import REPO
    from imageanalysis_amd import image, panda3d
    tmp_path = tmp_path_factory.mktemp('dense_refine_script')
    lib = tmp_path / 'standin' / 'lib'
    lib.mkdir(parents=True)
    for name, text in sc.LIB_STANDIN.items():
        (lib / name).write_text(text)
    pdir = tmp_path / 'project'
    (pdir / 'images').mkdir(parents=True)
    (pdir / 'ImageAnalysis').mkdir()
    proj = dc.standin_project(str(pdir / 'ImageAnalysis'))
    frames, matches = dc.project_frames(proj), dc.project_matches(proj)
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
           '--gsd', '1.0', '--scale', '0.25', '--ply']
    return proj, matches, decoded, cmd, env, tmp_path


def test_script_refines(script_project):
    """5d-dense-surface.py --refine 1 in a process of its own: its raster is the one this process makes
    from the same decoded frames through depth_maps and refine, and dense.json names the levels"""
    import json
    import subprocess
    proj, matches, decoded, cmd, env, tmp_path = script_project
    p = subprocess.run(cmd + ['--refine', '1', '--refine-ratio', '3'], capture_output=True, text=True, env=env,
                       cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Views: 4 of 64 x 48 pixels' in p.stdout and 'Level 1: 128 x 96 pixels, 37 planes' in p.stdout
    out = tmp_path / 'project' / 'ImageAnalysis' / 'dense'
    info = json.loads((out / 'dense.json').read_text())
    assert list(info)[-3:] == ['refine', 'ratio', 'planes_total']
    assert (info['refine'], info['ratio'], info['planes_total']) == (1, 3, 37)
    for name in ('dsm.npy', 'count.npy', 'dsm.wld', 'points.ply'):
        assert (out / name).is_file()
    levels = []
    for scale in (0.125, 0.25):
        levels.append(dense.views_from_project(proj, [dc.NAMES], 0, matches, scale,
                                               frames=[torch.from_numpy(f).cuda() for f in decoded]))
    (cviews, group), (fviews, _) = levels
    poses = [(v.R, v.C) for v in cviews]
    neighbours = dense.choose_neighbours(matches, group, poses, n=3)
    ranges = dense.depth_range(matches, group, poses)
    coarse = dense.depth_maps(cviews, neighbours, ranges, planes=dc.PLANES)
    maps = dense.refine(fviews, neighbours, ranges, coarse, dc.PLANES, ratio=3)
    surface = dense.fuse(fviews, maps, 1.0)
    assert (info['gsd'], info['height'], info['width']) == (1.0,) + surface.shape
    same('dsm', np.load(str(out / 'dsm.npy')), surface.dsm.cpu().numpy())
    assert info['points'] == int(maps.keep.sum()) > 4000
    bad = subprocess.run(cmd + ['--refine', '1', '--refine-ratio', '0'], capture_output=True, text=True, env=env,
                         cwd=str(tmp_path))
    assert bad.returncode == 2 and 'ratio' in bad.stderr


def test_script_without_refine_has_none_of_the_keys(script_project):
    import json
    import subprocess
    _proj, _matches, _decoded, cmd, env, tmp_path = script_project
    q = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert q.returncode == 0, q.stderr[-3000:]
    plain = json.loads((tmp_path / 'project' / 'ImageAnalysis' / 'dense' / 'dense.json').read_text())
    assert not {'refine', 'ratio', 'planes_total', 'regularize'} & set(plain) and 'Level' not in q.stdout
    assert 'Views: 4 of 128 x 96 pixels' in q.stdout and list(plain)[-1] == 'points'
