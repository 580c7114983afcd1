"""GPU: csrc/dense_sgm.hip and the cost emission of csrc/dense_sweep.hip against
tests/dense_sgm_restatement.py, bit for bit.  Outputs start poison-filled with guard elements behind
them; the inputs sit in buffers of their own with a guard behind them too."""
import functools

import numpy as np
import pytest
import torch

import dense_common as dc
import dense_restatement as dr
import dense_sgm_common as sc
import dense_sgm_restatement as ds
from imageanalysis_amd import dense, kernels

pytestmark = pytest.mark.gpu

GUARD = 128
POISON = {torch.int32: 0x5a5a5a5a, torch.uint8: 0x5a, torch.int16: 0x5a5a, torch.float32: -12345.5,
          torch.float64: -12345.5}


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


def behind_guard(a, fill):
    """numpy array -> its device copy with GUARD elements of `fill` behind it"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1)).cuda()
    buf = torch.full((t.numel() + GUARD,), fill, dtype=t.dtype, device='cuda')
    buf[:t.numel()] = t
    return buf[:t.numel()].view(a.shape)


def device_views(views):
    G = behind_guard(np.stack([np.asarray(v.G, np.float32) for v in views]), float('nan'))
    return [dense.View(G[k], v.K, v.dist, v.R, v.C, rays=behind_guard(v.rays, float('nan')), name=v.name)
            for k, v in enumerate(views)]


def u16(a):
    """the int16 bits of a device total as the uint16 they are"""
    return np.ascontiguousarray(a).view(np.uint16)


def same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    bad = np.nonzero(dc.bits(got) != dc.bits(want))
    assert len(bad[0]) == 0, "%s differs at %d places, first %s: %r != %r" % (
        name, len(bad[0]), tuple(int(b[0]) for b in bad), got[tuple(b[0] for b in bad)], want[tuple(b[0] for b in bad)])


def test_constants_match_the_header():
    import re
    from imageanalysis_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r'#define IAMX_DENSE_SGM_MAX_PLANES (\d+)', text).group(1)) == kernels.DENSE_SGM_MAX_PLANES == 64
    assert kernels.DENSE_SGM_DIRECTIONS == ds.DIRECTIONS


# ---- the sweep's cost volume ----
def far_east():
    """a neighbour 75 m to the east: about half of its warps leave the image, 255s inside tiles"""
    return dc.make_view('slope', 1, centre=(0.0, 75.0))[0]


SWEEPS = [('roof', 37, 29, 2, 5, 1), ('slope', 33, 17, 3, 13, 3), ('roof', 64, 48, 3, 64, 2), ('slope', 37, 29, 3, 2, 3),
          ('far-east', 64, 48, 3, 13, 2), ('far-east', 64, 48, 3, 6, 1)]


@pytest.mark.parametrize('surface, w, h, radius, planes, n_nbr', SWEEPS)
def test_sweep_volume_against_the_restatement(surface, w, h, radius, planes, n_nbr):
    if surface == 'far-east':
        views, _ = dc.scene('slope', h, w)
        ref, nbs = views[0], [far_east()] + views[2:1 + n_nbr]
    else:
        views, _ = dc.scene(surface, h, w)
        ref, nbs = views[0], views[1:1 + n_nbr]
    want = dr.sweep(ref, nbs, dc.W_FAR, dc.W_NEAR, planes, radius=radius)
    want_vol = ds.volume(ref, nbs, dc.W_FAR, dc.W_NEAR, planes, radius)
    assert (want_vol == 255).any() and (want_vol < 255).any()
    if surface == 'far-east':
        inner = want_vol[8:-8, 8:-8]
        assert 0.05 < (inner == 255).mean() < 0.8            # validity changes inside the image, inside tiles
    dviews = device_views([ref] + list(nbs))
    out = Guarded(((h, w), torch.int32), ((h, w), torch.float32), ((h, w), torch.float32), ((h, w, 3), torch.float32),
                  ((h, w, planes), torch.uint8))
    kernels.dense_sweep(dviews[0], dviews[1:], dc.W_FAR, dc.W_NEAR, planes, radius=radius, out=out.out[:4],
                        volume=out.out[4])
    got = out.check()
    for name, g, e in zip(('plane', 'score', 'depth', 'around'), got, want):
        same(name, g, e)
    same('volume', got[4], want_vol)
    # the winner's score is the volume's smallest cost, wherever there is a winner
    has = want[0] >= 0
    assert np.array_equal(got[4].min(axis=2)[has], ds.cost_of(want[1])[has]) and (got[4][~has] == 255).all()


# ---- the paths ----
def synthetic_volume(h, w, planes, seed=0):
    rng = np.random.default_rng(1000 * h + 10 * w + planes + seed)
    vol = rng.integers(0, 255, (h, w, planes), dtype=np.uint8)
    smooth = (40 + 30 * np.sin(np.arange(w) / 5.0)[None, :, None] + 3.0 * np.abs(np.arange(planes)[None, None, :] - planes / 2.0)
              + 10 * np.cos(np.arange(h) / 3.0)[:, None, None])
    vol = np.where(rng.uniform(size=vol.shape) < 0.5, np.clip(smooth, 0, 254).astype(np.uint8), vol)
    vol[rng.uniform(size=vol.shape) < 0.1] = 255
    vol[rng.uniform(size=(h, w)) < 0.05] = 255               # pixels without a valid plane
    vol[0, 0, 0], vol[h - 1, w - 1, planes - 1] = 255, 3
    return vol


PATH_SHAPES = [(1, 1, 2), (1, 70, 64), (70, 1, 3), (3, 65, 5), (65, 3, 17), (29, 37, 64), (48, 64, 13)]
PENALTIES = [(0, 0), (8, 8), (8, 64), (255, 255)]


def run_paths(vol, paths, p1, p2, c_invalid=127, direction=None):
    out = Guarded((vol.shape, torch.int16))
    kernels.dense_sgm_paths(behind_guard(vol, 0x5a), paths, p1, p2, c_invalid, out=out.out, direction=direction)
    return u16(out.check()[0])


@pytest.mark.parametrize('shape', PATH_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_paths_against_the_restatement(shape):
    """total is handed in poison-filled: the entry point leaves none of it"""
    vol = synthetic_volume(*shape)
    for paths in (4, 8):
        for p1, p2 in PENALTIES:
            want = ds.aggregate(vol, paths, p1, p2, 127)
            same('total, %d paths, P1 %d, P2 %d' % (paths, p1, p2), run_paths(vol, paths, p1, p2), want)
    same('c_invalid', run_paths(vol, 8, 8, 64, c_invalid=0), ds.aggregate(vol, 8, 8, 64, 0))
    same('c_invalid', run_paths(vol, 8, 8, 64, c_invalid=254), ds.aggregate(vol, 8, 8, 64, 254))


@pytest.mark.parametrize('value', [255, 0, 254])
def test_paths_of_a_constant_volume(value):
    for shape in ((29, 37, 64), (65, 3, 17)):
        vol = np.full(shape, value, np.uint8)
        for paths in (4, 8):
            for p1, p2 in PENALTIES:
                got = run_paths(vol, paths, p1, p2, c_invalid=200)
                same('total', got, ds.aggregate(vol, paths, p1, p2, 200))
                assert (got == paths * (200 if value == 255 else value)).all()


def test_the_bound_of_the_total_is_reached():
    """every path cost at its bound 254 + 255 next to one zero: the largest total the rules allow"""
    vol = np.full((9, 12, 64), 254, np.uint8)
    vol[:, :, 40] = 0
    vol[4, 5, 40] = 254
    want = ds.aggregate(vol, 8, 255, 255, 127)
    assert want.max() == 8 * 509 == 4072
    same('total', run_paths(vol, 8, 255, 255), want)


@pytest.mark.parametrize('direction', range(8))
def test_one_direction_is_its_path_cost(direction):
    vol = synthetic_volume(29, 37, 64)
    want = ds.path_cost(vol, ds.DIRECTIONS[direction], 8, 64, 127).astype(np.uint16)
    same('L_r', run_paths(vol, 8, 8, 64, direction=direction), want)


def test_paths_twice_give_the_same_total():
    vol = synthetic_volume(48, 64, 13, seed=1)
    d_vol = behind_guard(vol, 0x5a)
    total = torch.full(vol.shape, 0x5a5a, dtype=torch.int16, device='cuda')
    first = u16(kernels.dense_sgm_paths(d_vol, 8, 16, 128, out=(total,)).cpu().numpy()).copy()
    again = u16(kernels.dense_sgm_paths(d_vol, 8, 16, 128, out=(total,)).cpu().numpy())
    same('total', again, first)
    same('total', first, ds.aggregate(vol, 8, 16, 128))


# ---- select ----
def run_select(total, vol, max_cost, w_far=dc.W_FAR, w_near=dc.W_NEAR):
    h, w, _planes = vol.shape
    out = Guarded(((h, w), torch.int32), ((h, w), torch.uint8), ((h, w), torch.int16), ((h, w), torch.float32))
    kernels.dense_sgm_select(behind_guard(total.astype(np.int16), 0), behind_guard(vol, 0), w_far, w_near, max_cost, out=out.out)
    plane, cost, tot0, depth = out.check()
    return plane, cost, u16(tot0), depth


def assert_same_select(got, want):
    for name, g, e in zip(('plane', 'cost', 'total', 'depth'), got, want):
        same(name, g, e)


def test_select_rule_on_the_device():
    """ties to the smallest plane, the winner at either end, a raw 255 at the winner, max_cost"""
    T = np.array([[[7, 3, 3, 9, 9], [2, 5, 5, 5, 5], [9, 9, 9, 9, 1], [4, 4, 4, 4, 4], [9, 4, 4, 4, 9], [5, 5, 3, 5, 5],
                   [4072, 4072, 4071, 4072, 4072], [0, 0, 0, 0, 0], [9, 8, 7, 7, 8]]], np.uint16)
    vol = np.full(T.shape, 10, np.uint8)
    vol[0, 4, 1] = 255
    vol[0, 5, 2] = 52
    step = dr.plane_step(dc.W_FAR, dc.W_NEAR, 5)
    for max_cost in (51, 52, 9, 0, 254):
        want = ds.select(T, vol, dc.W_FAR, step, max_cost)
        assert want[0].tolist() == [[1, 0, 4, 0, 1, 2, 2, 0, 2]]
        assert np.isnan(want[3][0, 4])                          # (a raw 255 is never kept)
        assert_same_select(run_select(T, vol, max_cost), want)
    assert np.isnan(ds.select(T, vol, dc.W_FAR, step, 51)[3][0, 5]) and not np.isnan(ds.select(T, vol, dc.W_FAR, step, 52)[3][0, 5])


@pytest.mark.parametrize('shape', [(1, 1, 2), (3, 65, 5), (29, 37, 64), (48, 64, 13), (65, 3, 17)], ids=lambda s: '%dx%dx%d' % s)
def test_select_against_the_restatement(shape):
    vol = synthetic_volume(*shape)
    step = dr.plane_step(dc.W_FAR, dc.W_NEAR, shape[2])
    rng = np.random.default_rng(shape[1])
    totals = [ds.aggregate(vol, 8, 8, 64), ds.aggregate(vol, 4, 0, 0),
              rng.integers(0, 6, shape).astype(np.uint16),        # many ties
              rng.integers(0, 4073, shape).astype(np.uint16)]
    for T in totals:
        want = ds.select(T, vol, dc.W_FAR, step, 100)
        if shape[0] * shape[1] > 100:
            assert np.isnan(want[3]).any() and np.isfinite(want[3]).any()
        assert_same_select(run_select(T, vol, 100), want)


# ---- depth_maps ----
NEIGHBOURS = [[1, 2], [0, 2], [0, 1]]
RANGES = [(dc.Z_NEAR, dc.Z_FAR)] * 3


@functools.lru_cache(maxsize=None)
def restated(h, w):
    """the three-view scene through the restatements -> views, winner-take-all fields, semi-global fields"""
    views = dc.scene('roof', h, w)[0][:3]
    wta, sgm = [], []
    for i, v in enumerate(views):
        nbs = [views[j] for j in NEIGHBOURS[i]]
        S = ds.score_stack(v, nbs, dc.W_FAR, dc.W_NEAR, dc.PLANES, 3)
        wta.append(ds.winner_of_scores(S, dc.W_FAR, dc.W_NEAR))
        sgm.append(ds.sgm_of_scores(S, dc.W_FAR, dc.W_NEAR, p1=dense.SGM_P1, p2=dense.SGM_P2))
    return views, [np.stack(f) for f in zip(*wta)], [np.stack(f) for f in zip(*sgm)]


@pytest.mark.parametrize('w, h', [(37, 29), (64, 48)])
def test_depth_maps_sgm_against_the_restatement(w, h):
    views, (_wp, w_score, _wd), (plane, cost, total, depth) = restated(h, w)
    keep, ned = dr.check(depth, views, NEIGHBOURS)
    assert 0 < keep.sum() < np.isfinite(depth).sum()
    maps = dense.depth_maps(device_views(views), NEIGHBOURS, RANGES, planes=dc.PLANES, regularize='sgm')
    same('plane', maps.plane.cpu().numpy(), plane)
    same('score', maps.score.cpu().numpy(), w_score)
    same('depth', maps.depth.cpu().numpy(), depth)
    same('cost', maps.cost.cpu().numpy(), cost)
    same('total', u16(maps.total.cpu().numpy()), total)
    same('keep', maps.keep.cpu().numpy(), keep)
    same('ned', maps.ned.cpu().numpy(), ned)
    four = dense.depth_maps(device_views(views), NEIGHBOURS, RANGES, planes=dc.PLANES, regularize='sgm', paths=4,
                            p1=4, p2=32, c_invalid=60)
    S = [ds.sgm(v, [views[j] for j in NEIGHBOURS[i]], dc.W_FAR, dc.W_NEAR, dc.PLANES, p1=4, p2=32, paths=4, c_invalid=60)
         for i, v in enumerate(views)]
    same('depth, 4 paths', four.depth.cpu().numpy(), np.stack([s[3] for s in S]))
    same('total, 4 paths', u16(four.total.cpu().numpy()), np.stack([s[2] for s in S]))


@pytest.mark.parametrize('w, h', [(37, 29), (64, 48)])
def test_depth_maps_none_is_the_sweep(w, h):
    views, (plane, score, depth), _sgm = restated(h, w)
    keep, ned = dr.check(depth, views, NEIGHBOURS)
    maps = dense.depth_maps(device_views(views), NEIGHBOURS, RANGES, planes=dc.PLANES, regularize='none')
    same('plane', maps.plane.cpu().numpy(), plane)
    same('score', maps.score.cpu().numpy(), score)
    same('depth', maps.depth.cpu().numpy(), depth)
    same('keep', maps.keep.cpu().numpy(), keep)
    same('ned', maps.ned.cpu().numpy(), ned)
    assert not hasattr(maps, 'cost') and not hasattr(maps, 'total')
    first = dr.sweep(views[0], [views[j] for j in NEIGHBOURS[0]], dc.W_FAR, dc.W_NEAR, dc.PLANES)
    same('depth', depth[0], first[2])


def test_a_view_without_neighbours_stays_empty():
    views = dc.scene('roof', 29, 37)[0][:3]
    maps = dense.depth_maps(device_views(views), [[1], [0], []], [RANGES[0], None, RANGES[2]], planes=dc.PLANES,
                            regularize='sgm', check=False)
    want = ds.sgm(views[0], [views[1]], dc.W_FAR, dc.W_NEAR, dc.PLANES)
    same('depth', maps.depth[0].cpu().numpy(), want[3])
    for i in (1, 2):
        assert (maps.plane[i] == -1).all() and torch.isnan(maps.depth[i]).all() and (maps.cost[i] == 255).all()
        assert (maps.total[i] == 0).all() and not maps.keep[i].any()


# ---- the command line ----
def test_script_writes_the_mode(tmp_path):
    """5d-dense-surface.py --regularize sgm in a process of its own: its raster is the one this process
    makes from the same decoded frames in the same mode, and dense.json names the mode"""
    import json
    import os
    import pickle
    import subprocess
    import sys
    from conftest import REPO
    from imageanalysis_amd import image, panda3d
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
           '--gsd', '2.0', '--regularize', 'sgm', '--p1', '8', '--paths', '4']
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    out = pdir / 'ImageAnalysis' / 'dense'
    info = json.loads((out / 'dense.json').read_text())
    assert list(info)[-4:] == ['regularize', 'p1', 'p2', 'paths']
    assert (info['regularize'], info['p1'], info['p2'], info['paths']) == ('sgm', 8, dense.SGM_P2, 4)
    views, group = dense.views_from_project(proj, [dc.NAMES], 0, matches, 1.0 / dc.FULL,
                                            frames=[torch.from_numpy(f).cuda() for f in decoded])
    poses = [(v.R, v.C) for v in views]
    neighbours = dense.choose_neighbours(matches, group, poses, n=3)
    ranges = dense.depth_range(matches, group, poses)
    maps = dense.depth_maps(views, neighbours, ranges, planes=dc.PLANES, regularize='sgm', p1=8, paths=4)
    plain = dense.depth_maps(views, neighbours, ranges, planes=dc.PLANES)
    assert not torch.equal(maps.plane, plain.plane)
    want = dense.fuse(views, maps, 2.0).dsm.cpu().numpy()
    same('dsm', np.load(str(out / 'dsm.npy')), want)
    bad = subprocess.run(cmd[:-6] + ['--regularize', 'sgm', '--planes', '65'], capture_output=True, text=True, env=env,
                         cwd=str(tmp_path))
    assert bad.returncode == 2 and 'semi-global' in bad.stderr
