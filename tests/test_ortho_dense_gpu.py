"""GPU: csrc/ortho_dsm.hip (iamx_ortho_dsm_image, iamx_dense_fill) and ortho.compose_dense /
render_dense / dense.fill against tests/ortho_dense_restatement.py, bit for bit.  Outputs start
poison-filled with guard bytes behind them, NaN sits behind every DSM."""
import ctypes

import numpy as np
import pytest
import torch

import dense_common as dc
import ortho_common as oc
import ortho_dense_restatement as rs
from imageanalysis_amd import dense, kernels, ortho
from imageanalysis_amd._lib import lib, stream_ptr
from test_ortho_gpu import LIB_STANDIN, _dev, project  # noqa: F401  (the stand-in project fixture and the lib package)

pytestmark = pytest.mark.gpu

GUARD = 256                    # bytes
POISON = 0x5a
EINVAL = -1
WIDTH, HEIGHT, FOCAL = oc.FRAME_W, oc.FRAME_H, 60.0
K_CAMERA = np.array([FOCAL, FOCAL, (WIDTH - 1) / 2.0, (HEIGHT - 1) / 2.0])
MODES = ('best', 'feather')
_p = kernels._ptr


def behind_nan(a):
    """numpy float32 array -> its device copy with NaNs behind it"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.full((a.size + 64,), float('nan'), dtype=torch.float32, device='cuda')
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return buf[:a.size].view(a.shape)


class Guarded(object):
    """poison-filled output tensors, each with GUARD poison bytes behind it"""

    def __init__(self, *specs):
        self.bufs, self.out = [], []
        for spec in specs:
            if spec is None:
                self.bufs.append(None)
                self.out.append(None)
                continue
            shape, dtype = spec
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            buf = torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device='cuda')
            self.bufs.append(buf)
            self.out.append(buf[:nbytes].view(dtype).view(shape))

    def check(self):
        for buf in self.bufs:
            if buf is not None:
                assert bool((buf[-GUARD:] == POISON).all()), "a guard byte was written"
        return [None if t is None else t.view(torch.uint8).cpu().numpy().view(_NP[t.dtype]).reshape(tuple(t.shape))
                for t in self.out]

    def untouched(self):
        return all(buf is None or bool((buf == POISON).all()) for buf in self.bufs)


_NP = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32, torch.uint16: np.uint16,
       torch.uint8: np.uint8}


def accumulators(mode, Ho, Wo):
    n = (Ho, Wo)
    return Guarded((n if mode == 'best' else n + (4,), torch.float64), (n, torch.int32) if mode == 'best' else None,
                   (n, torch.uint16), (n + (3,), torch.uint8))


def look_at(C, target):
    """R (NED -> camera) of a camera at C whose axis passes through target, image x to the right"""
    z = np.asarray(target, float) - np.asarray(C, float)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x = np.array([0.0, 1.0, 0.0]) if np.linalg.norm(x) < 1e-9 else x / np.linalg.norm(x)
    return np.array([x, np.cross(z, x), z])


def camera(C, angles=(0.0, 0.0, 0.0), R=None, dist=dc.DIST):
    """-> the public tuple (K at camera size, width, height, dist, R, C)"""
    return (K_CAMERA, WIDTH, HEIGHT, np.array(dist, float), dc._rot(*angles).dot(dc.NADIR) if R is None else R,
            np.array(C, float))


def restated(cam, frame):
    K, width, height, dist, R, C = cam
    return rs.scaled_K(K, width, height, frame.shape[1], frame.shape[0]), dist, R, C


def bumpy(H, W, seed, holes=0):
    """a rough ground with a 9 m block on it -> (dsm float32, x0, y1, gsd)"""
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, 0.3, (H, W))
    z[H // 3:H // 3 + max(H // 4, 1), W // 2:W // 2 + max(W // 4, 1)] += 9.0
    z = z.astype(np.float32)
    for _ in range(holes):
        r, c = rng.integers(0, H), rng.integers(0, W)
        z[r:r + rng.integers(1, 3), c:c + rng.integers(1, 4)] = np.nan
    return z, -W * 1.0, H * 1.0, 2.0


FOUR = [camera((0.0, 0.0, -60.0), (0.03, -0.02, 0.01)), camera((10.0, -15.0, -58.0), (-0.2, 0.04, 0.03)),
        camera((-12.0, 8.0, -63.0), (0.5, -0.03, -0.04)), camera((5.0, 30.0, -61.0), (1.4, 0.02, 0.02))]


def five_images():
    """four cameras with 64 x 96 frames and the first camera again with a 32 x 48 frame (prefiltered)"""
    return FOUR + [FOUR[0]], [oc.hash_frame(k) for k in range(4)] + [oc.hash_frame(4, 32, 48)]


def run_device(mode, dsm, x0, y1, gsd, cams, frames, ss, bias, boxes=None):
    """clear, one iamx_ortho_dsm_image per image (the whole mosaic unless boxes= says otherwise),
    resolve -> dict like the restatement's"""
    L = lib()
    H, W = dsm.shape
    Ho, Wo = H * ss, W * ss
    d = behind_nan(dsm)
    out = accumulators(mode, Ho, Wo)
    acc, index, count, bgr = out.out
    m = ortho.MODES[mode]
    assert L.iamx_ortho_clear(m, Ho, Wo, _p(acc), _p(index), _p(count), _p(bgr), stream_ptr()) == 0
    zmax = rs.zmax_of(dsm)
    for k, (cam, frame) in enumerate(zip(cams, frames)):
        f = torch.from_numpy(np.array(frame)).cuda()
        K, dist, R, C = restated(cam, frame)
        params = kernels.ortho_dsm_params(x0, y1, gsd, bias, zmax, K, dist, R, C)
        kernels.ortho_dsm_image(m, d, ss, params, f, k, (0, 0, Wo - 1, Ho - 1) if boxes is None else boxes[k],
                                acc, index, count, bgr)
    torch.cuda.synchronize()
    before = out.check()[0].copy()
    if mode == 'feather':
        assert L.iamx_ortho_resolve(Ho, Wo, _p(acc), _p(count), _p(bgr), stream_ptr()) == 0
        torch.cuda.synchronize()
    acc, index, count, bgr = out.check()
    assert before.tobytes() == acc.tobytes()
    return dict(acc=acc, index=index, count=count, bgr=bgr)


def assert_same(got, want, what=''):
    for key in ('acc', 'index', 'count', 'bgr'):
        g, e = got[key], want[key]
        if e is None:
            assert g is None
            continue
        assert g.dtype == e.dtype and g.shape == e.shape, (what, key)
        bad = np.nonzero(dc.bits(g) != dc.bits(e))
        assert len(bad[0]) == 0, "%s %s differs at %d places, first %s: %r != %r" % (
            what, key, len(bad[0]), tuple(int(b[0]) for b in bad), g[tuple(b[0] for b in bad)], e[tuple(b[0] for b in bad)])


def both(dsm, x0, y1, gsd, cams, frames, ss, bias, mode, boxes=None):
    want = rs.compose(dsm, x0, y1, gsd, [restated(c, f) for c, f in zip(cams, frames)], frames, mode, ss=ss, bias=bias,
                      boxes=boxes)
    got = run_device(mode, dsm, x0, y1, gsd, cams, frames, ss, bias, boxes)
    assert_same(got, want, '%s ss %d' % (mode, ss))
    return want


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ss', [1, 3])
@pytest.mark.parametrize('size', [(24, 20), (33, 17)])
def test_five_images_equal_the_restatement(size, ss, mode):
    dsm, x0, y1, gsd = bumpy(size[0], size[1], 3)
    cams, frames = five_images()
    want = both(dsm, x0, y1, gsd, cams, frames, ss, 0.6, mode)
    assert want['count'].max() == 5 and (want['count'] > 0).mean() > 0.9
    seen = [int(v.sum()) for v in want['visible']]
    assert min(seen) > 0
    assert any(v.sum() < (want['count'] > 0).sum() for v in want['visible'])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ss', [1, 3])
def test_holes_in_the_dsm(ss, mode):
    """ss = 1: a pixel centre is a cell centre, tx = ty = 0, and a hole beside the cell must not reach it"""
    dsm, x0, y1, gsd = bumpy(24, 20, 8, holes=12)
    assert np.isnan(dsm).sum() > 12
    cams, frames = five_images()
    want = both(dsm, x0, y1, gsd, cams[:2], frames[:2], ss, 0.6, mode)
    if ss == 1:
        beside = ~np.isnan(dsm) & np.isnan(np.roll(dsm, -1, 1))
        beside[:, -1] = False
        assert beside.any() and not np.isnan(rs.heights(dsm, 1)[beside]).any() and (want['count'][beside] > 0).any()
        assert (want['count'][np.isnan(dsm)] == 0).all()


@pytest.mark.parametrize('mode', MODES)
def test_cameras_at_the_edges_of_the_rules(mode):
    dsm, x0, y1, gsd = bumpy(24, 20, 5)
    frames = [oc.hash_frame(k) for k in range(3)]
    H, W = dsm.shape
    top = float(dsm[H // 3, W // 2])
    block_n, block_e = y1 - (H // 3 + 0.5) * gsd, x0 + (W // 2 + 0.5) * gsd
    low = camera((block_n + 9.0, block_e - 14.0, -(top - 3.0)), R=look_at((block_n + 9.0, block_e - 14.0, -(top - 3.0)),
                                                                             (block_n - 2.0, block_e + 6.0, 0.0)))
    outside = (3.0, 90.0, -30.0)
    far = camera(outside, R=look_at(outside, (0.0, 0.0, 0.0)))
    level = (2.0, -4.0, -20.0)
    behind = camera(level, R=look_at(level, (2.0, 30.0, 0.0)))      # looks east, 30 degrees down: e < -16 is behind it
    want = both(dsm, x0, y1, gsd, [low, far, behind], frames, 2, 0.5, mode)
    seen = want['visible']
    assert 0 < seen[0].sum() and 0 < seen[1].sum() < seen[1].size and 0 < seen[2].sum() < seen[2].size
    n = (y1 - (np.arange(2 * H) + 0.5) * gsd / 2)[:, None]
    e = (x0 + (np.arange(2 * W) + 0.5) * gsd / 2)[None, :]
    h2 = rs.heights(dsm, 2)
    assert (h2 >= top - 3.0).any() and not seen[0][h2 >= top - 3.0].any()      # the camera is below these cells
    assert not seen[2][:, (e < level[1]).ravel()].any()                        # behind the camera


def test_twins_the_earlier_wins_and_both_count():
    dsm, x0, y1, gsd = bumpy(24, 20, 6)
    want = both(dsm, x0, y1, gsd, [FOUR[1], FOUR[1]], [oc.hash_frame(0), oc.hash_frame(1)], 2, 0.6, 'best')
    on = want['count'] > 0
    assert on.any() and (want['count'][on] == 2).all() and (want['index'][on] == 0).all()
    both(dsm, x0, y1, gsd, [FOUR[1], FOUR[1]], [oc.hash_frame(0), oc.hash_frame(1)], 2, 0.6, 'feather')


@pytest.mark.parametrize('mode', MODES)
def test_one_cell_and_small_boxes(mode):
    one = np.array([[2.5]], np.float32)
    cams, frames = [FOUR[0]], [oc.hash_frame(0)]
    for ss in (1, 8):
        want = both(one, -1.0, 1.0, 2.0, cams, frames, ss, 0.0, mode)
        assert (want['count'] == 1).all()
    dsm, x0, y1, gsd = bumpy(24, 20, 3)
    empty = both(dsm, x0, y1, gsd, cams, frames, 3, 0.6, mode, boxes=[(5, 7, 4, 7)])
    assert not empty['count'].any()
    both(dsm, x0, y1, gsd, cams, frames, 3, 0.6, mode, boxes=[(5, 7, 5, 6)])
    pixel = both(dsm, x0, y1, gsd, cams, frames, 3, 0.6, mode, boxes=[(17, 40, 17, 40)])
    assert pixel['count'].sum() == 1 and pixel['count'][40, 17] == 1
    corner = both(dsm, x0, y1, gsd, cams, frames, 3, 0.6, mode, boxes=[(59, 71, 59, 71)])
    assert corner['count'].sum() == 1


def roof_dsm(cells, gsd):
    x0, y1 = -0.5 * cells * gsd, 0.5 * cells * gsd
    e = x0 + (np.arange(cells) + 0.5) * gsd
    n = y1 - (np.arange(cells) + 0.5) * gsd
    on = (np.abs(n)[:, None] < dc.ROOF[0]) & (np.abs(e)[None, :] < dc.ROOF[1])
    return np.where(on, dc.ROOF[2], 0.0).astype(np.float32), x0, y1, gsd


@pytest.mark.parametrize('mode', MODES)
def test_long_marches_and_a_shadow_on_the_roof_scene(mode):
    dsm, x0, y1, gsd = roof_dsm(48, 2.0)
    C = (0.0, 120.0, -60.0)
    cam = camera(C, R=look_at(C, (0.0, 0.0, 0.0)))
    want = both(dsm, x0, y1, gsd, [cam], [oc.hash_frame(2)], 1, 1.0, mode)
    n = (y1 - (np.arange(48) + 0.5) * gsd)[:, None]
    e = (x0 + (np.arange(48) + 0.5) * gsd)[None, :]
    shadow = (np.abs(n) < 10) & (e < -24) & (e > -26)          # the ground just west of the roof
    lit = (np.abs(n) < 10) & (e > 24) & (e < 40)
    assert shadow.sum() == 10 and not want['visible'][0][shadow].any() and want['visible'][0][lit].all()


# ---- iamx_dense_fill ----
def seeded_holes(H, W, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(100.0, 5.0, (H, W)).astype(np.float32)
    z[rng.random((H, W)) < 0.3] = np.nan
    z[3:12, 5:16] = np.nan
    z[0, 0] = z[H - 1, W - 1] = np.nan
    return z


@pytest.mark.parametrize('rounds', [0, 1, 3])
@pytest.mark.parametrize('which', ['1x1', '3x3', '17x33'])
def test_fill_kernel_equals_the_restatement(which, rounds):
    z = {'1x1': np.array([[7.25]], np.float32),
         '3x3': np.array([[1.1, 2.2, 3.3], [4.4, np.nan, 6.6], [7.7, 8.8, 9.9]], np.float32),
         '17x33': seeded_holes(17, 33, 9)}[which]
    H, W = z.shape
    want_z, want_round = rs.fill(z, rounds)
    L = lib()
    src = behind_nan(z)
    bufs = [Guarded(((H, W), torch.float32), ((H, W), torch.uint8)) for _ in range(2)]
    assert L.iamx_dense_fill(_p(src), None, W, H, 0, _p(bufs[0].out[0]), _p(bufs[0].out[1]), stream_ptr()) == 0
    for k in range(1, rounds + 1):
        a, b = bufs[(k - 1) & 1], bufs[k & 1]
        assert L.iamx_dense_fill(_p(a.out[0]), _p(a.out[1]), W, H, k, _p(b.out[0]), _p(b.out[1]), stream_ptr()) == 0
    torch.cuda.synchronize()
    got_z, got_round = bufs[rounds & 1].check()
    bufs[(rounds + 1) & 1].check()
    assert dc.bits(got_z).tobytes() == dc.bits(want_z).tobytes() and got_round.tobytes() == want_round.tobytes()
    if which == '17x33' and rounds == 3:
        assert (want_round == 255).any() and set(np.unique(want_round)) == {0, 1, 2, 3, 255}
    via_z, via_round = kernels.dense_fill(z, rounds)
    assert dc.bits(via_z.cpu().numpy()).tobytes() == dc.bits(want_z).tobytes()
    assert via_round.cpu().numpy().tobytes() == want_round.tobytes()


def test_dense_fill_keeps_the_count_and_the_frame():
    z = seeded_holes(17, 33, 2)
    count = torch.arange(17 * 33, dtype=torch.int32, device='cuda').view(17, 33)
    s = dense.Surface(torch.from_numpy(z).cuda(), count, -3.0, 9.0, 0.5)
    filled, round_of = dense.fill(s, rounds=2)
    want_z, want_round = rs.fill(z, 2)
    assert filled.count is count and (filled.x0, filled.y1, filled.gsd) == (-3.0, 9.0, 0.5)
    assert dc.bits(filled.dsm.cpu().numpy()).tobytes() == dc.bits(want_z).tobytes()
    assert round_of.dtype == torch.uint8 and round_of.cpu().numpy().tobytes() == want_round.tobytes()
    assert dc.bits(s.dsm.cpu().numpy()).tobytes() == dc.bits(z).tobytes()      # the input is left alone


# ---- the public functions ----
@pytest.mark.parametrize('mode', MODES)
def test_compose_dense_on_the_roof_scene(mode):
    dsm, x0, y1, gsd = roof_dsm(48, 2.0)
    surface = dense.Surface(torch.from_numpy(dsm).cuda(), torch.zeros((48, 48), dtype=torch.int32, device='cuda'), x0, y1, gsd)
    K = np.array([dc.FOCAL, dc.FOCAL, (WIDTH - 1) / 2.0, (HEIGHT - 1) / 2.0])
    cams = [(K, WIDTH, HEIGHT, np.array(dc.DIST), dc.NADIR, np.array([c[0], c[1], -dc.ALTITUDE])) for c in dc.CENTRES[1:]]
    frames = [oc.hash_frame(k) for k in range(3)]
    m = ortho.compose_dense(surface, cams, [torch.from_numpy(np.array(f)).cuda() for f in frames], mode=mode, upsample=2,
                            bias=1.0, names=['a', 'b', 'c'])
    want = rs.compose(dsm, x0, y1, gsd, [restated(c, f) for c, f in zip(cams, frames)], frames, mode, ss=2, bias=1.0)
    torch.cuda.synchronize()
    got = dict(acc=want['acc'], index=None if m.index is None else m.index.cpu().numpy(),
               count=m.count.view(torch.uint8).cpu().numpy().view(np.uint16).reshape(96, 96), bgr=m.bgr.cpu().numpy())
    assert_same(got, want, 'compose_dense ' + mode)
    assert (m.surface, m.upsample, m.bias, m.gsd, m.mode, m.names, m.shape) == ('dense', 2, 1.0, 1.0, mode, ['a', 'b', 'c'], (96, 96))
    assert (want['count'] < 3).any() and (want['count'] == 3).any()
    # the default bias is one DSM cell
    d = ortho.compose_dense(surface, cams[:1], frames[:1], mode=mode)
    assert d.bias == gsd and d.upsample == 1 and d.shape == (48, 48)
    w1 = rs.compose(dsm, x0, y1, gsd, [restated(cams[0], frames[0])], frames[:1], mode, ss=1, bias=gsd)
    assert d.bgr.cpu().numpy().tobytes() == w1['bgr'].tobytes()


def test_the_host_box_of_a_pitched_camera_on_the_device():
    """compose_dense's own box (the device's undistortion of the border) against the whole mosaic"""
    dsm, x0, y1, gsd = roof_dsm(48, 2.0)
    surface = dense.Surface(dsm, np.zeros((48, 48), np.int32), x0, y1, gsd)
    cam = camera((-10.0, 6.0, -40.0), (0.3, 0.5, 0.0))
    frame = oc.hash_frame(1)
    K, dist, R, C = restated(cam, frame)
    box = ortho.work_box(K, dist, R, C, WIDTH, HEIGHT, 0.0, 12.0, x0, y1, 1.0, 96, 96)
    assert 0 < (box[2] - box[0] + 1) * (box[3] - box[1] + 1) < 96 * 96
    m = ortho.compose_dense(surface, [cam], [frame], mode='best', upsample=2, bias=1.0)
    want = rs.compose(dsm, x0, y1, gsd, [(K, dist, R, C)], [frame], 'best', ss=2, bias=1.0)
    assert m.bgr.cpu().numpy().tobytes() == want['bgr'].tobytes() and np.array_equal(m.index.cpu().numpy(), want['index'])


def test_render_dense_on_a_stand_in_project():
    """poses, optimised K and distortion of a project; frames=; the prefilter shrinks what the call says"""
    import contextlib
    import io
    proj = dc.standin_project()
    frames = dc.project_frames(proj)
    n, e = np.meshgrid(60.0 - (np.arange(60) + 0.5) * 2.0, -60.0 + (np.arange(60) + 0.5) * 2.0, indexing='ij')
    dsm = (-(0.15 * n + 0.1 * e)).astype(np.float32)            # the slope scene: down = 0.15 north + 0.1 east
    dsm[20:24, 30:36] += 8.0
    surface = dense.Surface(dsm, np.zeros(dsm.shape, np.int32), -60.0, 60.0, 2.0)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    with contextlib.redirect_stdout(io.StringIO()):
        m = ortho.render_dense(proj, [dc.NAMES], 0, surface, mode='best', upsample=1, bias=1.0, prefilter=False, frames=dev)
    from imageanalysis_amd.hostlib import camera as cam_mod
    K = np.asarray(cam_mod.get_K(optimized=True), np.float64)
    width, height = cam_mod.get_image_params()
    cams = [(K, width, height, np.array(dc.DIST), ) + dense.image_pose(im) for im in proj.image_list]
    want = rs.compose(dsm, -60.0, 60.0, 2.0, [restated(c, f) for c, f in zip(cams, frames)], frames, 'best', ss=1, bias=1.0)
    assert m.bgr.cpu().numpy().tobytes() == want['bgr'].tobytes() and np.array_equal(m.index.cpu().numpy(), want['index'])
    assert m.names == dc.NAMES and ortho.render_dense_stats['images'] == 4 and ortho.render_dense_stats['prefiltered'] == 0
    assert (want['index'] >= 0).mean() > 0.5
    # native = 100 / (43 * 8) = 0.29 m against 2 m pixels: f = 0.145, the frames are shrunk to 74 x 56
    with contextlib.redirect_stdout(io.StringIO()):
        s = ortho.render_dense(proj, [dc.NAMES], 0, surface, mode='best', upsample=1, bias=1.0, frames=dev)
    assert ortho.render_dense_stats['prefiltered'] == 4
    small = []
    for c, f in zip(cams, dev):
        factor = ortho.dense_prefilter_factor(K, c[5], ortho.surface_heights(torch.from_numpy(dsm).cuda())[2], 2.0)
        small.append(kernels.resize_area(f, factor, factor).cpu().numpy())
    assert small[0].shape[0] < 100
    want = rs.compose(dsm, -60.0, 60.0, 2.0, [restated(c, f) for c, f in zip(cams, small)], small, 'best', ss=1, bias=1.0)
    assert s.bgr.cpu().numpy().tobytes() == want['bgr'].tobytes() and np.array_equal(s.index.cpu().numpy(), want['index'])


# ---- the command line: scripts/5e-true-ortho.py on test_ortho_gpu's stand-in for the reference's lib package ----
def test_script_fills_renders_and_writes_true_ortho(project, tmp_path):
    """5e-true-ortho.py in a process of its own (frames decoded from files by histogram.frame_pass); its
    tiles are the mosaic render_dense() makes in this process from the same decoded frames and DSM"""
    import contextlib
    import io
    import json
    import os
    import subprocess
    import sys
    from PIL import Image
    import step5_common as s5
    from imageanalysis_amd import image, panda3d
    proj, g = project
    names = list(g['groups'][0])
    standin = tmp_path / 'standin' / 'lib'
    standin.mkdir(parents=True)
    for name, text in LIB_STANDIN.items():
        (standin / name).write_text(text)
    pdir = tmp_path / 'project'
    (pdir / 'images').mkdir(parents=True)
    analysis = pdir / 'ImageAnalysis'
    analysis.mkdir()
    decoded = []
    for k, n in enumerate(names):
        path = str(pdir / 'images' / (n + '.JPG'))
        with open(path, 'wb') as fp:
            fp.write(panda3d.encode_jpeg(np.array(oc.hash_frame(k))))
        decoded.append(image._decode_bgr(path))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / 'standin'), s5.REPO, os.path.join(s5.REPO, 'tests')]))
    script = os.path.join(s5.REPO, 'imageanalysis_amd', 'scripts', '5e-true-ortho.py')
    cmd = ['timeout', '-k', '10', '120', sys.executable, script, str(pdir), '--mode', 'best', '--upsample', '2', '--bias', '1.5',
           '--fill-rounds', '3', '--tile', '128', '--format', 'png']
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode != 0 and '5d-dense-surface.py' in p.stderr and not (analysis / 'true_ortho').exists()
    # a DSM of 4 m cells over the sparse mosaic's frame: the grids' mean height, a block, a hole of 5 x 5 cells
    grids = oc.scene_input('step5_mid_default')[1]
    rf = ortho.raster_frame(grids, 4.0)
    dsm = np.full((rf.H, rf.W), np.float32(np.nanmean(grids[:, :, 2])), np.float32)
    dsm[10:16, 20:30] += np.float32(15.0)
    dsm[30:35, 40:45] = np.nan
    surface = dense.Surface(torch.from_numpy(dsm).cuda(), torch.ones(dsm.shape, dtype=torch.int32, device='cuda'),
                            rf.x0, rf.y1, 4.0)
    dense.save(surface, str(analysis))
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert '25 filled in 3 rounds, 0 still empty' in p.stdout and 'Wrote' in p.stdout and 'true_ortho' in p.stdout
    out = analysis / 'true_ortho'
    info = json.loads((out / 'ortho.json').read_text())
    assert (info['mode'], info['gsd'], info['surface'], info['upsample'], info['bias'], info['images']) == (
        'best', 2.0, 'dense', 2, 1.5, names)
    assert (info['width'], info['height']) == (2 * rf.W, 2 * rf.H) and not (analysis / 'ortho').exists()
    filled, _round_of = dense.fill(dense.load(str(analysis)), rounds=3)
    with contextlib.redirect_stdout(io.StringIO()):
        want = ortho.render_dense(proj, g['groups'], 0, filled, mode='best', upsample=2, bias=1.5, frames=_dev(decoded))
    want = want.bgr.cpu().numpy()
    assert (want.sum(axis=2) > 0).mean() > 0.5
    for t in info['tiles']:
        with Image.open(str(out / t['file'])) as im:
            px = np.asarray(im.convert('RGB'))[:, :, ::-1]
        r0, c0 = t['row'] * 128, t['col'] * 128
        assert px.tobytes() == np.ascontiguousarray(want[r0:r0 + t['height'], c0:c0 + t['width']]).tobytes(), t['file']


# ---- argument checks ----
def test_bad_arguments_return_the_error_code_and_write_nothing():
    L = lib()
    dsm, x0, y1, gsd = bumpy(24, 20, 3)
    d = behind_nan(dsm)
    frame = torch.from_numpy(np.array(oc.hash_frame(0))).cuda()
    K, dist, R, C = restated(FOUR[0], oc.hash_frame(0))
    params = kernels.ortho_dsm_params(x0, y1, gsd, 0.5, rs.zmax_of(dsm), K, dist, R, C)
    pp = params.ctypes.data_as(ctypes.c_void_p)
    for mode in (0, 1):
        out = accumulators(ortho.DENSE_MODES[mode], 24, 20)
        acc, index, count, bgr = out.out

        def call(mode=mode, dsm=d, H=24, W=20, ss=1, params=pp, frame=frame, h_s=64, w_s=96, box=(0, 0, 19, 23),
                 acc=acc, index=index, count=count, bgr=bgr):
            return L.iamx_ortho_dsm_image(mode, _p(dsm), H, W, ss, params, _p(frame), h_s, w_s, 0, box[0], box[1], box[2],
                                          box[3], _p(acc), _p(index), _p(count), _p(bgr), stream_ptr())

        bad = [dict(dsm=None), dict(params=None), dict(frame=None), dict(acc=None), dict(count=None), dict(bgr=None),
               dict(ss=0), dict(ss=9), dict(H=0), dict(W=0), dict(h_s=1), dict(w_s=1), dict(mode=2),
               dict(box=(0, 0, 20, 23)), dict(box=(0, 0, 19, 24)), dict(box=(-1, 0, 19, 23)), dict(box=(0, -1, 19, 23))]
        if mode == 0:
            bad.append(dict(index=None))
        for kw in bad:
            assert call(**kw) == EINVAL, kw
        assert call(box=(3, 3, 2, 3)) == 0 and call(box=(3, 3, 3, 2)) == 0          # an empty box succeeds
        torch.cuda.synchronize()
        assert out.untouched()
    nan = params.copy()
    nan[3] = np.nan
    out = accumulators('best', 24, 20)
    acc, index, count, bgr = out.out
    assert L.iamx_ortho_dsm_image(0, _p(d), 24, 20, 1, nan.ctypes.data_as(ctypes.c_void_p), _p(frame), 64, 96, 0, 0, 0, 19, 23,
                                  _p(acc), _p(index), _p(count), _p(bgr), stream_ptr()) == EINVAL
    z = Guarded(((24, 20), torch.float32), ((24, 20), torch.uint8))
    for kw in (dict(src=None), dict(dst=None), dict(rdst=None), dict(W=0), dict(H=0), dict(k=255), dict(k=-1), dict(k=1)):
        a = dict(src=d, rsrc=None, W=20, H=24, k=0, dst=z.out[0], rdst=z.out[1])
        a.update(kw)
        assert L.iamx_dense_fill(_p(a['src']), _p(a['rsrc']), a['W'], a['H'], a['k'], _p(a['dst']), _p(a['rdst']),
                                 stream_ptr()) == EINVAL, kw
    torch.cuda.synchronize()
    assert out.untouched() and z.untouched()
    with pytest.raises(MemoryError, match='GB of accumulators'):
        big = dense.Surface(torch.zeros((1 << 17, 1 << 17), dtype=torch.float32, device='meta'), None, 0.0, 0.0, 1.0)
        ortho.compose_dense(big, [FOUR[0]], [oc.hash_frame(0)], upsample=8)
