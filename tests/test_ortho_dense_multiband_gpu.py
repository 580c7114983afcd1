"""GPU: the true orthophoto's blend -- csrc/ortho_dsm.hip's owner and layer passes
(iamx_ortho_dsm_owner, iamx_ortho_dsm_layer) and ortho.compose_dense / render_dense(bands=) and
5e-true-ortho.py --bands against tests/ortho_dense_multiband_restatement.py, bit for bit.  Through the C
ABI the outputs start poison-filled with guard bytes behind them, NaN sits behind every DSM."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import dense_common as dc
import ortho_common as oc
import ortho_dense_multiband_restatement as ms
import ortho_dense_restatement as rs
from imageanalysis_amd import dense, kernels, ortho
from imageanalysis_amd._lib import lib, stream_ptr
from test_ortho_dense_gpu import (EINVAL, FOUR, Guarded, LIB_STANDIN, POISON, _dev, _p, behind_nan, bumpy, camera,  # noqa: F401
                                  five_images, look_at, project, restated)

pytestmark = pytest.mark.gpu

FAR = (3.0, 90.0, -30.0)       # covers the east of the bumpy scenes, obliquely: it never wins a pixel there
AWAY = (0.0, 500.0, -60.0)     # looks down half a kilometre east of them: its work box is empty


def u16(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint16).reshape(tuple(t.shape))


def surface_of(dsm, x0, y1, gsd):
    return dense.Surface(behind_nan(dsm), torch.zeros(dsm.shape, dtype=torch.int32, device='cuda'), x0, y1, gsd)


def run_public(dsm, x0, y1, gsd, cams, frames, ss, bias, bands):
    """compose_dense(bands=) step by step, so that accumulators() can be read before finish()
    -> (dict like the restatement's, the composer)"""
    comp = ortho._DenseComposer(surface_of(dsm, x0, y1, gsd), 'best', ss, bias, None, bands, cams,
                                [f.shape[:2] for f in frames])
    for k, (cam, frame) in enumerate(zip(cams, frames)):
        comp.add(k, cam, torch.from_numpy(np.array(frame)).cuda())
    levels = [(N.cpu().numpy(), D.cpu().numpy()[:, :, None]) for N, D in comp.accumulators()]
    m = comp.finish()
    torch.cuda.synchronize()
    assert (m.mode, m.surface, m.upsample, m.bias) == ('multiband', 'dense', ss, bias)
    return dict(bgr=m.bgr.cpu().numpy(), index=m.index.cpu().numpy(), count=u16(m.count), bands=m.bands,
                N=[l[0] for l in levels], D=[l[1] for l in levels]), comp


def assert_blend_same(got, want, what=''):
    assert got['bands'] == want['bands'] == len(got['N']), what
    for key in ('index', 'count', 'bgr'):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert got[key].tobytes() == want[key].tobytes(), "%s %s differs at %d places" % (
            what, key, int((got[key] != want[key]).sum()))
    for l in range(want['bands']):
        for key in ('N', 'D'):
            g, e = got[key][l], want[key][l]
            assert g.dtype == e.dtype and g.shape == e.shape, (what, key, l)
            bad = dc.bits(g) != dc.bits(e)
            assert not bad.any(), "%s %s of level %d differs at %d places, first %r" % (
                what, key, l, int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad)))


def both(dsm, x0, y1, gsd, cams, frames, ss, bias, bands):
    want = ms.compose(dsm, x0, y1, gsd, [restated(c, f) for c, f in zip(cams, frames)], frames, bands=bands, ss=ss, bias=bias)
    got, comp = run_public(dsm, x0, y1, gsd, cams, frames, ss, bias, bands)
    assert_blend_same(got, want, 'ss %d bands %d' % (ss, bands))
    return want, comp


# ---- 1. equality with the restatement ----
@pytest.mark.parametrize('bands', [1, 5])
@pytest.mark.parametrize('ss', [1, 3])
@pytest.mark.parametrize('size', [(24, 20), (33, 17)])
def test_five_images_equal_the_restatement(size, ss, bands):
    dsm, x0, y1, gsd = bumpy(size[0], size[1], 3)
    cams, frames = five_images()
    want, _comp = both(dsm, x0, y1, gsd, cams, frames, ss, 0.6, bands)
    assert want['bands'] == bands and want['count'].max() == 5 and (want['count'] > 0).mean() > 0.9
    assert len(set(np.unique(want['index'])) - {-1}) >= 3


def test_compose_dense_is_the_same_call():
    dsm, x0, y1, gsd = bumpy(24, 20, 3)
    cams, frames = five_images()
    m = ortho.compose_dense(surface_of(dsm, x0, y1, gsd), cams, frames, upsample=2, bias=0.6, names=list('abcde'), bands=5)
    want = ms.compose(dsm, x0, y1, gsd, [restated(c, f) for c, f in zip(cams, frames)], frames, bands=5, ss=2, bias=0.6)
    assert m.bgr.cpu().numpy().tobytes() == want['bgr'].tobytes() and m.index.cpu().numpy().tobytes() == want['index'].tobytes()
    assert u16(m.count).tobytes() == want['count'].tobytes()
    assert (m.mode, m.bands, m.surface, m.upsample, m.bias, m.gsd, m.names) == ('multiband', 5, 'dense', 2, 0.6, 1.0, list('abcde'))
    # bands=0 is mode best, byte for byte
    zero = ortho.compose_dense(surface_of(dsm, x0, y1, gsd), cams, frames, upsample=2, bias=0.6, bands=0)
    best = rs.compose(dsm, x0, y1, gsd, [restated(c, f) for c, f in zip(cams, frames)], frames, 'best', ss=2, bias=0.6)
    assert (zero.mode, zero.bands) == ('best', None) and zero.bgr.cpu().numpy().tobytes() == best['bgr'].tobytes()


# ---- 2. the owner pass alone ----
def image_params(dsm, x0, y1, gsd, bias, cam, frame):
    K, dist, R, C = restated(cam, frame)
    return kernels.ortho_dsm_params(x0, y1, gsd, bias, rs.zmax_of(dsm), K, dist, R, C)


def cleared(Ho, Wo):
    out = Guarded(((Ho, Wo), torch.float64), ((Ho, Wo), torch.int32), ((Ho, Wo), torch.uint16), ((Ho, Wo, 3), torch.uint8))
    acc, index, count, bgr = out.out
    assert lib().iamx_ortho_clear(0, Ho, Wo, _p(acc), _p(index), _p(count), _p(bgr), stream_ptr()) == 0
    return out


@pytest.mark.parametrize('ss', [1, 3])
def test_the_owner_pass_leaves_what_mode_best_leaves(ss):
    dsm, x0, y1, gsd = bumpy(33, 17, 3)
    cams, frames = five_images()
    Ho, Wo = 33 * ss, 17 * ss
    d = behind_nan(dsm)
    a, b = cleared(Ho, Wo), cleared(Ho, Wo)
    whole = (0, 0, Wo - 1, Ho - 1)
    for k, (cam, frame) in enumerate(zip(cams, frames)):
        params = image_params(dsm, x0, y1, gsd, 0.6, cam, frame)
        kernels.ortho_dsm_owner(d, ss, params, frame.shape[:2], k, whole, a.out[0], a.out[1], a.out[2])
        kernels.ortho_dsm_image(0, d, ss, params, torch.from_numpy(np.array(frame)).cuda(), k, whole, *b.out)
    torch.cuda.synchronize()
    metric, index, count, bgr = a.check()
    acc, index_b, count_b, _bgr = b.check()
    assert index.tobytes() == index_b.tobytes() and count.tobytes() == count_b.tobytes() and metric.tobytes() == acc.tobytes()
    assert not bgr.any() and (index >= 0).mean() > 0.9 and len(np.unique(index)) >= 4


# ---- 3. sizes around the tile and the level rule ----
@pytest.mark.parametrize('size,levels', [((1, 1), 1), ((15, 17), 6), ((16, 16), 5), ((17, 33), 7)])
def test_sizes_around_the_tile_and_the_level_rule(size, levels):
    if size == (1, 1):
        dsm, x0, y1, gsd = np.array([[2.5]], np.float32), -1.0, 1.0, 2.0
    else:
        dsm, x0, y1, gsd = bumpy(size[0], size[1], 7)
    cams, frames = FOUR[:3], [oc.hash_frame(k) for k in range(3)]
    want, _comp = both(dsm, x0, y1, gsd, cams, frames, 1, 0.6, 16)
    assert want['bands'] == levels and (want['count'] > 0).mean() > 0.9
    assert [n.shape[:2] for n in want['N']][-1] == (1, 1)


# ---- 4. edges ----
def test_an_empty_work_box_and_a_view_that_never_wins():
    dsm, x0, y1, gsd = bumpy(24, 20, 3)
    cams = [FOUR[0], camera(AWAY), FOUR[1], camera(FAR, R=look_at(FAR, (0.0, 0.0, 0.0)))]
    frames = [oc.hash_frame(k) for k in range(4)]
    for ss in (1, 2):
        want, comp = both(dsm, x0, y1, gsd, cams, frames, ss, 0.6, 5)
        box = comp.images[1][1]
        assert box[2] < box[0] or box[3] < box[1]
        covered = ms.cover(dsm, x0, y1, gsd, ss, restated(cams[3], frames[3]), (64, 96))[0]
        assert covered.sum() >= 480 and not (want['index'] == 3).any() and not (want['index'] == 1).any()
        without = ms.compose(dsm, x0, y1, gsd, [restated(c, f) for c, f in zip(cams[:3], frames)], frames[:3], bands=5,
                             ss=ss, bias=0.6)
        assert without['bgr'].tobytes() == want['bgr'].tobytes() and (want['count'] > without['count']).any()


def test_twins_the_earlier_owns_and_both_count():
    dsm, x0, y1, gsd = bumpy(24, 20, 6)
    want, _comp = both(dsm, x0, y1, gsd, [FOUR[1], FOUR[1]], [oc.hash_frame(0), oc.hash_frame(1)], 2, 0.6, 5)
    on = want['count'] > 0
    assert on.any() and (want['count'][on] == 2).all() and (want['index'][on] == 0).all()


@pytest.mark.parametrize('ss', [1, 3])
def test_holes_in_the_dsm(ss):
    dsm, x0, y1, gsd = bumpy(24, 20, 8, holes=12)
    assert np.isnan(dsm).sum() > 12
    cams, frames = five_images()
    want, _comp = both(dsm, x0, y1, gsd, cams[:3], frames[:3], ss, 0.6, 5)
    empty = want['count'] == 0
    assert empty.any() and not want['bgr'][empty].any() and (want['count'] > 0).mean() > 0.5
    if ss == 1:
        assert empty[np.isnan(dsm)].all()


def layer_of(dsm, x0, y1, gsd, ss, bias, cam, frame, k, index, box):
    """the restatement's layer of image k cut to the box -> float32 [rows][cols][4]"""
    on, fu, fv = ms.cover(dsm, x0, y1, gsd, ss, restated(cam, frame), frame.shape[:2])
    C, A = ms.layer(k, on, fu, fv, index, frame)
    c0, r0, c1, r1 = box
    return np.concatenate([C, A], axis=2)[r0:r1 + 1, c0:c1 + 1]


@pytest.mark.parametrize('which', ['last row and column', 'one pixel', 'across a tile edge', 'whole'])
def test_the_layer_kernel_writes_its_box_and_nothing_else(which):
    ss = 3
    dsm, x0, y1, gsd = bumpy(24, 20, 8, holes=6)
    Ho, Wo = 24 * ss, 20 * ss
    box = {'last row and column': (Wo - 5, Ho - 3, Wo - 1, Ho - 1), 'one pixel': (17, 40, 17, 40),
           'across a tile edge': (13, 14, 18, 17), 'whole': (0, 0, Wo - 1, Ho - 1)}[which]
    cams, frames = five_images()
    best = rs.compose(dsm, x0, y1, gsd, [restated(c, f) for c, f in zip(cams, frames)], frames, 'best', ss=ss, bias=0.6)
    index = torch.from_numpy(best['index']).cuda()
    d = behind_nan(dsm)
    rows, cols = box[3] - box[1] + 1, box[2] - box[0] + 1
    for k in (4, 2, 0):
        out = Guarded(((rows * cols, 4), torch.float32))
        params = image_params(dsm, x0, y1, gsd, 0.6, cams[k], frames[k])
        kernels.ortho_dsm_layer(d, ss, params, torch.from_numpy(np.array(frames[k])).cuda(), k, box, index, out.out[0])
        torch.cuda.synchronize()
        got = out.check()[0].reshape(rows, cols, 4)
        want = layer_of(dsm, x0, y1, gsd, ss, 0.6, cams[k], frames[k], k, best['index'], box)
        assert dc.bits(got).tobytes() == dc.bits(want).tobytes(), (which, k)
    if which == 'whole':
        assert (want[:, :, 3] == 1).any() and (want[:, :, :3].any(axis=2) & (want[:, :, 3] == 0)).any()


def test_the_owner_kernel_on_small_boxes():
    ss = 3
    dsm, x0, y1, gsd = bumpy(24, 20, 3)
    Ho, Wo = 24 * ss, 20 * ss
    cam, frame = FOUR[0], oc.hash_frame(0)
    params = image_params(dsm, x0, y1, gsd, 0.6, cam, frame)
    d = behind_nan(dsm)
    for box in ((5, 7, 4, 7), (5, 7, 5, 6), (17, 40, 17, 40), (59, 71, 59, 71), (13, 14, 18, 17)):
        out = cleared(Ho, Wo)
        kernels.ortho_dsm_owner(d, ss, params, frame.shape[:2], 0, box, out.out[0], out.out[1], out.out[2])
        torch.cuda.synchronize()
        metric, index, count, _bgr = out.check()
        want = rs.compose(dsm, x0, y1, gsd, [restated(cam, frame)], [frame], 'best', ss=ss, bias=0.6, boxes=[box])
        assert index.tobytes() == want['index'].tobytes() and count.tobytes() == want['count'].tobytes(), box
        assert metric.tobytes() == want['acc'].tobytes(), box


# ---- 5. refusals through the C ABI ----
def test_bad_arguments_return_the_error_code_and_write_nothing():
    L = lib()
    dsm, x0, y1, gsd = bumpy(24, 20, 3)
    d = behind_nan(dsm)
    frame = torch.from_numpy(np.array(oc.hash_frame(0))).cuda()
    params = image_params(dsm, x0, y1, gsd, 0.5, FOUR[0], oc.hash_frame(0))
    pp = params.ctypes.data_as(ctypes.c_void_p)
    nan = params.copy()
    nan[3] = np.nan
    inf = params.copy()
    inf[17] = np.inf
    index = torch.zeros((24, 20), dtype=torch.int32, device='cuda')
    lay = Guarded(((24 * 20 + 1, 4), torch.float32))
    layer = lay.out[0]

    def call_layer(dsm=d, H=24, W=20, ss=1, params=pp, frame=frame, h_s=64, w_s=96, box=(0, 0, 19, 23), index=index,
                   layer=_p(layer)):
        return L.iamx_ortho_dsm_layer(_p(dsm), H, W, ss, params, _p(frame), h_s, w_s, 0, box[0], box[1], box[2], box[3],
                                      _p(index), layer, stream_ptr())

    bad = [dict(layer=None), dict(layer=ctypes.c_void_p(layer.data_ptr() + 4)), dict(layer=ctypes.c_void_p(layer.data_ptr() + 8)),
           dict(dsm=None), dict(params=None), dict(frame=None), dict(index=None), dict(ss=0), dict(ss=9), dict(H=0), dict(W=0),
           dict(h_s=1), dict(w_s=1), dict(box=(0, 0, 20, 23)), dict(box=(0, 0, 19, 24)), dict(box=(-1, 0, 19, 23)),
           dict(box=(0, -1, 19, 23)), dict(params=nan.ctypes.data_as(ctypes.c_void_p)),
           dict(params=inf.ctypes.data_as(ctypes.c_void_p))]
    for kw in bad:
        assert call_layer(**kw) == EINVAL, kw
    assert call_layer(box=(3, 3, 2, 3)) == 0 and call_layer(box=(3, 3, 3, 2)) == 0          # an empty box succeeds
    own = Guarded(((24, 20), torch.float64), ((24, 20), torch.int32), ((24, 20), torch.uint16))
    metric, oindex, count = own.out

    def call_owner(dsm=d, H=24, W=20, ss=1, params=pp, h_s=64, w_s=96, box=(0, 0, 19, 23), metric=metric, index=oindex,
                   count=count):
        return L.iamx_ortho_dsm_owner(_p(dsm), H, W, ss, params, h_s, w_s, 0, box[0], box[1], box[2], box[3], _p(metric),
                                      _p(index), _p(count), stream_ptr())

    bad = [dict(dsm=None), dict(params=None), dict(metric=None), dict(index=None), dict(count=None), dict(ss=0), dict(ss=9),
           dict(H=0), dict(W=0), dict(h_s=1), dict(w_s=1), dict(box=(0, 0, 20, 23)), dict(box=(0, 0, 19, 24)),
           dict(box=(-1, 0, 19, 23)), dict(box=(0, -1, 19, 23)), dict(params=nan.ctypes.data_as(ctypes.c_void_p)),
           dict(params=inf.ctypes.data_as(ctypes.c_void_p))]
    for kw in bad:
        assert call_owner(**kw) == EINVAL, kw
    assert call_owner(box=(3, 3, 2, 3)) == 0 and call_owner(box=(3, 3, 3, 2)) == 0
    torch.cuda.synchronize()
    assert lay.untouched() and own.untouched()


# ---- 6. render_dense(bands=) ----
def slope_surface():
    n, e = np.meshgrid(60.0 - (np.arange(60) + 0.5) * 2.0, -60.0 + (np.arange(60) + 0.5) * 2.0, indexing='ij')
    dsm = (-(0.15 * n + 0.1 * e)).astype(np.float32)            # the slope scene: down = 0.15 north + 0.1 east
    dsm[20:24, 30:36] += 8.0
    return dsm, dense.Surface(dsm, np.zeros(dsm.shape, np.int32), -60.0, 60.0, 2.0)


def test_render_dense_with_bands_on_a_stand_in_project(monkeypatch):
    from imageanalysis_amd import histogram
    from imageanalysis_amd.hostlib import camera as cam_mod
    proj = dc.standin_project()
    frames = dc.project_frames(proj)
    dsm, surface = slope_surface()
    dev = _dev(frames)
    K = np.asarray(cam_mod.get_K(optimized=True), np.float64)
    width, height = cam_mod.get_image_params()
    cams = [(K, width, height, np.array(dc.DIST), ) + dense.image_pose(im) for im in proj.image_list]
    for prefilter in (False, True):
        with contextlib.redirect_stdout(io.StringIO()):
            m = ortho.render_dense(proj, [dc.NAMES], 0, surface, upsample=1, bias=1.0, prefilter=prefilter, frames=dev, bands=5)
        assert ortho.render_dense_stats['prefiltered'] == (4 if prefilter else 0)
        ready = dev
        if prefilter:                                       # native 0.29 m against 2 m pixels: shrunk to 74 x 56
            z_mean = ortho.surface_heights(torch.from_numpy(dsm).cuda())[2]
            factors = [ortho.dense_prefilter_factor(K, c[5], z_mean, 2.0) for c in cams]
            ready = [kernels.resize_area(f, v, v) for f, v in zip(dev, factors)]
            assert ready[0].shape[0] < 100
        want = ortho.compose_dense(surface, cams, ready, upsample=1, bias=1.0, bands=5)
        assert (m.mode, m.bands, m.surface, m.names) == ('multiband', 5, 'dense', dc.NAMES)
        assert m.bgr.cpu().numpy().tobytes() == want.bgr.cpu().numpy().tobytes() and torch.equal(m.index, want.index)
        assert u16(m.count).tobytes() == u16(want.count).tobytes() and (u16(m.count) > 0).mean() > 0.5
    # the frames as the decoder would deliver them: the sizes come from the camera's image size
    monkeypatch.setattr(histogram, 'frame_pass', lambda images, want_hist, on_frames: on_frames(dev))
    with contextlib.redirect_stdout(io.StringIO()):
        decoded = ortho.render_dense(proj, [dc.NAMES], 0, surface, upsample=1, bias=1.0, bands=5)
    assert decoded.bgr.cpu().numpy().tobytes() == m.bgr.cpu().numpy().tobytes()
    odd = [dev[0], dev[1][:-2].contiguous(), dev[2], dev[3]]
    monkeypatch.setattr(histogram, 'frame_pass', lambda images, want_hist, on_frames: on_frames(odd))
    with pytest.raises(RuntimeError, match=dc.NAMES[1]), contextlib.redirect_stdout(io.StringIO()):
        ortho.render_dense(proj, [dc.NAMES], 0, surface, upsample=1, bias=1.0, bands=5)


def test_a_frame_of_another_size_accumulates_nothing():
    dsm, x0, y1, gsd = bumpy(24, 20, 3)
    cams, frames = five_images()
    comp = ortho._DenseComposer(surface_of(dsm, x0, y1, gsd), 'best', 2, 0.6, list('abcde'), 5, cams,
                                [f.shape[:2] for f in frames])
    comp.add(0, cams[0], frames[0])
    before = [(N.cpu().numpy().copy(), D.cpu().numpy().copy()) for N, D in comp.accumulators()]
    assert any(D.any() for _N, D in before)
    with pytest.raises(RuntimeError, match='b: a 48 x 32 frame'):
        comp.add(1, cams[1], frames[4])
    torch.cuda.synchronize()
    for (N0, D0), (N, D) in zip(before, comp.accumulators()):
        assert dc.bits(N.cpu().numpy()).tobytes() == dc.bits(N0).tobytes() and dc.bits(D.cpu().numpy()).tobytes() == dc.bits(D0).tobytes()


# ---- 7. the command line ----
def frame_sized_camera():
    """the configured camera at the size of the test frames, 96 x 64, K as dense.scaled_K scales it: the
    blend is told the frames' size by the camera (the stand-in project's own camera is 5472 x 3648)
    -> what undoes it"""
    from imageanalysis_amd.hostlib import camera as cam_mod
    w0, h0 = cam_mod.get_image_params()
    before = [np.asarray(cam_mod.get_K(optimized=opt), np.float64) for opt in (False, True)]
    for opt, K in zip((False, True), before):
        cam_mod.set_K(*rs.scaled_K(K, w0, h0, oc.FRAME_W, oc.FRAME_H), optimized=opt)
    cam_mod.set_image_params(oc.FRAME_W, oc.FRAME_H)

    def undo():
        for opt, K in zip((False, True), before):
            cam_mod.set_K(K[0, 0], K[1, 1], K[0, 2], K[1, 2], optimized=opt)
        cam_mod.set_image_params(w0, h0)
    return undo


def test_script_with_bands(project, tmp_path):
    """5e-true-ortho.py in processes of its own: --bands 3 writes the blended mosaic render_dense(bands=3)
    makes here; without --bands its files are a mode best run's, byte for byte; --mode feather --bands 3
    is refused with the script's error code before anything is written"""
    undo = frame_sized_camera()
    try:
        _script_with_bands(project, tmp_path)
    finally:
        undo()


def _script_with_bands(project, tmp_path):
    import json
    import os
    import shutil
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
        if name == 'project.py':                            # (the same camera in the script's process)
            text += '        import test_ortho_dense_multiband_gpu as here\n        here.frame_sized_camera()\n'
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
    grids = oc.scene_input('step5_mid_default')[1]
    rf = ortho.raster_frame(grids, 4.0)
    dsm = np.full((rf.H, rf.W), np.float32(np.nanmean(grids[:, :, 2])), np.float32)
    dsm[10:16, 20:30] += np.float32(15.0)
    dsm[30:35, 40:45] = np.nan
    dense.save(dense.Surface(torch.from_numpy(dsm).cuda(), torch.ones(dsm.shape, dtype=torch.int32, device='cuda'),
                             rf.x0, rf.y1, 4.0), str(analysis))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / 'standin'), s5.REPO, os.path.join(s5.REPO, 'tests')]))
    script = os.path.join(s5.REPO, 'imageanalysis_amd', 'scripts', '5e-true-ortho.py')
    base = ['timeout', '-k', '10', '120', sys.executable, script, str(pdir), '--upsample', '2', '--bias', '1.5',
            '--fill-rounds', '3', '--tile', '128', '--format', 'png']
    out = analysis / 'true_ortho'
    filled, _round_of = dense.fill(dense.load(str(analysis)), rounds=3)

    def files():
        return {p.name: p.read_bytes() for p in sorted(out.iterdir())}

    # refused: the error code, nothing written
    p = subprocess.run(base + ['--mode', 'feather', '--bands', '3'], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 1 and '--bands' in p.stderr and not out.exists()
    # without --bands: a mode best run's files
    p = subprocess.run(base, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Blended' not in p.stdout
    plain = files()
    with contextlib.redirect_stdout(io.StringIO()):
        best = ortho.render_dense(proj, g['groups'], 0, filled, mode='best', upsample=2, bias=1.5, frames=_dev(decoded))
    ortho.save(best, str(tmp_path / 'here'), tile=128, fmt='png', subdir='true_ortho')
    here = {p.name: p.read_bytes() for p in sorted((tmp_path / 'here' / 'true_ortho').iterdir())}
    assert sorted(plain) == sorted(here) and len(plain) > 3
    for name in plain:                                      # (ned_reference is the process's own setting)
        if name == 'ortho.json':
            a, b = json.loads(plain[name]), json.loads(here[name])
            assert a.pop('ned_reference') is not None and b.pop('ned_reference') is not None and a == b
            assert a['mode'] == 'best' and 'bands' not in a
        else:
            assert plain[name] == here[name], name
    shutil.rmtree(str(out))
    # --bands 3
    p = subprocess.run(base + ['--bands', '3'], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Blended over 3 pyramid levels' in p.stdout and 'Wrote' in p.stdout
    info = json.loads((out / 'ortho.json').read_text())
    assert (info['mode'], info['bands'], info['surface'], info['upsample'], info['bias'], info['images']) == (
        'multiband', 3, 'dense', 2, 1.5, names)
    with contextlib.redirect_stdout(io.StringIO()):
        want = ortho.render_dense(proj, g['groups'], 0, filled, upsample=2, bias=1.5, frames=_dev(decoded), bands=3)
    want = want.bgr.cpu().numpy()
    assert (want.sum(axis=2) > 0).mean() > 0.5 and want.tobytes() != best.bgr.cpu().numpy().tobytes()
    for t in info['tiles']:
        with Image.open(str(out / t['file'])) as im:
            px = np.asarray(im.convert('RGB'))[:, :, ::-1]
        r0, c0 = t['row'] * 128, t['col'] * 128
        assert px.tobytes() == np.ascontiguousarray(want[r0:r0 + t['height'], c0:c0 + t['width']]).tobytes(), t['file']
