"""CPU: the true-ortho rules do what a true orthophoto must (tests/ortho_dense_restatement.py against
analytic shadows, planar slopes and an exact drape), the host's work box loses nothing, the fill rule,
the host errors of ortho.compose_dense / dense.fill and the files."""
import json
import os

import numpy as np
import pytest

import dense_common as dc
import ortho_common as oc
import ortho_dense_restatement as rs
from imageanalysis_amd import dense, ortho

CAMERAS = ((0.0, 30.0, -100.0), (28.0, 3.0, -100.0), (-25.0, -20.0, -100.0), (0.0, 120.0, -60.0), (70.0, -90.0, -50.0))
ROOF_N, ROOF_E, ROOF_UP = dc.ROOF


def roof_dsm(cells=96, gsd=1.0):
    """dense_common's roof sampled at cell centres -> (dsm float32, x0, y1, gsd)"""
    x0, y1 = -0.5 * cells * gsd, 0.5 * cells * gsd
    e = x0 + (np.arange(cells) + 0.5) * gsd
    n = y1 - (np.arange(cells) + 0.5) * gsd
    on = (np.abs(n)[:, None] < ROOF_N) & (np.abs(e)[None, :] < ROOF_E)
    return np.where(on, ROOF_UP, 0.0).astype(np.float32), x0, y1, gsd


def centres(x0, y1, gsd, H, W, ss):
    g = gsd / ss
    return (y1 - (np.arange(H * ss) + 0.5) * g)[:, None], (x0 + (np.arange(W * ss) + 0.5) * g)[None, :]


def occl(n, e, cam, half_n, half_e, top):
    """slab test: the segment from the ground point (n, e, 0) to the camera crosses the box
    |north| < half_n, |east| < half_e below `top`"""
    n, e = np.broadcast_arrays(n, e)
    lo = np.zeros(n.shape)
    hi = np.full(n.shape, min(1.0, top / -cam[2]))
    for p, c, half in ((n, cam[0], half_n), (e, cam[1], half_e)):
        d = c - p
        with np.errstate(divide='ignore', invalid='ignore'):
            t1, t2 = (-half - p) / d, (half - p) / d
        flat = d == 0
        lo = np.where(flat, np.where(np.abs(p) < half, lo, np.inf), np.maximum(lo, np.minimum(t1, t2)))
        hi = np.where(flat, hi, np.minimum(hi, np.maximum(t1, t2)))
    return lo < hi


@pytest.mark.parametrize('ss', [1, 2, 3])
@pytest.mark.parametrize('bias', [0.5, 1.5])
def test_march_is_sandwiched_by_analytic_shadows(bias, ss):
    """Undecided band and decided-occluded pixels per case are printed; a numpy prototype of the march
    (not this code) had at most 0.057 of the mosaic undecided and at least 128 pixels decided."""
    dsm, x0, y1, gsd = roof_dsm()
    n, e = centres(x0, y1, gsd, 96, 96, ss)
    ground = ~((np.abs(n) < 16) & (np.abs(e) < 21))
    for cam in CAMERAS:
        got, _h = rs.march(dsm, x0, y1, gsd, ss, bias, np.array(cam))
        big, small = occl(n, e, cam, 16, 21, ROOF_UP), occl(n, e, cam, 14, 19, ROOF_UP - bias)
        undecided = float((ground & big & ~small).mean())
        decided = int((ground & small).sum())
        print('camera %r bias %.1f ss %d: undecided %.4f of the mosaic, decided occluded %d' % (cam, bias, ss, undecided, decided))
        assert not (got & ground & ~big).any()
        assert not (ground & small & ~got).any()
        assert not (got & (np.abs(n) < 14) & (np.abs(e) < 19)).any()
        assert undecided <= 0.08
        assert decided > 0


@pytest.mark.parametrize('ss', [1, 2])
@pytest.mark.parametrize('bias', [0.0, 0.5, 1.5])
@pytest.mark.parametrize('slope', [(0.15, 0.1), (0.7, 0.7), (1.0, 0.0)])
def test_planar_slopes_hide_nothing(slope, bias, ss):
    n, e = centres(-32.0, 32.0, 1.0, 64, 64, 1)
    dsm = (slope[0] * n + slope[1] * e).astype(np.float32)
    for cam in (CAMERAS[0], CAMERAS[2]):
        got, h = rs.march(dsm, -32.0, 32.0, 1.0, ss, bias, np.array(cam))
        assert got.shape == (64 * ss, 64 * ss) and not np.isnan(h).any()
        assert int(got.sum()) == 0


def test_exact_drape_of_a_nadir_camera():
    """focal length = height above the surface = 32 (a power of two, so x / z * f is exact): mosaic
    pixel (r, c) projects onto frame pixel (c + 12, r + 5) exactly"""
    frame = oc.hash_frame(0)
    dsm = np.full((12, 16), 4.0, np.float32)
    cam = (np.array([32.0, 32.0, 20.0, 10.0]), np.zeros(5), dc.NADIR, np.array([0.5, 0.5, -36.0]))
    for mode in ('best', 'feather'):
        out = rs.compose(dsm, -8.0, 6.0, 1.0, [cam], [frame], mode, ss=1, bias=0.5)
        assert out['bgr'].tobytes() == np.ascontiguousarray(frame[5:17, 12:28]).tobytes()
        assert (out['count'] == 1).all()
    out = rs.compose(dsm, -8.0, 6.0, 1.0, [cam], [frame], 'best', ss=1, bias=0.5)
    assert (out['index'] == 0).all() and out['index'].dtype == np.int32 and out['count'].dtype == np.uint16


def roof_cameras(frame_hw=(oc.FRAME_H, oc.FRAME_W), dist=dc.DIST, focal=dc.FOCAL):
    h, w = frame_hw
    K = np.array([focal, focal, (w - 1) / 2.0, (h - 1) / 2.0])
    return [(K, np.array(dist, float), dc.NADIR, np.array(c)) for c in CAMERAS[:3]]


def test_no_pixel_is_coloured_from_a_view_that_cannot_see_it():
    dsm, x0, y1, gsd = roof_dsm()
    bias = 0.5
    cams = roof_cameras()
    out = rs.compose(dsm, x0, y1, gsd, cams, [oc.hash_frame(k) for k in range(3)], 'best', ss=1, bias=bias)
    n, e = centres(x0, y1, gsd, 96, 96, 1)
    ground = ~((np.abs(n) < 16) & (np.abs(e) < 21))
    assert (out['index'] >= 0).mean() > 0.9
    for k, cam in enumerate(CAMERAS[:3]):
        hidden = ground & occl(n, e, cam, 14, 19, ROOF_UP - bias)
        assert hidden.sum() > 100
        assert not (out['index'][hidden] == k).any()
        assert not out['visible'][k][hidden].any()
    # without the test (a bias no roof reaches) the nearest view would colour part of its own shadow
    blind = rs.compose(dsm, x0, y1, gsd, cams, [oc.hash_frame(k) for k in range(3)], 'best', ss=1, bias=1e6)
    assert any((blind['index'][ground & occl(n, e, cam, 14, 19, ROOF_UP - bias)] == k).any()
               for k, cam in enumerate(CAMERAS[:3]))


BOX_CAMERAS = {'distorted': ((0.02, -0.03, 0.01), (5.0, -8.0, -40.0)),
               'pitched': ((0.3, 0.5, 0.0), (-10.0, 6.0, -40.0)),
               'horizon': ((0.0, 1.0, 0.0), (0.0, 0.0, -40.0))}


@pytest.mark.parametrize('which', sorted(BOX_CAMERAS))
def test_the_work_box_loses_nothing(which):
    dsm, x0, y1, gsd = roof_dsm(48, 2.0)
    ss, h, w = 2, 48, 64
    angles, C = BOX_CAMERAS[which]
    R, C = dc._rot(*angles).dot(dc.NADIR), np.array(C)
    K = np.array([dc.FOCAL, dc.FOCAL, (w - 1) / 2.0, (h - 1) / 2.0])
    cam = (K, np.array(dc.DIST), R, C)
    border = ortho.border_pixels(w, h)
    assert len(border) == len(set(map(tuple, border))) and {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (32, 0)} <= set(map(tuple, border))
    rays = dc.host_rays(K, dc.DIST, h, w)[border[:, 1], border[:, 0]]
    box = ortho.work_box(K, dc.DIST, R, C, w, h, 0.0, float(ROOF_UP), x0, y1, gsd / ss, 96, 96, rays=rays)
    if which == 'horizon':
        assert box == (0, 0, 95, 95)
    else:
        assert 0 < (box[2] - box[0] + 1) * (box[3] - box[1] + 1) < 96 * 96
    frame = oc.hash_frame(1, h, w)
    for mode in ('best', 'feather'):
        whole = rs.compose(dsm, x0, y1, gsd, [cam], [frame], mode, ss=ss, bias=1.0)
        boxed = rs.compose(dsm, x0, y1, gsd, [cam], [frame], mode, ss=ss, bias=1.0, boxes=[box])
        assert whole['count'].sum() > 200
        for key in ('acc', 'index', 'count', 'bgr'):
            if whole[key] is not None:
                assert np.ascontiguousarray(whole[key]).tobytes() == np.ascontiguousarray(boxed[key]).tobytes(), key


# ---- fill ----
def test_fill_an_isolated_hole():
    z = np.arange(25, dtype=np.float32).reshape(5, 5) * np.float32(0.1)
    z[2, 2] = np.nan
    got, round_of = rs.fill(z, 3)
    s = np.float32(0)
    for k, (r, c) in enumerate([(1, 1), (1, 2), (1, 3), (2, 1), (2, 3), (3, 1), (3, 2), (3, 3)]):
        s = z[r, c] if k == 0 else np.float32(s + z[r, c])
    assert got[2, 2] == np.float32(np.float64(s) / 8.0) and got.dtype == np.float32
    want = np.zeros((5, 5), np.uint8)
    want[2, 2] = 1
    assert np.array_equal(round_of, want)
    z[2, 2] = got[2, 2]
    assert np.array_equal(got, z)                           # finite cells never change


def test_fill_a_wide_hole_keeps_its_middle_and_a_corner_counts_its_own_neighbours():
    z = np.ones((9, 11), np.float32)
    z[1:8, 1:10] = np.nan                                   # 7 x 9: wider than 2 rounds from both sides
    z[0, 0] = np.nan
    got, round_of = rs.fill(z, 2)
    assert round_of[0, 0] == 1 and got[0, 0] == 1.0         # two finite neighbours of three existing cells
    assert (round_of[1, 1:10] == 1).all() and (round_of[2, 2:9] == 2).all() and (round_of[3:6, 3:8] == 255).all()
    assert np.isnan(got[round_of == 255]).all() and not np.isnan(got[round_of != 255]).any()
    more, round_more = rs.fill(z, 8)
    assert round_more.max() == 4 and not np.isnan(more).any()


def test_fill_rounds_zero_and_refusals():
    z = np.array([[1.0, np.nan], [np.nan, 2.0]], np.float32)
    got, round_of = rs.fill(z, 0)
    assert dc.bits(got).tobytes() == dc.bits(z).tobytes() and round_of.tolist() == [[0, 255], [255, 0]]
    empty = np.full((3, 4), np.nan, np.float32)
    for fn in (rs.fill, lambda d, r: dense.fill(dense.Surface(d, np.zeros(d.shape, np.int32), 0.0, 0.0, 1.0), r)):
        with pytest.raises(ValueError):
            fn(empty, 2)
        with pytest.raises(ValueError):
            fn(z, -1)
        with pytest.raises(ValueError):
            fn(z, 255)


# ---- host errors: a ValueError before any device call (there is no device here) ----
def test_host_errors():
    dsm, x0, y1, gsd = roof_dsm(8, 1.0)
    surface = dense.Surface(dsm, np.zeros(dsm.shape, np.int32), x0, y1, gsd)
    cam = (np.array([[40.0, 0, 47.5], [0, 40.0, 31.5], [0, 0, 1]]), 96, 64, np.zeros(5), dc.NADIR, np.array([0.0, 0.0, -50.0]))
    rcam = (np.array([40.0, 40.0, 47.5, 31.5]), np.zeros(5), dc.NADIR, np.array([0.0, 0.0, -50.0]))
    frame = oc.hash_frame(0)
    for bad in (dict(upsample=0), dict(upsample=9), dict(upsample=1.5), dict(bias=-0.1), dict(bias=float('nan')),
                dict(bias=float('inf')), dict(mode='multiband'), dict(mode='nearest')):
        with pytest.raises(ValueError):
            ortho.compose_dense(surface, [cam], [frame], **bad)
        kw = dict(bad)
        if 'upsample' in kw:
            kw['ss'] = kw.pop('upsample')
        with pytest.raises(ValueError):
            rs.compose(dsm, x0, y1, gsd, [rcam], [frame], **kw)
    for thin in (np.zeros((1, 7, 3), np.uint8), np.zeros((7, 1, 3), np.uint8), np.zeros((4, 4), np.uint8)):
        with pytest.raises(ValueError, match='2 x 2'):
            ortho.compose_dense(surface, [cam], [thin])
        with pytest.raises(ValueError):
            rs.compose(dsm, x0, y1, gsd, [rcam], [thin])
    with pytest.raises(ValueError):
        ortho.compose_dense(surface, [cam, cam], [frame])


# ---- files ----
def _reference_node():
    from imageanalysis_amd._deps import getNode
    ref = getNode('/config/ned_reference', True)
    for k, v in (('lat_deg', 44.5), ('lon_deg', -93.25), ('alt_m', 278.0)):
        ref.setFloat(k, v)


def test_load_is_the_inverse_of_save(tmp_path):
    import torch
    _reference_node()
    rng = np.random.default_rng(4)
    dsm = rng.normal(280.0, 3.0, (7, 9)).astype(np.float32)
    dsm[2, 3] = np.nan
    count = rng.integers(0, 9, (7, 9)).astype(np.int32)
    s = dense.Surface(torch.from_numpy(dsm), torch.from_numpy(count), -12.3, 40.7, 0.3)
    dense.save(s, str(tmp_path))
    back = dense.load(str(tmp_path), device='cpu')
    assert (back.x0, back.y1, back.gsd, back.shape) == (-12.3, 40.7, 0.3, (7, 9))
    assert back.dsm.dtype == torch.float32 and back.count.dtype == torch.int32
    assert dc.bits(back.dsm.numpy()).tobytes() == dc.bits(dsm).tobytes() and np.array_equal(back.count.numpy(), count)
    with pytest.raises(FileNotFoundError):
        dense.load(str(tmp_path / 'nowhere'), device='cpu')


class _HostMosaic(object):
    def __init__(self, bgr, **kw):
        import torch
        self.bgr = torch.from_numpy(bgr)
        self.index = self.count = None
        self.x0, self.y1, self.gsd, self.mode, self.names = -12.5, 40.0, 0.25, 'best', ['a.JPG']
        self.shape = bgr.shape[:2]
        self.__dict__.update(kw)


def test_save_writes_the_new_keys_only_for_a_dense_mosaic(tmp_path):
    _reference_node()
    bgr = oc.hash_frame(3, 20, 30).copy()
    old = ortho.save(_HostMosaic(bgr), str(tmp_path), tile=16, fmt='png')
    assert not {'surface', 'upsample', 'bias'} & set(old) and os.path.isdir(str(tmp_path / 'ortho'))
    assert list(json.loads((tmp_path / 'ortho' / 'ortho.json').read_text())) == [
        'ned_reference', 'units', 'gsd', 'mode', 'width', 'height', 'tile', 'format', 'bounds', 'tiles', 'images']
    m = ortho.Mosaic(bgr=_HostMosaic(bgr).bgr, index=None, count=None, x0=-12.5, y1=40.0, gsd=0.25, mode='best', names=['a.JPG'])
    assert (m.surface, m.upsample, m.bias) == (None, None, None)
    again = ortho.save(m, str(tmp_path / 'again'), tile=16, fmt='png')
    assert again == old
    assert (tmp_path / 'again' / 'ortho' / 'ortho.json').read_bytes() == (tmp_path / 'ortho' / 'ortho.json').read_bytes()
    new = ortho.save(_HostMosaic(bgr, surface='dense', upsample=2, bias=0.5), str(tmp_path), tile=16, fmt='png',
                     subdir='true_ortho')
    assert (new['surface'], new['upsample'], new['bias']) == ('dense', 2, 0.5)
    assert json.loads((tmp_path / 'true_ortho' / 'ortho.json').read_text()) == new
    assert {k: v for k, v in new.items() if k not in ('surface', 'upsample', 'bias')} == old
