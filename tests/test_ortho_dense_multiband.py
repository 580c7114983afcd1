"""CPU: the true orthophoto's blend (ortho.compose_dense(bands=)) -- the host's argument checks, and
what the rules of tests/ortho_dense_multiband_restatement.py do on the roof scene: a single image stays
mode best, flat frames stay inside their range (and would not with a layer of the visible pixels
only), the seam goes, a view that never wins changes nothing, holes stay empty; the files."""
import json

import numpy as np
import pytest

import dense_common as dc
import ortho_common as oc
import ortho_dense_multiband_restatement as ms
import ortho_dense_restatement as rs
from imageanalysis_amd import dense, ortho
from test_ortho_dense import _HostMosaic, _reference_node, roof_cameras, roof_dsm

BIAS = 0.5
FLAT = (100, 200, 150)


def flat_scene():
    """the roof at 96 x 96, the first three cameras at focal 150 with flat 400 x 400 frames: every
    camera covers the whole mosaic"""
    dsm, x0, y1, gsd = roof_dsm()
    cams = roof_cameras((400, 400), focal=150.0)
    frames = [np.full((400, 400, 3), v, np.uint8) for v in FLAT]
    return dsm, x0, y1, gsd, cams, frames


@pytest.fixture(scope='module')
def flat():
    return flat_scene()


@pytest.fixture(scope='module')
def flat_best(flat):
    dsm, x0, y1, gsd, cams, frames = flat
    return rs.compose(dsm, x0, y1, gsd, cams, frames, 'best', ss=1, bias=BIAS)


@pytest.fixture(scope='module')
def flat_five(flat):
    dsm, x0, y1, gsd, cams, frames = flat
    return ms.compose(dsm, x0, y1, gsd, cams, frames, bands=5, ss=1, bias=BIAS)


# ---- 1. argument checks: a ValueError before any device call (there is no device here) ----
def test_argument_checks():
    dsm, x0, y1, gsd = roof_dsm(8, 1.0)
    surface = dense.Surface(dsm, np.zeros(dsm.shape, np.int32), x0, y1, gsd)
    cam = (np.array([[40.0, 0, 47.5], [0, 40.0, 31.5], [0, 0, 1]]), 96, 64, np.zeros(5), dc.NADIR, np.array([0.0, 0.0, -50.0]))
    rcam = (np.array([40.0, 40.0, 47.5, 31.5]), np.zeros(5), dc.NADIR, np.array([0.0, 0.0, -50.0]))
    frame = oc.hash_frame(0)
    for bands in (-1, 17, 1.5, True):
        with pytest.raises(ValueError, match='bands'):
            ortho.compose_dense(surface, [cam], [frame], bands=bands)
        with pytest.raises(ValueError):
            ms.compose(dsm, x0, y1, gsd, [rcam], [frame], bands=bands)
    with pytest.raises(ValueError, match='bands'):
        ortho.compose_dense(surface, [cam], [frame], mode='feather', bands=3)
    with pytest.raises(ValueError, match='bands'):
        ortho.compose_dense(surface, [cam], [frame], mode='multiband')
    with pytest.raises(ValueError, match='bands'):
        ortho.compose_dense(surface, [cam], [frame], mode='multiband', bands=3)
    with pytest.raises(ValueError):
        ms.compose(dsm, x0, y1, gsd, [rcam], [frame], bands=0)


# ---- 2. a single image is mode best ----
@pytest.mark.parametrize('k', [0, 1, 2])
def test_a_single_image_is_best_within_one_grey_level(k):
    dsm, x0, y1, gsd = roof_dsm()
    cam = roof_cameras((400, 400), focal=150.0)[k]
    frame = oc.hash_frame(k, 400, 400)
    best = rs.compose(dsm, x0, y1, gsd, [cam], [frame], 'best', ss=1, bias=BIAS)
    empty = int((best['count'] == 0).sum())
    assert 0 < empty < 96 * 96 // 8
    for bands in (1, 5, 16):
        got = ms.compose(dsm, x0, y1, gsd, [cam], [frame], bands=bands, ss=1, bias=BIAS)
        assert got['index'].tobytes() == best['index'].tobytes() and got['count'].tobytes() == best['count'].tobytes()
        assert got['bands'] == min(bands, 8)
        worst = int(np.abs(got['bgr'].astype(np.int64) - best['bgr'].astype(np.int64)).max())
        print('camera %d bands %d: %d pixels with count == 0, largest difference to best %d' % (k, bands, empty, worst))
        assert worst <= 1
        assert not got['bgr'][best['count'] == 0].any()


# ---- 3. flat frames stay in range; with a layer of the visible pixels only they do not ----
@pytest.mark.parametrize('ss', [1, 2])
def test_flat_frames_stay_in_range(flat, ss):
    dsm, x0, y1, gsd, cams, frames = flat
    for cam in cams:                                        # the scene's premise
        assert ms.cover(dsm, x0, y1, gsd, ss, cam, (400, 400))[0].all()
    for bands in (1, 3, 5, 8):
        got = ms.compose(dsm, x0, y1, gsd, cams, frames, bands=bands, ss=ss, bias=BIAS)
        on = got['count'] > 0
        lo, hi = int(got['bgr'][on].min()), int(got['bgr'][on].max())
        print('cover rule, ss %d, bands %d: %d .. %d' % (ss, bands, lo, hi))
        assert on.mean() > 0.9 and lo >= min(FLAT) and hi <= max(FLAT)
    seen = ms.compose(dsm, x0, y1, gsd, cams, frames, bands=3, ss=ss, bias=BIAS, visible_only=True)
    on = seen['count'] > 0
    lo, hi = int(seen['bgr'][on].min()), int(seen['bgr'][on].max())
    print('visible pixels only, ss %d, bands 3: %d .. %d' % (ss, lo, hi))
    assert lo < min(FLAT) and hi > max(FLAT)                # the rule, not the scene, carries the property


# ---- 4. the seam ----
def largest_step(bgr, margin=8):
    a = bgr[margin:-margin, margin:-margin].astype(np.int64)
    return int(max(np.abs(np.diff(a, axis=0)).max(), np.abs(np.diff(a, axis=1)).max()))


def test_the_seam_goes(flat_best, flat_five):
    assert len(set(np.unique(flat_best['index'])) - {-1}) == 3
    hard, soft = largest_step(flat_best['bgr']), largest_step(flat_five['bgr'])
    print('largest step between neighbours inside a margin of 8: best %d, 5 bands %d' % (hard, soft))
    assert hard == 100
    assert soft <= 10


# ---- 5. a view that never wins ----
def test_a_view_that_never_wins_changes_nothing(flat, flat_five):
    dsm, x0, y1, gsd, cams, frames = flat
    K, dist, _R, _C = cams[0]
    C = np.array([150.0, 180.0, -120.0])                    # far off to the north-east, looking at the roof
    z = -C / np.linalg.norm(C)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    far = (K, dist, np.array([x, np.cross(z, x), z]), C)
    frame = np.full((400, 400, 3), 30, np.uint8)
    got = ms.compose(dsm, x0, y1, gsd, cams + [far], frames + [frame], bands=5, ss=1, bias=BIAS)
    assert ms.cover(dsm, x0, y1, gsd, 1, far, (400, 400))[0].sum() > 1000 and not (got['index'] == 3).any()
    assert (got['count'] > flat_five['count']).any()        # it is seen, and counted
    assert got['bgr'].tobytes() == flat_five['bgr'].tobytes() and got['index'].tobytes() == flat_five['index'].tobytes()
    for l in range(got['bands']):
        assert dc.bits(got['N'][l]).tobytes() == dc.bits(flat_five['N'][l]).tobytes(), l
        assert dc.bits(got['D'][l]).tobytes() == dc.bits(flat_five['D'][l]).tobytes(), l


# ---- 6. holes ----
def test_holes_stay_empty_and_nothing_is_nan(flat):
    dsm, x0, y1, gsd, cams, _flat = flat
    dsm = dsm.copy()
    dsm[40:47, 10:19] = np.nan
    dsm[5, 90] = np.nan
    dsm[60:63, 50:52] = np.nan                              # on the roof
    frames = [oc.hash_frame(k, 400, 400) for k in range(3)]
    got = ms.compose(dsm, x0, y1, gsd, cams, frames, bands=5, ss=1, bias=BIAS)
    holes = np.isnan(dsm)
    assert (got['count'][holes] == 0).all() and not got['bgr'][holes].any() and (got['index'][holes] == -1).all()
    assert (got['count'][~holes] > 0).mean() > 0.9
    for l in range(got['bands']):
        assert np.isfinite(got['N'][l]).all() and np.isfinite(got['D'][l]).all()
    up = ms.compose(dsm, x0, y1, gsd, cams, frames, bands=3, ss=2, bias=BIAS)
    inside = np.zeros((192, 192), bool)
    inside[82:92, 22:36] = True                             # pixels whose four taps are all holes
    assert (up['count'][inside] == 0).all() and not up['bgr'][inside].any()


# ---- 7. files ----
def test_save_writes_mode_bands_and_the_surface_keys(tmp_path):
    _reference_node()
    bgr = oc.hash_frame(3, 20, 30).copy()
    info = ortho.save(_HostMosaic(bgr, mode='multiband', bands=4, surface='dense', upsample=2, bias=0.5), str(tmp_path),
                      tile=16, fmt='png', subdir='true_ortho')
    assert (info['mode'], info['bands'], info['surface'], info['upsample'], info['bias']) == ('multiband', 4, 'dense', 2, 0.5)
    assert json.loads((tmp_path / 'true_ortho' / 'ortho.json').read_text()) == info
    m = ortho.Mosaic(bgr=_HostMosaic(bgr).bgr, index=None, count=None, x0=-12.5, y1=40.0, gsd=0.25, mode='multiband',
                     names=['a.JPG'], bands=4, surface='dense', upsample=2, bias=0.5)
    assert ortho.save(m, str(tmp_path / 'again'), tile=16, fmt='png', subdir='true_ortho') == info
