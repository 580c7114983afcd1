"""CPU: mode multiband's host logic (imageanalysis_amd/ortho.py) and the properties of its numpy
restatement (tests/ortho_multiband_restatement.py).  The device is held to the restatement in
test_ortho_multiband_gpu.py."""
import ctypes

import numpy as np
import pytest

import ortho_common as oc
import ortho_multiband_common as mc
import ortho_multiband_restatement as mb


@pytest.mark.parametrize('bands', [0, 17, -1])
def test_bands_out_of_range_are_refused_without_a_gpu(bands):
    from imageanalysis_amd import ortho
    with pytest.raises(ValueError, match='bands'):
        ortho.compose(mc.PAIR, mc.uv(1), mc.SEAM_FRAMES, mc.WIDTH, mc.HEIGHT, 1.0, 'multiband', bands=bands)
    with pytest.raises(ValueError, match='bands'):
        ortho.band_levels(10, 10, bands)
    with pytest.raises(ValueError, match='bands'):
        mb.levels(10, 10, bands)
    with pytest.raises(ValueError, match='mode'):
        ortho.compose(mc.PAIR, mc.uv(1), mc.SEAM_FRAMES, mc.WIDTH, mc.HEIGHT, 1.0, 'nearest', bands=5)
    assert sorted(ortho.MODES) == ['best', 'feather', 'multiband'] and ortho.MODES['multiband'] is None
    assert (ortho.MODES['best'], ortho.MODES['feather']) == (0, 1) and 'multiband' in ortho.BYTES_PER_PIXEL


@pytest.mark.parametrize('size, want', [((1, 1), 1), ((1, 9), 5), ((64, 64), 7), ((65, 3), 8)])
def test_levels_used(size, want):
    """L = min(B, 1 + ceil(log2(max(H, W)))): the last level of the full pyramid is 1 x 1"""
    from imageanalysis_amd import ortho
    H, W = size
    full = ortho.band_levels(H, W, 16)
    assert len(full) == want and full == mb.levels(H, W, 16) and full[0] == (H, W) and full[-1] == (1, 1)
    for a, b in zip(full, full[1:]):
        assert b == ((a[0] + 1) // 2, (a[1] + 1) // 2)
    for bands in range(1, 17):
        assert ortho.band_levels(H, W, bands) == full[:bands] == mb.levels(H, W, bands)
    assert len(ortho.band_levels(H, W)) == min(5, want)


def test_level_regions_hold_everything_the_restatement_leaves_non_zero():
    """a one-pixel layer in every corner and inside: where R^l of it is non-zero lies in level_regions()"""
    from imageanalysis_amd import ortho
    for H, W in ((1, 1), (7, 1), (16, 17), (33, 40)):
        sizes = ortho.band_levels(H, W, 16)
        for r0, c0, r1, c1 in ((0, 0, 0, 0), (H - 1, W - 1, H - 1, W - 1), (H // 2, W // 3, H // 2 + 2, W // 3 + 1),
                               (0, 0, H - 1, W - 1)):
            r1, c1 = min(r1, H - 1), min(c1, W - 1)
            regions = ortho.level_regions((c0, r0, c1, r1), sizes)
            x = np.zeros((H, W, 1), np.float32)
            x[r0:r1 + 1, c0:c1 + 1] = 1.0
            for l, (y0, x0, y1, x1) in enumerate(regions):
                assert 0 <= y0 <= y1 < sizes[l][0] and 0 <= x0 <= x1 < sizes[l][1]
                rr, cc = np.nonzero(x[:, :, 0])
                assert (y0, x0, y1, x1) == (rr.min(), cc.min(), rr.max(), cc.max()), (H, W, l)   # tight, too
                x = mb.reduce(x)
    stay, metric, temp = ortho.multiband_bytes(ortho.band_levels(8, 8, 2), [(0, 0, 7, 7), (0, 0, -1, -1)])
    assert (stay, metric, temp) == (16 * (64 + 16) + 9 * 64, 8 * 64, 16 * (64 + 16))


def test_reduce_and_expand_of_constants_and_an_impulse():
    one = np.ones((9, 12, 2), np.float32)
    r = mb.reduce(one)
    assert r.shape == (5, 6, 2) and (r[1:-1, 1:-1] == 1.0).all() and r[0, 0, 0] == np.float32(0.6875) ** 2
    e = mb.expand(r, 9, 12)
    assert e.shape == (9, 12, 2) and (e[4:6, 4:8] == 1.0).all()
    x = np.zeros((5, 5, 1), np.float32)
    x[2, 2] = 256.0
    assert mb.reduce(x)[:, :, 0].tolist() == [[1.0, 6.0, 1.0], [6.0, 36.0, 6.0], [1.0, 6.0, 1.0]]
    assert mb.expand(x, 9, 9)[1:8, 4, 0].tolist() == [0.0, 24.0, 96.0, 144.0, 96.0, 24.0, 0.0]


@pytest.mark.parametrize('bands', [1, 5, 16])
def test_single_image_is_best_within_one_grey_level(bands):
    g = mc.grid(mc.lattice(2, 0.3, 0.2, 90.6, 70.7), 71.0)
    best = mc.restated('single', [g], mc.uv(2), [oc.hash_frame(1)], 1.0, 'best')
    multi = mc.restated('single', [g], mc.uv(2), [oc.hash_frame(1)], 1.0, 'multiband', bands)
    d = np.abs(multi['bgr'].astype(int) - best['bgr'].astype(int))
    assert multi['bands'] == min(bands, 8) and multi['bgr'].shape == (71, 91, 3)
    assert d.max() <= 1, '%d bytes differ, by up to %d' % ((d > 0).sum(), d.max())
    assert multi['index'].tobytes() == best['index'].tobytes() and multi['count'].tobytes() == best['count'].tobytes()


def test_one_band_is_best_within_one_grey_level_on_a_recorded_scene():
    best = mc.golden('step5_mid_default', 'best')
    multi = mc.golden('step5_mid_default', 'multiband', 1)
    d = np.abs(multi['bgr'].astype(int) - best['bgr'].astype(int))
    assert multi['bands'] == 1 and best['count'].max() >= 15
    assert d.max() <= 1, '%d bytes differ, by up to %d' % ((d > 0).sum(), d.max())
    assert multi['index'].tobytes() == best['index'].tobytes() and multi['count'].tobytes() == best['count'].tobytes()


def test_an_image_that_wins_no_pixel_changes_no_byte():
    """a third image inside the other two whose span (a tall z range) gives it the largest metric everywhere"""
    big = mc.grid(mc.lattice(2, 0.0, 0.0, 60.0, 40.0), 40.0)
    other = mc.grid(mc.lattice(2, 30.0, 0.0, 90.0, 40.0), 40.0)
    frames = [oc.hash_frame(k) for k in (1, 2, 3)]
    inner = mc.grid(mc.lattice(2, 20.0, 10.0, 70.0, 30.0), 40.0)
    inner[:, 2] = np.linspace(0.0, 4000.0, len(inner))                  # a tall span: its metric loses everywhere
    without = mb.compose([big, other], mc.uv(2), frames[:2], mc.WIDTH, mc.HEIGHT, 1.0)
    with_it = mb.compose([big, other, inner], mc.uv(2), frames, mc.WIDTH, mc.HEIGHT, 1.0)
    assert not (with_it['index'] == 2).any() and with_it['bgr'].shape == without['bgr'].shape
    assert with_it['bgr'].tobytes() == without['bgr'].tobytes()
    assert with_it['index'].tobytes() == without['index'].tobytes()
    assert (with_it['count'] != without['count']).sum() >= 50 * 20 - 100
    for l in range(with_it['bands']):
        assert with_it['N'][l].tobytes() == without['N'][l].tobytes() and with_it['D'][l].tobytes() == without['D'][l].tobytes()


def test_seam_and_detail_on_the_restatement():
    best = mc.restated('seam', mc.PAIR, mc.uv(1), mc.SEAM_FRAMES, 1.0, 'best')
    multi = mc.restated('seam', mc.PAIR, mc.uv(1), mc.SEAM_FRAMES, 1.0, 'multiband')
    assert multi['bands'] == 5 and multi['bgr'].shape == (60, 100, 3)
    assert (best['index'][:, :mc.SEAM] == 0).all() and (best['index'][:, mc.SEAM:] == 1).all()
    mc.check_seam(best['bgr'], multi['bgr'])
    best = mc.restated('detail', mc.PAIR, mc.uv(1), mc.DETAIL_FRAMES, 1.0, 'best')
    multi = mc.restated('detail', mc.PAIR, mc.uv(1), mc.DETAIL_FRAMES, 1.0, 'multiband')
    feather = mc.restated('detail', mc.PAIR, mc.uv(1), mc.DETAIL_FRAMES, 1.0, 'feather')
    assert set(np.unique(best['bgr']).tolist()) == {60, 180}
    mc.check_detail(best['bgr'], multi['bgr'], feather['bgr'])


def test_save_writes_mode_and_bands(tmp_path):
    import json
    import torch
    from imageanalysis_amd import ortho
    m = ortho.Mosaic(bgr=torch.from_numpy(oc.hash_frame(3, 20, 30).copy()), index=None, count=None, x0=0.0, y1=20.0,
                     gsd=1.0, mode='multiband', names=['a'], bands=4)
    info = ortho.save(m, str(tmp_path), tile=32, fmt='png')
    assert (info['mode'], info['bands']) == ('multiband', 4)
    assert json.loads((tmp_path / 'ortho' / 'ortho.json').read_text()) == info
    m = ortho.Mosaic(bgr=m.bgr, index=None, count=None, x0=0.0, y1=20.0, gsd=1.0, mode='best', names=['a'])
    assert m.bands is None and 'bands' not in ortho.save(m, str(tmp_path), tile=32, fmt='png')


def test_argument_checks_do_not_need_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(8)      # never dereferenced: the checks come before the launch
    par = (ctypes.c_double * 8)(5472, 3648, 0.0, 10.0, 0.5, 1.0, 2.0, 3.0)
    bad = (ctypes.c_double * 8)(5472, 3648, 0.0, 10.0, 0.0, 1.0, 2.0, 3.0)
    err = L.iamx_last_error

    def owner(S=8, X=one, params=par, box=(0, 0, 3, 3), H=4, W=4, metric=one):
        return L.iamx_ortho_mb_owner(S, X, one, one, params, 0, *box, H, W, metric, one, one, None)
    assert owner(X=None) == -1 and b'null pointer' in err() and owner(metric=None) == -1 and owner(params=None) == -1
    assert owner(S=0) == -1 and owner(S=33) == -1 and b'grid steps' in err()
    assert owner(H=0) == -1 and owner(W=(1 << 20) + 1) == -1 and b'sides out of range' in err()
    assert owner(box=(0, 0, 4, 3)) == -1 and b'leaves the raster' in err() and owner(box=(0, -1, 3, 3)) == -1
    assert owner(params=bad) == -1 and b'not finite' in err()
    assert owner(box=(2, 0, 1, 3)) == 0                                          # covers nothing: no launch

    def layer(S=8, frame=one, h_s=64, params=par, box=(0, 0, 3, 3), H=4, W=4, index=one, out=one):
        return L.iamx_ortho_mb_layer(S, one, one, one, one, frame, h_s, 96, params, 0, *box, H, W, index, out, None)
    assert layer(frame=None) == -1 and b'null pointer' in err() and layer(index=None) == -1 and layer(out=None) == -1
    assert layer(S=33) == -1 and layer(h_s=0) == -1 and b'empty frame' in err()
    assert layer(H=0) == -1 and layer(box=(0, 0, 3, 4)) == -1 and b'leaves the raster' in err()
    assert layer(out=odd) == -1 and b'aligned' in err()
    assert layer(params=bad) == -1 and layer(box=(0, 3, 3, 2)) == 0

    def reduce(h=8, w=9, src=one, sr=(0, 0, 7, 8), dst=one, dr=(0, 0, 3, 4)):
        return L.iamx_ortho_mb_reduce(h, w, src, *sr, dst, *dr, None)
    assert reduce(src=None) == -1 and reduce(dst=None) == -1 and b'null pointer' in err()
    assert reduce(h=0) == -1 and b'sides out of range' in err()
    assert reduce(src=odd) == -1 and b'aligned' in err()
    assert reduce(sr=(0, 0, 8, 8)) == -1 and b'source region' in err() and reduce(sr=(3, 0, 2, 8)) == -1
    assert reduce(dr=(0, 0, 4, 4)) == -1 and b'destination region' in err() and reduce(dr=(0, -1, 3, 4)) == -1

    def accumulate(h=8, w=9, fine=one, fr=(0, 0, 7, 8), coarse=one, cr=(0, 0, 3, 4), acc=one):
        return L.iamx_ortho_mb_accumulate(h, w, fine, *fr, coarse, *cr, acc, None)
    assert accumulate(fine=None) == -1 and accumulate(acc=None) == -1 and b'null pointer' in err()
    assert accumulate(w=0) == -1 and accumulate(acc=odd) == -1 and b'aligned' in err()
    assert accumulate(fr=(0, 0, 7, 9)) == -1 and b'leaves its level' in err()
    assert accumulate(cr=(0, 0, 3, 5)) == -1 and b'coarser region' in err()

    def collapse(h=8, w=9, acc=one, up=one, count=one, bgr=one):
        return L.iamx_ortho_mb_collapse(h, w, acc, up, count, bgr, None)
    assert collapse(acc=None) == -1 and collapse(count=None) == -1 and b'null pointer' in err()
    assert collapse(h=(1 << 20) + 1) == -1 and collapse(up=odd) == -1 and b'aligned' in err()
    # the old calls have no third mode
    assert L.iamx_ortho_clear(2, 4, 4, one, one, one, one, None) == -1 and b'mode' in err()
