"""CPU: the area-downscale restatement (tests/area_restatement.py) against the exact area average,
the size / scale rule of the texture step, the new C ABI's argument checks, and install()."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import REPO

import area_restatement as ar


def _textured(h, w, ch, seed):
    """random and textured: smooth gradients, a stripe pattern and full-range noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 96 + 80 * np.sin(x / 17.0 + seed) * np.cos(y / 23.0) + 40 * ((x // 5 + y // 7) % 2)
    img = base[:, :, None] + rng.normal(0, 35, (h, w, ch)) + rng.integers(-20, 20, ch)
    img[rng.random((h, w)) < 0.02] = 255                     # saturated specks
    img[rng.random((h, w)) < 0.02] = 0
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img if ch == 3 else img[:, :, 0]


# (width, height, resolution, channels): the texture step's call fx = r / float(w), fy = r / float(h)
CASES = [(684, 456, 64, 3), (1000, 750, 64, 3), (342, 228, 32, 3),
         (684, 456, 64, 1),                                  # one channel
         (512, 384, 64, 3)]                                  # integer ratio: 8 x 6


@pytest.mark.parametrize('w,h,r,ch', CASES)
def test_restatement_against_the_exact_average(w, h, r, ch):
    """No pixel may be more than ONE level from the rounded exact area average.  Derived, not
    measured: the restatement sums about 90 float32 terms whose weights sum to 1, an error near
    1e-3 of a level, so the rounded value can move only where the exact average sits at a half."""
    img = _textured(h, w, ch, seed=w + r)
    fx, fy = r / float(w), r / float(h)
    got = ar.resize_area(img, fx, fy)
    assert got.shape[:2] == (r, r) and got.dtype == np.uint8
    exact = ar.exact_area_average(img, r, r)
    want = np.clip(np.rint(exact), 0, 255)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    err = np.abs(got.astype(np.float64) - exact).max()
    print('%dx%d -> %d (%d ch): %d of %d pixels differ from the rounded exact average, '
          'largest distance to the exact average %.6f levels' % (w, h, r, ch, int((diff > 0).sum()),
                                                                 diff.size, err))
    assert diff.max() <= 1
    assert err <= 0.5 + 1e-2          # what "only at a half" means: within rounding of the exact value


def test_integer_ratio_takes_the_integer_branch():
    img = _textured(96, 128, 3, seed=5)
    got = ar.resize_area(img, 1 / 8.0, 1 / 6.0)
    blocks = img.reshape(16, 6, 16, 8, 3).astype(np.int64).sum(axis=(1, 3))
    want = np.rint(blocks.astype(np.float32) * (np.float32(1.0) / np.float32(48))).astype(np.uint8)
    assert np.array_equal(got, want)
    got2 = ar.resize_area(img, 0.5, 0.5)
    want2 = (img.reshape(48, 2, 64, 2, 3).astype(np.int64).sum(axis=(1, 3)) + 2) >> 2
    assert np.array_equal(got2, want2.astype(np.uint8))


def test_restatement_runs_a_survey_frame_in_seconds():
    import time
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (3648, 5472, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    out = ar.resize_area(img, 512 / float(5472), 512 / float(3648))
    assert out.shape == (512, 512, 3)
    assert time.perf_counter() - t0 < 30.0


@pytest.mark.parametrize('r', [512, 64])
def test_scale_and_size_rule(r):
    """dsize == resolution for a 5472 x 3648 frame, and the scale is 1.0 / (r / float(w))"""
    w, h = 5472, 3648
    fx, fy = r / float(w), r / float(h)
    assert ar.area_dims(h, w, fx, fy) == (r, r)
    from imageanalysis_amd import _lib
    L = _lib.lib()
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    assert L.iamx_image_area_dims(h, w, fx, fy, ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oh.value, ow.value) == (r, r)
    # the taps are built from 1.0 / fx: the last destination pixel ends at the image's last sample
    first, wts, n = ar.area_taps(r, w, 1.0 / fx)
    assert first[0] == 0 and first[-1] + n[-1] == w
    assert abs(float(wts.sum(axis=1).max()) - 1.0) < 1e-5 and abs(float(wts.sum(axis=1).min()) - 1.0) < 1e-5


def test_half_even_size_rounding():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    assert L.iamx_image_area_dims(5, 7, 0.5, 0.5, ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oh.value, ow.value) == (2, 4) == ar.area_dims(5, 7, 0.5, 0.5)      # 2.5 -> 2, 3.5 -> 4


def test_new_symbols_are_declared_and_bound():
    from imageanalysis_amd import _lib
    text = open(os.path.join(REPO, 'include', 'iamx.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('iamx_image_area_dims', 'iamx_image_resize_area'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


def test_argument_errors_do_not_need_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: the checks come before the launch
    rc = L.iamx_image_resize_area(None, 64, 64, 3, 0.5, 0.5, None, None)
    assert rc == -1 and b'null pointer' in L.iamx_last_error()
    rc = L.iamx_image_resize_area(one, 64, 64, 2, 0.5, 0.5, one, None)
    assert rc == -1 and b'channels' in L.iamx_last_error()
    rc = L.iamx_image_resize_area(one, 64, 64, 3, 1.5, 0.5, one, None)
    assert rc == -1 and b'upscaling' in L.iamx_last_error()
    rc = L.iamx_image_resize_area(one, 64, 64, 3, 0.5, 2.0, one, None)
    assert rc == -1 and b'upscaling' in L.iamx_last_error()
    assert L.iamx_image_area_dims(64, 64, 0.5, 0.5, None, None) == -1
    with pytest.raises(ValueError):
        ar.resize_area(np.zeros((8, 8, 3), np.uint8), 1.5, 0.5)


def test_install_replaces_the_reference_function():
    from imageanalysis_amd import panda3d
    ref = types.ModuleType('panda3d')
    ref.make_textures_opencv = lambda *a, **k: 'reference'
    ref.generate_from_grid = lambda *a, **k: 'untouched'
    panda3d.install(ref)
    assert ref.make_textures_opencv is panda3d.make_textures_opencv
    assert ref.generate_from_grid() == 'untouched'
    assert panda3d.TEXTURE_ENTROPY in ('host', 'device')
    assert 1 <= panda3d.TEXTURE_WORKERS <= 16
