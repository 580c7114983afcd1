"""Shared by the SIFT tests (test_sift_gpu.py, test_sift_edges_gpu.py, test_sift_oracle_params.py):
the test texture, the row-by-row comparison with the oracle and the read-back of a device pyramid
level."""
import numpy as np


def texture(h, w, seed=0):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.float64)
    for s in (2, 4, 8, 16, 32):
        g = rng.normal(size=(h // s + 2, w // s + 2))
        img += np.kron(g, np.ones((s, s)))[:h, :w] * s ** 0.7
    k = np.array([1, 4, 6, 4, 1.]) / 16
    img = np.apply_along_axis(lambda r: np.convolve(r, k, 'same'), 1, img)
    img = np.apply_along_axis(lambda r: np.convolve(r, k, 'same'), 0, img)
    img = (img - img.min()) / (img.max() - img.min()) * 255
    return np.stack([img, img * 0.9 + 10, img * 0.8 + 20], 2).clip(0, 255).astype(np.uint8)


def rows_equal(kps, des, kp, octv, d):
    """oracle (float64 array of float32 values) vs device rows, in the same order: -> (rows whose
    five float32 fields are not bit-equal, descriptor bytes that differ, largest difference)"""
    assert len(kp) == len(kps), (len(kp), len(kps))
    assert np.array_equal(kps[:, 5].astype(np.int64), octv.astype(np.int64))
    same = kps[:, :5].astype(np.float32).view(np.int32) == np.ascontiguousarray(kp).view(np.int32)
    diff = np.abs(des.astype(int) - d.astype(int))
    return int((~same.all(1)).sum()), int((diff != 0).sum()), int(diff.max()) if diff.size else 0


def device_level(img_shape, ws, octave, kind, index):
    import ctypes
    from imageanalysis_amd import _lib
    off, lh, lw, no = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().iamx_sift_pyramid_level(img_shape[0], img_shape[1], octave, kind, index,
                                                  ctypes.byref(off), ctypes.byref(lh), ctypes.byref(lw),
                                                  ctypes.byref(no)), 'iamx_sift_pyramid_level')
    n = lh.value * lw.value
    lvl = ws[off.value:off.value + 4 * n].view(dtype=__import__('torch').float32)
    return lvl.cpu().numpy().reshape(lh.value, lw.value), no.value
