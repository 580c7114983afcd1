"""Host: the SIFT oracle's parameters (oracle/sift_oracle.py, oracle/sift_ref.c) -- sigma,
contrast_threshold, edge_threshold and the tap-radius cap max_radius.  The defaults must remain
what they were, the C path and its numpy twin must agree away from the defaults too, and the two
thresholds must cut in the direction their names say (plumbing checks, not value checks)."""
import numpy as np

from sift_common import texture


def _same(ka, da, kb, db):
    return ka.shape == kb.shape and ka.tobytes() == kb.tobytes() and da.tobytes() == db.tobytes()


def test_defaults_are_unchanged():
    """naming every default explicitly == a call without arguments: same rows, same bytes, the
    same pyramid, through the glue (detect_and_compute) and through the all-C detector"""
    from oracle import sift_oracle as so
    img = texture(200, 260, 0)
    ka, da, ra = so.detect_and_compute(img, return_removed=True)
    kb, db, rb = so.detect_and_compute(img, return_removed=True, sigma=1.6, contrast_threshold=0.04,
                                       edge_threshold=10.0, max_radius=None)
    assert len(ka) > 100 and ra == rb and _same(ka, da, kb, db)
    # no kernel of the default pyramid reaches radius 16: the device's tap cap changes nothing here
    kc, dc = so.detect_and_compute(img, max_radius=16)
    assert _same(ka, da, kc, dc)
    kd, dd = so.detect_and_compute_c(img)
    ke, de = so.detect_and_compute_c(img, sigma=1.6, contrast_threshold=0.04, edge_threshold=10.0)
    assert _same(kd, dd, ke, de) and _same(ka, da, kd, dd)
    ga, _ = so.build_pyramids(img)
    gb, _ = so.build_pyramids(img, sigma=1.6, max_radius=None)
    assert all(np.array_equal(x, y) for la, lb in zip(ga, gb) for x, y in zip(la, lb))
    assert so.layer_sigmas() == so.layer_sigmas(1.6)
    assert np.array_equal(so.gaussian_kernel(1.6), so.gaussian_kernel(1.6, None))


def test_c_path_equals_numpy_twin_off_the_defaults():
    """(sigma 2.0, contrast 0.02, edge 5): the per-keypoint loops in C == their numpy twins == the
    all-C detector, row for row"""
    from oracle import sift_oracle as so
    img = texture(60, 80, 1)
    par = dict(sigma=2.0, contrast_threshold=0.02, edge_threshold=5.0)
    ka, da = so.detect_and_compute(img, use_c=True, **par)
    kb, db = so.detect_and_compute(img, use_c=False, **par)
    kc, dc = so.detect_and_compute_c(img, **par)
    assert len(ka) >= 10
    assert _same(ka, da, kb, db) and _same(ka, da, kc, dc)
    # and they are not the default's rows
    k0, _d0 = so.detect_and_compute(img)
    assert k0.shape != ka.shape or k0.tobytes() != ka.tobytes()


def test_thresholds_cut_the_way_their_names_say():
    from oracle import sift_oracle as so
    img = texture(120, 160, 2)
    n = {c: len(so.detect(img, contrast_threshold=c)[0]) for c in (0.02, 0.04, 0.08)}
    assert n[0.02] > n[0.04] > n[0.08] > 0, n
    m = {e: len(so.detect(img, edge_threshold=e)[0]) for e in (5.0, 10.0, 20.0)}
    assert 0 < m[5.0] < m[10.0] < m[20.0], m
    assert n[0.04] == m[10.0]


def test_max_radius_truncates_and_renormalises():
    from oracle import sift_oracle as so
    full, cut = so.gaussian_kernel(3.0), so.gaussian_kernel(3.0, 8)
    assert len(full) == 25 and len(cut) == 17
    assert abs(float(cut.astype(np.float64).sum()) - 1.0) < 1e-6
    mid = full[4:-4].astype(np.float64)
    assert np.allclose(cut, mid / mid.sum(), rtol=1e-6, atol=0)
    assert np.array_equal(so.gaussian_kernel(3.0, 12), full) and np.array_equal(so.gaussian_kernel(3.0, 40), full)
    img = texture(40, 50, 3)[:, :, 0].astype(np.float32)
    assert np.array_equal(so.gaussian_blur(img, 3.0, 8), so.gaussian_blur_py(img, 3.0, 8))
    assert not np.array_equal(so.gaussian_blur(img, 3.0, 8), so.gaussian_blur(img, 3.0))
