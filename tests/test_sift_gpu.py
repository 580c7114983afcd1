"""GPU: the SIFT kernels (csrc/sift.hip) against the CPU restatement of the same published
algorithm (oracle/sift_oracle.py).  PARITY UNPINNED against cv2 (absent); the bar here is
agreement with the oracle, which restates OpenCV's float32 scalar code: the same rows in the same
(OpenCV's) order, fields bit-equal, descriptor bytes equal."""
import numpy as np
import pytest

from sift_common import texture, rows_equal as _rows_equal, device_level as _device_level

pytestmark = pytest.mark.gpu


def _match(ka, oa, kb, ob):
    """greedy one-to-one matching of keypoints with identical packed octave"""
    used = np.zeros(len(kb), bool)
    pairs = []
    for i in range(len(ka)):
        cand = np.nonzero((ob == oa[i]) & ~used & (np.abs(kb[:, 0] - ka[i, 0]) < 0.02)
                          & (np.abs(kb[:, 1] - ka[i, 1]) < 0.02))[0]
        if len(cand) == 0:
            continue
        da = np.abs(((kb[cand, 3] - ka[i, 3]) + 180.0) % 360.0 - 180.0)
        j = cand[np.argmin(da)]
        if da.min() < 0.2:
            used[j] = True
            pairs.append((i, j))
    return np.array(pairs).reshape(-1, 2)


@pytest.mark.parametrize('shape,seed,gray', [((200, 260), 0, False), ((167, 301), 3, False),
                                             ((240, 180), 5, True), ((400, 520), 0, True)])
def test_sift_equals_oracle(shape, seed, gray):
    """row by row in OpenCV's output order: same count, same duplicates removed, every keypoint
    field bit-equal, every descriptor byte equal (the device follows the oracle operation by
    operation; only the order of the float64 histogram atomics is free, ~1e-9 per bin)"""
    from imageanalysis_amd import kernels
    from oracle import sift_oracle as so
    img = texture(shape[0], shape[1], seed)
    if gray:
        img = so.bgr_to_gray(img)
    kps, des, removed = so.detect_and_compute(img, return_removed=True)
    kp, octv, d = kernels.sift_detect(img)
    assert len(kps) > 100 and kernels.sift_detect.last_removed == removed
    bad_rows, bad_bytes, worst = _rows_equal(kps, des, kp, octv, d)
    assert bad_rows == 0 and bad_bytes <= 1 and worst <= 1, (bad_rows, bad_bytes, worst)
    # OpenCV's order: KeyPoint12_LessThan strictly ascending
    order = np.lexsort(so.opencv_sort_keys(np.concatenate([kp.astype(np.float64), octv[:, None]], 1)))
    assert np.array_equal(order, np.arange(len(kp)))
    # descriptor invariants of the format (x512, clip 0.2): u8, L2 norm ~ 512
    nrm = np.sqrt((d.astype(float) ** 2).sum(1))
    assert np.all(np.abs(nrm - 512) < 40)
    # the pyramid-local order of rounds 1-3 is still on offer: same rows, other order
    ck, co, cd = kernels.sift_detect(img, order='canonical')
    sel = so.canonical_order(kps, des)
    assert _rows_equal(kps[sel], des[sel], ck, co, cd) == (0, bad_bytes, worst)


def test_sift_removes_duplicates():
    """KeyPointsFilter::removeDuplicatedSorted: two extrema of a DoG stack can refine to the same
    point and yield identical keypoints; detectAndCompute keeps one.  This texture produces such
    pairs (asserted), the device drops exactly the oracle's, and no two output rows agree in
    (x, y, size, angle)."""
    from imageanalysis_amd import kernels
    from oracle import sift_oracle as so
    gray = so.bgr_to_gray(texture(400, 520, 0))
    raw, _g = so.detect(gray)
    kept, _idx, removed = so.remove_duplicated_sorted(raw)
    assert removed >= 1 and len(kept) == len(raw) - removed
    kp, octv, d = kernels.sift_detect(gray)
    assert kernels.sift_detect.last_removed == removed and len(kp) == len(kept)
    four = np.ascontiguousarray(kp[:, :4]).view(np.int32)
    assert len(np.unique(four, axis=0)) == len(kp)
    # the survivor of a run is the one with the highest response
    assert np.array_equal(kept[:, :5].astype(np.float32).view(np.int32), np.ascontiguousarray(kp).view(np.int32))


def test_sift_translation_repeatability():
    """a crop shifted by whole pixels yields the same features shifted (interior ones)."""
    from imageanalysis_amd import kernels
    big = texture(260, 320, 9)
    a = big[10:250, 10:310]
    b = big[18:258, 26:326]                     # content of b at (x,y) = a at (x+16, y+8)
    ka, oa, da = kernels.sift_detect(a)
    kb, ob, db = kernels.sift_detect(b)
    inner = (ka[:, 0] > 60) & (ka[:, 0] < 240) & (ka[:, 1] > 50) & (ka[:, 1] < 190) & (ka[:, 2] < 8)
    ka2 = ka[inner].astype(np.float64)
    ka2[:, 0] -= 16
    ka2[:, 1] -= 8
    pairs = _match(ka2, oa[inner].astype(np.int64), kb.astype(np.float64), ob.astype(np.int64))
    assert len(pairs) >= 0.85 * inner.sum()
    dd = np.abs(da[inner][pairs[:, 0]].astype(int) - db[pairs[:, 1]].astype(int))
    assert np.median(dd.sum(1)) < 60


@pytest.mark.parametrize('k', [1, 2, 3])
def test_sift_rotation_invariance(k):
    """np.rot90 is an exact pixel permutation: the same scene must give the same keypoints at
    the rotated positions, orientations turned by k*90 degrees and (orientation-normalised)
    descriptors that agree -- what matching between the opposite headings of a lawn-mower
    survey relies on."""
    from imageanalysis_amd import kernels
    img = texture(240, 240, 11)[:, :, 0].copy()
    rot = np.ascontiguousarray(np.rot90(img, k))
    ka, oa, da = kernels.sift_detect(img)
    kb, ob, db = kernels.sift_detect(rot)
    assert len(ka) > 150 and abs(len(ka) - len(kb)) <= len(ka) // 10
    n = img.shape[0]
    # pixel (x, y) of img lands at rot90^k: k=1 -> (y, n-1-x), k=2 -> (n-1-x, n-1-y), k=3 -> (n-1-y, x)
    x, y = ka[:, 0].astype(np.float64), ka[:, 1].astype(np.float64)
    xr, yr = {1: (y, n - 1 - x), 2: (n - 1 - x, n - 1 - y), 3: (n - 1 - y, x)}[k]
    matched, dist, dang = 0, [], []
    for i in range(len(ka)):
        d2 = (kb[:, 0] - xr[i]) ** 2 + (kb[:, 1] - yr[i]) ** 2
        # (cv2 convention: no half-pixel shift for octave -1 => up to 0.5 px between the frames;
        #  the packed octave also carries the sub-layer offset in its top bits: compare octave+layer)
        cand = np.nonzero((d2 < 2.0) & ((ob & 0xFFFF) == (oa[i] & 0xFFFF)))[0]
        if len(cand) == 0:
            continue
        # image rotated counter-clockwise by k*90 deg; keypoint angles are clockwise (y down)
        want = (ka[i, 3] - 90.0 * k) % 360.0
        da_ = np.abs(((kb[cand, 3] - want) + 180.0) % 360.0 - 180.0)
        j = cand[np.argmin(da_)]
        if da_.min() < 3.0:
            matched += 1
            dang.append(da_.min())
            dist.append(np.sqrt(((da[i].astype(float) - db[j].astype(float)) ** 2).sum()))
    print('rot90 x%d: %d / %d keypoints re-found, median angle error %.3f deg, descriptor distance '
          'median %.1f p90 %.1f' % (k, matched, len(ka), np.median(dang), np.median(dist),
                                  np.percentile(dist, 90)))
    assert matched >= 0.8 * len(ka), (matched, len(ka))
    # |desc| = 512, unrelated descriptors are ~500 apart; the half-pixel frame shift costs a little
    assert np.median(dist) < 80 and np.percentile(dist, 90) < 200
    # and they are each other's nearest neighbours among all descriptors
    from oracle import cpu_ref
    idx, dd = cpu_ref.knn2_l2_u8(da, db)
    ratio_ok = (np.sqrt(dd[:, 0].astype(float)) < 0.6 * np.sqrt(dd[:, 1].astype(float))).mean()
    assert ratio_ok > 0.6


def _lib_error():
    from imageanalysis_amd import _lib
    return _lib.IamxError


def test_config_size_pyramid_bit_equal_and_whole_frame():
    """BASELINE configs[1] detect size (5472x3648 at scale 0.4 -> 2189x1459): every Gaussian and
    DoG level of every octave is BIT-identical to the oracle's float32 pyramid, and the WHOLE
    frame's keypoints and descriptors (the oracle's per-keypoint loops run in C,
    oracle/sift_ref.c) agree row by row in OpenCV's output order: same duplicates removed (>= 1 on
    this frame), every field bit-equal, descriptor bytes equal; also on four crops."""
    from imageanalysis_amd import kernels
    from oracle import sift_oracle as so
    frame = texture(1459, 2189, 21)
    gray = so.bgr_to_gray(frame)
    kp, octv, d = kernels.sift_detect(gray)
    dropped = kernels.sift_detect.last_removed
    assert len(kp) > 5000
    import torch
    ws = kernels._sift_ws[(torch.cuda.current_device(), 0)]
    gauss, dog = so.build_pyramids(gray)
    _lvl, n_oct = _device_level(gray.shape, ws, 0, 0, 0)
    assert n_oct == len(gauss) >= 10
    for o in range(n_oct):
        levels = []
        for i in range(6):
            got, _ = _device_level(gray.shape, ws, o, 0, i)
            assert got.shape == gauss[o][i].shape and np.array_equal(got, gauss[o][i]), ('gauss', o, i)
            levels.append(got)
        # the DoG levels are not stored on the device: the scan and the sub-pixel fit take
        # level i + 1 minus level i (one float32 subtraction) -- the oracle's DoG images
        for i in range(5):
            assert np.array_equal(levels[i + 1] - levels[i], dog[o][i]), ('dog', o, i)
    with pytest.raises(_lib_error()):
        _device_level(gray.shape, ws, 0, 1, 0)
    # keypoints / descriptors of the whole frame, row by row
    kps, des, removed = so.detect_and_compute(gray, return_removed=True)
    assert len(kps) > 5000 and removed >= 1 and dropped == removed
    bad_rows, bad_bytes, worst = _rows_equal(kps, des, kp, octv, d)
    print('whole frame: %d keypoints (%d duplicates removed); rows not bit-equal: %d, descriptor '
          'bytes that differ: %d (max %d)' % (len(kps), removed, bad_rows, bad_bytes, worst))
    assert bad_rows <= len(kps) // 5000 and bad_bytes <= 4 and worst <= 1
    order = np.lexsort(so.opencv_sort_keys(np.concatenate([kp.astype(np.float64), octv[:, None]], 1)))
    assert np.array_equal(order, np.arange(len(kp)))
    # keypoints / descriptors on crops of the frame
    for (y0, x0) in ((0, 0), (500, 900), (1159, 1888), (300, 1500)):
        crop = np.ascontiguousarray(gray[y0:y0 + 300, x0:x0 + 301])
        kps, des, removed = so.detect_and_compute(crop, return_removed=True)
        ck, co, cd = kernels.sift_detect(crop)
        assert len(kps) > 100 and kernels.sift_detect.last_removed == removed
        assert _rows_equal(kps, des, ck, co, cd)[0] == 0 and _rows_equal(kps, des, ck, co, cd)[2] <= 1


def test_base_level_for_two_sigmas():
    """The base level is the blur of the doubled gray image: the oracle's level bit for bit, on a
    colour image too (cvtColor inside the doubling), for the default sigma and for one whose base
    blur has another radius (5 and 12)."""
    import torch
    from imageanalysis_amd import kernels
    from oracle import sift_oracle as so
    frame = texture(150, 211, 5)
    for image in (frame, so.bgr_to_gray(frame)):
        gray = so.bgr_to_gray(frame).astype(np.float32)
        for sigma in (1.6, 3.0):
            kernels.sift_detect(image, sigma=sigma)
            ws = kernels._sift_ws[(torch.cuda.current_device(), 0)]
            got, _ = _device_level(gray.shape, ws, 0, 0, 0)
            want = so.gaussian_blur(so.resize_linear_2x(gray), np.sqrt(sigma * sigma - 1.0))
            assert np.array_equal(got, want), sigma
