"""GPU: the SIFT kernels (csrc/sift.hip) at their structural edges, against the CPU oracle
(oracle/sift_oracle.py, parametrised: sigma, contrast_threshold, edge_threshold, max_radius).

The bars are those of test_sift_gpu.py: the same rows in OpenCV's order, zero rows whose five
float32 fields are not bit-equal, at most one descriptor byte off by at most 1, last_removed equal
to the oracle's; pyramids compared with np.array_equal on every stored level of every octave.
Every case first asserts on the host that it is the case it claims to be (octave count, tail
membership by the admission test of iamx_sift_detect restated below, window side, ...).

The dense-tile path of the extrema scan (more than EXT_LIST = 512 candidates in one 62 x 64 tile,
which then go straight to the global list) is case 9, test_dense_tile_overflows_the_workgroup_list.
Inputs tried on the CPU (per-tile counts over the three layers of one octave; checkerboards of
1-4 pixel cells, dot lattices of period 2-5, single-pixel stripes, uniform and binary noise, at
90 x 90 and 128 x 128, sigma 0.8 / 1.05 / 1.2 / 1.6, contrast 0.04 / 0.02 / 0.001): at the default
contrast threshold and sigma 1.6 the scan threshold is 1 grey level and the densest tile holds 128
(dots of period 4; 3-pixel checkerboard 121; at sigma 0.8 dots of period 3 reach 814); from
contrast_threshold 0.0235 down the scan threshold is floor(...) = 0, and the 1-pixel checkerboard
-- which octave 1 samples into a constant, so that its DoG levels are plateaus of rounding residue
where `>=` every neighbour holds everywhere -- puts 7553 candidates into one tile of octave 1
(stripes 3136, dots of period 2: 3059 at sigma 1.2)."""
import functools
import math

import numpy as np
import pytest

from sift_common import texture, rows_equal, device_level

pytestmark = pytest.mark.gpu

# ---- csrc/sift.hip's constants and host arithmetic, restated -------------------------------------
BORDER = 5
TAIL_PIXELS = 12800
TAIL_NEXT = TAIL_PIXELS // 4 + 128           # floats of the tail kernel's staging array: 3328
SIDE_OCTAVE = 4
DESC_ROWS = 160
EXT_LIST = 512
CAP_CAND = 1 << 21


def layout(h, w):
    """make_layout: the (height, width) of every octave of an h x w image"""
    H, W = 2 * h, 2 * w
    n_oct = max(int(round(math.log(min(H, W)) / math.log(2.0) - 2)) + 1, 1)
    dims = []
    for _o in range(n_oct):
        dims.append((H, W))
        H, W = H // 2, W // 2
        if H < 1 or W < 1:
            break
    return dims


def tail_start(dims, staged_base_counts):
    """first octave of the one-workgroup tail (len(dims): no tail).  An octave is admitted when its
    level fits the kernel's arrays at the odd pitch w | 1 and -- staged_base_counts, the fix; the
    predicate before it had only the first clause -- the base it stages for its successor,
    (h / 2) rows at pitch (w / 2) | 1, fits the TAIL_NEXT floats of the staging array."""
    n = len(dims)
    o_side = min(n, SIDE_OCTAVE)
    o_tail = n
    for o in range(n - 1, max(o_side, 1) - 1, -1):
        h, w = dims[o]
        ok = h * (w | 1) <= TAIL_PIXELS
        if ok and staged_base_counts and o + 1 < n:
            ok = (h // 2) * ((w // 2) | 1) <= TAIL_NEXT
        if not ok:
            break
        o_tail = o
    return o_tail


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _workspace():
    import torch
    from imageanalysis_amd import kernels
    return kernels._sift_ws[(torch.cuda.current_device(), 0)]


def _check_pyramid(shape, gauss):
    """every stored level of every octave of the detection that just ran == the oracle's"""
    ws = _workspace()
    _lvl, n_oct = device_level(shape, ws, 0, 0, 0)
    assert n_oct == len(gauss) == len(layout(*shape))
    for o in range(n_oct):
        for i in range(6):
            got, _ = device_level(shape, ws, o, 0, i)
            assert got.shape == gauss[o][i].shape and np.array_equal(got, gauss[o][i]), ('gauss', o, i)


def _check_rows(kps, des, removed, got, bar=(0, 1, 1)):
    from imageanalysis_amd import kernels
    from oracle import sift_oracle as so
    kp, octv, d = got
    assert kp.dtype == np.float32 and octv.dtype == np.int32 and d.dtype == np.uint8
    assert kp.shape == (len(kps), 5) and octv.shape == (len(kps),) and d.shape == (len(kps), 128)
    assert kernels.sift_detect.last_removed == removed
    bad_rows, bad_bytes, worst = rows_equal(kps, des, kp, octv, d)
    assert bad_rows <= bar[0] and bad_bytes <= bar[1] and worst <= bar[2], (bad_rows, bad_bytes, worst)
    order = np.lexsort(so.opencv_sort_keys(np.concatenate([kp.astype(np.float64), octv[:, None]], 1)))
    assert np.array_equal(order, np.arange(len(kp)))


def _detect_equals_oracle(img, pyramid=True, **par):
    """one detection with `par` against the oracle with the same parameters and the device's tap
    budget (33 taps: max_radius=16) -> the oracle's rows"""
    from imageanalysis_amd import kernels
    from oracle import sift_oracle as so
    opar = dict(par, max_radius=16)
    kps, des, removed = so.detect_and_compute(img, return_removed=True, **opar)
    got = kernels.sift_detect(img, **par)
    if pyramid:
        gauss, _dog = so.build_pyramids(img, sigma=opar.get('sigma', so.SIGMA), max_radius=16)
        _check_pyramid(img.shape[:2], gauss)
    _check_rows(kps, des, removed, got)
    return kps, des, removed


# ---- 1. the staging bound of the one-workgroup tail ------------------------------------------------
def test_tail_staging_bound_tall_narrow():
    """6000 x 128: octave 4 is 750 x 16, 12750 floats at pitch 17 -- inside TAIL_PIXELS -- but the
    base it would stage for octave 5, 375 rows at pitch 9 = 3375 floats, is 47 more than the 3328
    of the staging array: the admission test before the fix took it into the tail (an LDS overrun
    that corrupts levels silently), the test now builds it with the strip kernels and the tail
    starts at octave 5."""
    dims = layout(6000, 128)
    assert len(dims) == 7 and dims[4] == (750, 16) and dims[5] == (375, 8)
    assert tail_start(dims, staged_base_counts=False) == 4            # before the fix: a tail octave ...
    assert (dims[4][0] // 2) * ((dims[4][1] // 2) | 1) == 3375 > TAIL_NEXT == 3328     # ... that overran
    assert tail_start(dims, staged_base_counts=True) == 5
    img = texture(6000, 128, 7)
    kps, _des, removed = _detect_equals_oracle(img)
    assert len(kps) == 2602 and removed == 1


def test_tail_staging_bound_control_transposed():
    """128 x 6000: the same pixels the other way round never overran (octave 4 is 16 x 750 and
    stages 8 x 375 = 3000 floats): tail from octave 4 before and after"""
    dims = layout(128, 6000)
    assert len(dims) == 7 and dims[4] == (16, 750)
    assert tail_start(dims, False) == tail_start(dims, True) == 4
    assert (dims[4][0] // 2) * ((dims[4][1] // 2) | 1) == 3000 <= TAIL_NEXT
    img = np.ascontiguousarray(texture(6000, 128, 7).transpose(1, 0, 2))
    kps, _des, _removed = _detect_equals_oracle(img)
    assert len(kps) > 1000


# ---- 2. octave counts, tile remainders, images without keypoints -----------------------------------
#   shape, image, octaves, first tail octave (== octaves: no tail), oracle keypoints
#   (noise1 / noise0: uniform noise of seed 1 / 0 -- seed 1 leaves the oracle without a keypoint
#   at every size here, seed 0 gives it 3 at 23 x 40)
_SMALL = [
    ((2, 2), 'noise1', 1, 1, 0), ((2, 3), 'noise1', 1, 1, 0), ((5, 7), 'noise1', 2, 2, 0),
    ((8, 8), 'noise1', 3, 3, 0), ((12, 12), 'noise1', 4, 4, 0),
    ((22, 40), 'noise1', 4, 4, 0),            # 4 octaves: no side stream, no tail
    ((22, 40), 'noise0', 4, 4, 2),
    ((23, 40), 'noise0', 5, 4, 3),            # 5 octaves: the first tail octave
    ((23, 40), 'texture', 5, 4, 9),
    ((33, 65), 'texture', 5, 4, 18),          # 2w = 2 * 64 + 2 columns, 2h = 2 * 32 + 2 rows (blur strips)
    ((70, 99), 'texture', 6, 4, 37),          # extrema scan of octave 0: 2 columns / 2 rows in the last tile
    ((64, 64), 'flat128', 6, 4, 0), ((64, 64), 'flat255', 6, 4, 0),
]


@pytest.mark.parametrize('shape,kind,n_oct,o_tail,n_kp', _SMALL,
                         ids=['%dx%d-%s' % (s[0], s[1], k) for s, k, _a, _b, _c in _SMALL])
def test_octave_count_and_tile_edges(shape, kind, n_oct, o_tail, n_kp):
    from imageanalysis_amd import kernels
    from oracle import sift_oracle as so
    h, w = shape
    dims = layout(h, w)
    assert len(dims) == n_oct and tail_start(dims, True) == tail_start(dims, False) == o_tail
    if shape == (33, 65):
        assert 2 * w == 2 * 64 + 2 and 2 * h == 2 * 32 + 2
    if shape == (70, 99):
        assert (2 * w - 2 * BORDER) % 62 == 2 and (2 * h - 2 * BORDER) % 64 == 2
    img = {'noise1': lambda: _noise(h, w, 1), 'noise0': lambda: _noise(h, w, 0), 'texture': lambda: texture(h, w, 7),
           'flat128': lambda: np.full((h, w), 128, np.uint8),
           'flat255': lambda: np.full((h, w), 255, np.uint8)}[kind]()
    if all(dh <= 2 * BORDER or dw <= 2 * BORDER for dh, dw in dims):
        assert n_kp == 0                      # no octave has an interior to scan
    kps, des, removed = _detect_equals_oracle(img)
    assert len(kps) == n_kp
    if n_kp == 0:
        kp, octv, d = kernels.sift_detect(img)
        assert kp.shape == (0, 5) and octv.shape == (0,) and d.shape == (0, 128)
        assert kernels.sift_detect.last_removed == 0 and removed == 0
        ck, co, cd = kernels.sift_detect(img, order='canonical')
        assert ck.shape == (0, 5) and co.shape == (0,) and cd.shape == (0, 128)
    assert so.detect_and_compute(img)[0].tobytes() == kps.tobytes()      # (max_radius=16 is no cap at sigma 1.6)


# ---- 3. capacity -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_200x260():
    from oracle import sift_oracle as so
    img = texture(200, 260, 0)
    kps, des, removed = so.detect_and_compute(img, return_removed=True)
    raw, _gauss = so.detect(img)              # the rows before duplicate removal, in scan order
    assert len(raw) == len(kps) + removed
    return img, kps, des, removed, raw


def test_capacity_exact_and_exceeded():
    from imageanalysis_amd import _lib, kernels
    img, kps, des, removed, _raw = _reference_200x260()
    n_raw = len(kps) + removed                # rows before duplicate removal
    assert n_raw > 200
    _check_rows(kps, des, removed, kernels.sift_detect(img, cap=n_raw))
    for cap in (n_raw - 1, 64):
        with pytest.raises(_lib.IamxError):
            kernels.sift_detect(img, cap=cap)
    _check_rows(kps, des, removed, kernels.sift_detect(img))              # nothing was damaged


def test_capacity_clamps_inside_poisoned_buffers():
    """iamx_sift_detect + iamx_sift_sort with cap = 64 on an image with hundreds of keypoints: the
    count is reported in full, at most 64 rows are stored and sorted, and nothing beyond row 64 of
    any of the four buffers is written"""
    import torch
    from imageanalysis_amd import _lib, kernels
    from imageanalysis_amd.kernels import _ptr
    img, kps, _des, removed, raw = _reference_200x260()
    cap, rows = 64, 64 + 200
    dev = kernels.require_gpu()
    d_img = kernels._dev(img, torch.uint8)    # (contiguous: texture()'s array is not)
    L = _lib.lib()
    need = int(L.iamx_sift_workspace_bytes(img.shape[0], img.shape[1]))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    need_s = int(L.iamx_sift_sort_workspace_bytes(cap))
    sw = torch.empty(need_s, dtype=torch.uint8, device=dev)
    POISON = -12345.0
    kp = torch.full((rows, 8), POISON, dtype=torch.float32, device=dev)
    out_kp = torch.full((rows, 8), POISON, dtype=torch.float32, device=dev)
    desc = torch.full((rows, 128), 0xA5, dtype=torch.uint8, device=dev)
    out_desc = torch.full((rows, 128), 0xA5, dtype=torch.uint8, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    n_sorted = torch.full((1,), -1, dtype=torch.int32, device=dev)
    _lib.check(L.iamx_sift_detect(_ptr(d_img), img.shape[0], img.shape[1], 3, 0.04, 10.0, 1.6, _ptr(ws), need,
                                  _ptr(kp), _ptr(desc), cap, _ptr(n), kernels.stream_ptr()), 'iamx_sift_detect')
    _lib.check(L.iamx_sift_sort(_ptr(kp), _ptr(desc), _ptr(n), cap, 1, img.shape[1], img.shape[0], _ptr(sw), need_s,
                                _ptr(out_kp), _ptr(out_desc), _ptr(n_sorted), kernels.stream_ptr()), 'iamx_sift_sort')
    torch.cuda.synchronize()
    assert int(n.item()) == len(kps) + removed                             # the true count
    assert 0 < int(n_sorted.item()) <= cap
    for buf, poison in ((kp, POISON), (out_kp, POISON), (desc, 0xA5), (out_desc, 0xA5)):
        assert bool((buf[cap:] == poison).all()), 'a row beyond the capacity was written'
    # the 64 stored rows are 64 of the detection's rows; the sorted ones are among them, in order
    stored = np.ascontiguousarray(kp[:cap, :6].cpu().numpy()).view(np.int32)
    every = np.concatenate([raw[:, :5].astype(np.float32).view(np.int32), raw[:, 5:6].astype(np.int32)], 1)
    known = {r.tobytes() for r in every}
    assert all(r.tobytes() in known for r in stored)
    srt = np.ascontiguousarray(out_kp[:int(n_sorted.item()), :6].cpu().numpy())
    assert all(r.tobytes() in {q.tobytes() for q in stored} for r in srt.view(np.int32))
    assert np.all(np.diff(srt[:, 0]) >= 0)


# ---- 4. the unsorted descriptor pass ---------------------------------------------------------------
def test_unsorted_descriptor_pass():
    """cap = 1 700 000 > CAP_CAND * sizeof(Cand) / 20 = 1 677 721: the bucket tables of the ordered
    descriptor pass no longer fit the candidate list's memory, descriptor_kernel walks the list as
    appended (no permutation, cos / sin taken in the kernel, one slab)"""
    import torch
    from imageanalysis_amd import kernels
    img, kps, des, removed, _raw = _reference_200x260()
    cap = 1700000
    assert cap * 20 > CAP_CAND * 16 >= (cap - 30000) * 20
    dflt = kernels.sift_detect(img)
    _check_rows(kps, des, removed, dflt)
    key = (torch.cuda.current_device(), 0)
    try:
        big = kernels.sift_detect(img, cap=cap)
        _check_rows(kps, des, removed, big)
        assert all(np.array_equal(a, b) for a, b in zip(dflt, big))
    finally:
        # ~0.6 GB of capacity-sized buffers: back to the allocator
        for cache in (kernels._sift_out, kernels._sift_sort_ws, kernels._sift_pin):
            cache.pop(key, None)
        kernels._sift_pin.pop((key, 'n'), None)
        torch.cuda.empty_cache()
    _check_rows(kps, des, removed, kernels.sift_detect(img))


# ---- 5. parameters ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _default_167x301():
    from oracle import sift_oracle as so
    img = texture(167, 301, 3)
    return img, so.detect_and_compute(img)[0]


@pytest.mark.parametrize('contrast,edge,sigma', [(0.02, 10, 1.6), (0.08, 10, 1.6), (0.04, 5, 1.6),
                                                 (0.04, 20, 1.6), (0.04, 10, 1.2), (0.04, 10, 2.0)])
def test_parameters(contrast, edge, sigma):
    from oracle import sift_oracle as so
    img, k_default = _default_167x301()
    assert so.layer_sigmas(sigma)[-1] * 8 + 1 < 33.5          # no kernel is truncated at these sigmas
    kps, _des, _removed = _detect_equals_oracle(img, pyramid=sigma != 1.6, contrast_threshold=float(contrast),
                                                edge_threshold=float(edge), sigma=float(sigma))
    assert len(kps) > 20
    a = {r.tobytes() for r in kps[:, :4]}
    b = {r.tobytes() for r in k_default[:, :4]}
    if contrast < 0.04 or edge > 10:
        assert a > b                                          # a proper superset of the default's
    elif contrast > 0.04 or edge < 10:
        assert a < b
    else:
        assert a != b and len(a & b) < len(b) // 2            # another pyramid: other keypoints


# ---- 6. tap truncation -----------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [3.0, 3.5])
def test_tap_truncation_is_what_the_device_computes(sigma):
    """A kernel keeps at most 33 taps (radius 16, renormalised): exact OpenCV Gaussians only while
    round(8 sigma_i + 1) | 1 <= 33 for every layer, i.e. sigma <= 2.10.  Beyond, the levels equal
    the oracle's TRUNCATED pyramid and differ from the whole-kernel one (include/iamx.h, DESIGN.md
    section 2)."""
    from imageanalysis_amd import kernels
    from oracle import sift_oracle as so
    sig = so.layer_sigmas(sigma)
    assert max((int(round(s * 8 + 1)) | 1) // 2 for s in sig[1:]) > 16
    img = texture(90, 120, 5)
    kernels.sift_detect(img, sigma=sigma)
    cut, _ = so.build_pyramids(img, sigma=sigma, max_radius=16)
    _check_pyramid(img.shape[:2], cut)
    whole, _ = so.build_pyramids(img, sigma=sigma)
    ws = _workspace()
    differ = [(o, i) for o in range(len(whole)) for i in range(1, 6)
              if not np.array_equal(device_level(img.shape[:2], ws, o, 0, i)[0], whole[o][i])]
    assert differ, 'the device pyramid equals the untruncated one'
    kps, des, removed = so.detect_and_compute(img, return_removed=True, sigma=sigma, max_radius=16)
    assert len(kps) > 10
    _check_rows(kps, des, removed, kernels.sift_detect(img, sigma=sigma))


# ---- 7. the large descriptor window ----------------------------------------------------------------
def _window_sides(kps, shape):
    """2 * radius + 1 of every keypoint's descriptor window, by the expressions of
    sift_oracle.descriptor() on the arguments of descriptor_params()"""
    from oracle import sift_oracle as so
    F = np.float32
    par, level = so.descriptor_params(kps)
    dims = layout(*shape)
    sides = []
    for k in range(len(kps)):
        h, w = dims[level[k, 0]]
        hist_width = F(F(so.DESCR_SCL_FCTR) * par[k, 3])
        radius = so.cv_round(F(F(F(hist_width * F(1.4142135623730951)) * F(so.DESCR_WIDTH + 1)) * F(0.5)))
        sides.append(2 * min(radius, int(math.sqrt(float(w) * w + float(h) * h))) + 1)
    return np.array(sides)


def test_large_descriptor_window():
    """sigma 3.5: a keypoint of the third layer has a window radius of ~23.8 sigma >= 80, more
    rows than descriptor_kernel's interval walk holds (DESC_ROWS = 160): the plain walk over the
    whole window.  Seed 4 of the 160 x 200 texture has six such keypoints (sides up to 167)."""
    from oracle import sift_oracle as so
    img = texture(160, 200, 4)
    kps, des, removed = so.detect_and_compute(img, return_removed=True, sigma=3.5, max_radius=16)
    sides = _window_sides(kps, img.shape[:2])
    assert int((sides > DESC_ROWS).sum()) == 6 and int(sides.max()) == 167
    assert int((sides <= DESC_ROWS).sum()) >= 50              # and the interval walk beside it
    _detect_equals_oracle(img, pyramid=False, sigma=3.5)


# ---- 9. more than EXT_LIST candidates in one tile of the extrema scan ------------------------------
def _max_candidates_per_tile(dog, contrast):
    """the 26-neighbour test of the oracle's detect(), counted per (octave, 64-row x 62-column tile)"""
    thr = math.floor(0.5 * contrast / 3 * 255)
    best = 0
    for dogs in dog:
        h, w = dogs[0].shape
        if h <= 2 * BORDER or w <= 2 * BORDER:
            continue
        per_tile = {}
        for layer in (1, 2, 3):
            core = dogs[layer][BORDER:h - BORDER, BORDER:w - BORDER]
            is_max = (np.abs(core) > thr) & (core > 0)
            is_min = (np.abs(core) > thr) & (core < 0)
            for dl in (-1, 0, 1):
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        sh = dogs[layer + dl][BORDER + dr:h - BORDER + dr, BORDER + dc:w - BORDER + dc]
                        is_max &= core >= sh
                        is_min &= core <= sh
            rr, cc = np.nonzero(is_max | is_min)
            for t in zip((rr // 64).tolist(), (cc // 62).tolist()):
                per_tile[t] = per_tile.get(t, 0) + 1
        best = max([best] + list(per_tile.values()))
    return best


def test_dense_tile_overflows_the_workgroup_list():
    """a checkerboard of single pixels at contrast_threshold 0.02 (scan threshold 0): octave 1
    samples it into a constant whose DoG levels are plateaus of rounding residue -- thousands of
    candidates in one tile, all but the first EXT_LIST appended to the global list one by one.
    None of those survives the refinement, so columns 40.. carry a texture instead: tile (0, 0)
    of octave 1 (columns 5 .. 66, rows 5 .. 68) then holds ~2000 plateau candidates AND the
    candidates of keypoints, which are lost if the overflow path drops what it is given."""
    from oracle import sift_oracle as so
    y, x = np.mgrid[0:90, 0:90]
    img = np.where((y + x) % 2 == 0, 0, 255).astype(np.uint8)
    img[:, 40:] = texture(90, 90, 1)[:, 40:, 1]
    _gauss, dog = so.build_pyramids(img, max_radius=16)
    assert _max_candidates_per_tile(dog, 0.02) > 3 * EXT_LIST
    assert _max_candidates_per_tile(dog, 0.04) <= EXT_LIST
    kps, _des, _removed = _detect_equals_oracle(img, contrast_threshold=0.02)
    oc = kps[:, 5].astype(np.int64)
    in_tile = ((oc & 255) == 0) & (kps[:, 0] >= 5) & (kps[:, 0] < 67) & (kps[:, 1] >= 5) & (kps[:, 1] < 69)
    assert int(in_tile.sum()) >= 8 and len(kps) > 50
    _detect_equals_oracle(img, pyramid=False)


# ---- 8. iamx_sift_sort alone -----------------------------------------------------------------------
WIDTH, HEIGHT = 640, 480


def _packed(octave, layer, xi_byte):
    """cv2.KeyPoint.octave as iamx_sift_detect stores it (first octave -1 in the low byte)"""
    return (octave & 255) | (layer << 8) | (xi_byte << 16)


def _random_rows(n, rng):
    """n rows distinct in (x, y): x, y, size, angle, response, packed octave (float32 values)"""
    rows = np.zeros((n, 6), np.float64)
    rows[:, 0] = rng.permutation(n) * (WIDTH - 1.0) / max(n, 1) + rng.uniform(0, 0.4, n)
    rows[:, 1] = rng.uniform(0, HEIGHT - 1, n)
    rows[:, 2] = rng.uniform(1.5, 40, n)
    rows[:, 3] = rng.uniform(0, 360, n)
    rows[:, 4] = rng.uniform(0.01, 0.2, n)
    rows[:, :5] = rows[:, :5].astype(np.float32)
    rows[:, 5] = [_packed(int(o), int(l), int(b)) for o, l, b in
                  zip(rng.integers(-1, 6, n), rng.integers(1, 4, n), rng.integers(0, 256, n))]
    return rows


def _with_runs(n, rng, runs, order=1):
    """rows with a run of `length` rows equal in (x, y, size, angle) and the packed octave, with
    distinct responses, at positions start .. start + length - 1 of `order` (1: OpenCV's -- by x,
    which is distinct; 0: pyramid-local -- by octave, layer, then y, which is distinct), for
    (start, length) in runs.  A run overwrites the rows that stood at its positions, so every
    other row keeps its own; test_sort_alone recomputes the positions with the oracle."""
    rows = _random_rows(n, rng)
    if order == 1:
        rows = rows[np.argsort(rows[:, 0], kind='stable')]
    else:
        oc = rows[:, 5].astype(np.int64)
        rows = rows[np.lexsort((rows[:, 1], (oc >> 8) & 255, ((oc & 255) + 1) & 255))]
    for start, length in runs:
        rows[start:start + length, :4] = rows[start, :4]
        rows[start:start + length, 5] = rows[start, 5]
        rows[start:start + length, 4] = np.float32(0.3) - np.arange(length).astype(np.float32) * np.float32(0.01)
    return rows[rng.permutation(n)]


def _run_spans(rows, order):
    """[first, last] sorted position (order 1: OpenCV's, 0: pyramid-local) of every run of rows
    equal in (x, y, size, angle): the first is kept, the others are the bits of dup_bits"""
    from oracle import sift_oracle as so
    perm = np.lexsort(so.opencv_sort_keys(rows)) if order == 1 else so.canonical_order(rows)
    s = rows[perm]
    spans = []
    for p in np.nonzero(np.all(s[1:, :4] == s[:-1, :4], axis=1))[0] + 1:
        if spans and spans[-1][1] == p - 1:
            spans[-1][1] = int(p)
        else:
            spans.append([int(p) - 1, int(p)])
    return spans


SORT_BUCKETS, SORT_SEGS = 4096, 128


def _buckets(rows, order):
    """make_key's bucket of every row, in its float32 arithmetic"""
    F = np.float32
    oc = rows[:, 5].astype(np.int64)
    if order == 1:
        return np.clip((rows[:, 0].astype(F) / F(WIDTH) * F(SORT_BUCKETS)).astype(np.int64), 0, SORT_BUCKETS - 1)
    per = SORT_BUCKETS // SORT_SEGS
    seg = (((((oc & 255) + 1) & 255) << 2) | ((oc >> 8) & 3)) & (SORT_SEGS - 1)
    return seg * per + np.clip((rows[:, 1].astype(F) / F(HEIGHT) * F(per)).astype(np.int64), 0, per - 1)


def _sort_cases():
    rng = np.random.default_rng(11)
    cases = []
    for n in (0, 1, 31, 32, 33, 255, 256, 257, 1000):
        cases.append(('n%d' % n, _random_rows(n, rng), n, max(n, 1)))          # (the ABI wants cap > 0)
        cases.append(('n%d-cap+37' % n, _random_rows(n, rng), n, n + 37))
    # runs of 2, 3 and 7; across a word of dup_bits (32) and across a tile of 256 positions
    cases.append(('runs', _with_runs(1000, rng, [(10, 2), (100, 3), (500, 7)]), 1000, 1000))
    # the same positions in OpenCV's order and, a second set, in the pyramid-local order
    straddle = [(30, 7), (63, 2), (254, 3), (510, 7), (767, 2)]
    cases.append(('runs-straddle', _with_runs(1000, rng, straddle), 1000, 1037))
    cases.append(('runs-straddle-local', _with_runs(1000, rng, straddle, order=0), 1000, 1037))
    one_x = _random_rows(300, rng)
    one_x[:, 0] = np.float32(123.25)                          # order 1: one bucket
    cases.append(('one-x', one_x, 300, 300))
    one_y = _random_rows(300, rng)
    one_y[:, 1] = np.float32(77.5)                            # order 0: one bucket of (octave, layer, y)
    one_y[:, 5] = _packed(2, 2, 128)
    cases.append(('one-octave-layer-y', one_y, 300, 300))
    edge_x = _random_rows(200, rng)
    edge_x[:50, 0] = 0.0                                      # the bucket scale is x / width
    edge_x[50:100, 0] = np.nextafter(np.float32(WIDTH), np.float32(0))
    cases.append(('x-edges', edge_x, 200, 200))
    # rows that differ only in the packed octave: in its sub-layer byte, its layer, its octave
    oc = _random_rows(240, rng)
    for k in range(0, 240, 4):
        oc[k:k + 4, :5] = oc[k, :5]
    oc[0::4, 5] = [_packed(1, 2, 10)] * 60
    oc[1::4, 5] = [_packed(1, 2, 200)] * 60
    oc[2::4, 5] = [_packed(1, 3, 10)] * 60
    oc[3::4, 5] = [_packed(-1, 2, 10)] * 60
    cases.append(('octave-only', oc[rng.permutation(240)], 240, 240))
    cases.append(('n_out>cap', _with_runs(1000, rng, [(100, 3)]), 1000, 600))
    return cases


_SORT_CASES = _sort_cases()


def _sort_reference(rows, order):
    """oracle: removeDuplicatedSorted on the rows (OpenCV's order), for order 0 re-ordered
    pyramid-locally -> (kept rows, their source indices)"""
    from oracle import sift_oracle as so
    kept, idx, _removed = so.remove_duplicated_sorted(rows)
    if order == 0 and len(kept):
        sel = so.canonical_order(kept)
        kept, idx = kept[sel], idx[sel]
    return kept, idx


@pytest.mark.parametrize('order', [1, 0])
@pytest.mark.parametrize('name,rows,n_out,cap', _SORT_CASES, ids=[c[0] for c in _SORT_CASES])
def test_sort_alone(name, rows, n_out, cap, order):
    """iamx_sift_sort on crafted rows; descriptor k is filled with the bytes of its source index,
    so the gather is checked row by row; everything behind the kept rows keeps its poison"""
    import torch
    from imageanalysis_amd import _lib, kernels
    from imageanalysis_amd.kernels import _ptr
    dev = kernels.require_gpu()
    L = _lib.lib()
    stored = min(n_out, cap)
    want, idx = _sort_reference(rows[:stored], order)
    # the case is what its name says, in this order
    spans = _run_spans(rows[:stored], order)
    if name != 'octave-only':
        assert stored - len(want) == sum(b - a for a, b in spans)
    if name == 'runs':
        assert sorted(b - a + 1 for a, b in spans) == [2, 3, 7]
    if (name, order) in (('runs-straddle', 1), ('runs-straddle-local', 0)):
        assert [(a, b - a + 1) for a, b in spans] == [(30, 7), (63, 2), (254, 3), (510, 7), (767, 2)]
        assert sum(a // 32 != b // 32 for a, b in spans) == 5 and sum(a // 256 != b // 256 for a, b in spans) == 3
    if (name, order) in (('one-x', 1), ('one-octave-layer-y', 0)):
        assert len(set(_buckets(rows[:stored], order).tolist())) == 1
    if (name, order) == ('x-edges', 1):
        assert {0, SORT_BUCKETS - 1} <= set(_buckets(rows[:stored], order).tolist())
    if name == 'octave-only':
        # 60 groups of 4: neighbours in OpenCV's order; in the pyramid-local order only the two
        # rows that share octave and layer are, the others lie in other (octave, layer) segments
        assert [b - a + 1 for a, b in spans] == [4 if order == 1 else 2] * 60 and stored - len(want) == 180
    if name == 'n_out>cap':
        assert n_out > cap == stored
    POISON = -54321.0
    rows_alloc = cap + 16
    h_kp = np.full((rows_alloc, 8), POISON, np.float32)
    h_kp[:stored, :5] = rows[:stored, :5]
    h_kp[:stored, 5] = rows[:stored, 5].astype(np.int32).view(np.float32)
    h_kp[:stored, 6:] = 0
    h_desc = np.full((rows_alloc, 128), 0xEE, np.uint8)
    src = np.arange(stored, dtype=np.int32)
    h_desc[:stored] = np.tile(src[:, None], (1, 32)).view(np.uint8)
    kp, desc = torch.from_numpy(h_kp).to(dev), torch.from_numpy(h_desc).to(dev)
    out_kp = torch.full((rows_alloc, 8), POISON, dtype=torch.float32, device=dev)
    out_desc = torch.full((rows_alloc, 128), 0xEE, dtype=torch.uint8, device=dev)
    n = torch.tensor([n_out], dtype=torch.int32, device=dev)
    n_sorted = torch.full((1,), -1, dtype=torch.int32, device=dev)
    need = int(L.iamx_sift_sort_workspace_bytes(cap))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(L.iamx_sift_sort(_ptr(kp), _ptr(desc), _ptr(n), cap, order, WIDTH, HEIGHT, _ptr(ws), need,
                                _ptr(out_kp), _ptr(out_desc), _ptr(n_sorted), kernels.stream_ptr()), 'iamx_sift_sort')
    torch.cuda.synchronize()
    kept = int(n_sorted.item())
    assert kept == len(want) and int(n.item()) == n_out
    g_kp, g_desc = out_kp.cpu().numpy(), out_desc.cpu().numpy()
    assert np.array_equal(g_desc[:kept].view(np.int32)[:, 0], idx.astype(np.int32)), 'another order or survivor'
    assert np.array_equal(g_desc[:kept], h_desc[idx]) and np.array_equal(g_kp[:kept].view(np.int32), h_kp[idx].view(np.int32))
    assert np.all(g_kp[kept:] == POISON) and np.all(g_desc[kept:] == 0xEE)
    assert np.array_equal(kp.cpu().numpy().view(np.int32), h_kp.view(np.int32))          # the input is only read
