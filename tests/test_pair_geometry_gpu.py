"""GPU: the four kernels of csrc/triangulate.hip against the high-precision references of
tests/pair_geometry_reference.py, called through the C ABI at the sizes and edges where they can
go wrong: match counts 0 / 1 / 2 / 255 / 256 / 257, a clip that is no multiple of 256, empty pairs
in m_off, a re-fit schedule that runs out of inliers, degenerate point sets, sky rays, cameras far
from the origin, a 5 cm baseline, and what the kernels leave alone past m_cnt.

Every index handed to a kernel lies inside its arena (_check_indices); unused match rows point at
one in-range keypoint whose coordinates are NaN, outputs are pre-filled with 777.0 and carry a
guard tail.  tests/test_pair_geometry.py shows on the host that the inputs are fair.

Tolerances are never taken from the device (see pair_geometry_reference and DESIGN.md, "pair
geometry accuracy"):
  similarity  |M - M_longdouble| (translations over the largest coordinate)
              <= max(16 x fit_similarity's error on the case, 64 . 2^-52)
  DLT (a)     ||A x|| / ||x|| / sigma4 - 1 <= max(8 x numpy's SVD on the family, 1e-9)
  DLT (b)     |z - z_mpmath| <= max(8 x numpy's SVD on the family, 64 . 2^-52 . sigma3/sigma4 . scale)
  ground      |out - ordered float64 restatement| <= 1e-9 . max(1, |ref|) (not bit-equal: see the test)

Measured on an MI355X (worst per case): see the docstrings of the tests.
"""
import ctypes
import functools

import numpy as np
import pytest

import pair_geometry_reference as ref

pytestmark = pytest.mark.gpu

FILL = ref.POISON_FILL
TAIL = 64


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device='cuda', dtype=dt)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _filled(n, dt=None):
    import torch
    return torch.full((n + TAIL,), FILL, dtype=dt or torch.float64, device='cuda')


def _check_indices(xy, kp_off, pair_img, m_pairs):
    """every keypoint a launch can reach, used row or not, lies inside the arena"""
    for p, (a, b) in enumerate(pair_img):
        for col, im in ((0, a), (1, b)):
            idx = kp_off[im] + m_pairs[p][..., col].astype(np.int64)
            assert idx.size == 0 or (idx.min() >= 0 and idx.max() < len(xy))


def _call(name, *args):
    from imageanalysis_amd._lib import check, lib, stream_ptr
    import torch
    check(getattr(lib(), name)(*args, stream_ptr()), name)
    torch.cuda.synchronize()


def _triangulate_pairs(xy, kp_off, PROJ, pair_img, m_cnt, m_pairs, xyz):
    """iamx_triangulate_pairs / _xyz -> (out [n_pairs, clip(, 3)], guard tail)"""
    import torch
    n_pairs, clip = m_pairs.shape[:2]
    _check_indices(xy, kp_off, pair_img, m_pairs)
    assert np.all(m_cnt <= clip) and len(PROJ) > pair_img.max() and len(kp_off) > pair_img.max()
    w = 3 if xyz else 1
    out = _filled(n_pairs * clip * w)
    keep = [_dev(pair_img, torch.int32), _dev(PROJ, torch.float64), _dev(ref.IK.ravel(), torch.float64),
            _dev(kp_off, torch.int64), _dev(xy, torch.float32), _dev(m_cnt, torch.int32),
            _dev(m_pairs, torch.int32)]
    _call('iamx_triangulate_pairs_xyz' if xyz else 'iamx_triangulate_pairs', *[_ptr(t) for t in keep],
          n_pairs, clip, _ptr(out))
    o = out.cpu().numpy()
    body = o[:n_pairs * clip * w]
    return (body.reshape(n_pairs, clip, 3) if xyz else body.reshape(n_pairs, clip)), o[n_pairs * clip * w:]


def _similarity(xy, kp_off, pair_img, m_cnt, m_pairs):
    """iamx_similarity_pairs -> (aff [n_pairs, 2, 2, 3], ok [n_pairs, 2])"""
    import torch
    n_pairs, clip = m_pairs.shape[:2]
    _check_indices(xy, kp_off, pair_img, m_pairs)
    assert np.all(m_cnt <= clip)
    aff = _filled(n_pairs * 12)
    ok = _filled(n_pairs * 2, torch.int32)
    keep = [_dev(pair_img, torch.int32), _dev(kp_off, torch.int64), _dev(xy, torch.float32),
            _dev(m_cnt, torch.int32), _dev(m_pairs, torch.int32)]
    _call('iamx_similarity_pairs', *[_ptr(t) for t in keep], n_pairs, clip, _ptr(aff), _ptr(ok))
    aff, ok = aff.cpu().numpy(), ok.cpu().numpy()
    assert np.all(aff[n_pairs * 12:] == FILL) and np.all(ok[n_pairs * 2:] == int(FILL))
    return aff[:n_pairs * 12].reshape(n_pairs, 2, 2, 3), ok[:n_pairs * 2].reshape(n_pairs, 2)


def _similarity_single(a, b):
    """one pair alone, the shape smart.find_affine launches: n_pairs = 1, clip = n (clip = 1 and a
    poisoned row where there is no match: the ABI wants clip > 0)"""
    n = len(a)
    xy = np.concatenate([a, b, np.full((1, 2), np.nan, np.float32)])
    kp_off = np.array([0, n, 2 * n], np.int64)
    rows = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32).reshape(1, n, 2)
    if n == 0:
        rows = np.array([[[0, 0]]], np.int32)          # keypoint 0 of each "image" is the poison
    aff, ok = _similarity(xy, kp_off, np.array([[0, 1]], np.int32), np.array([n], np.int32), rows)
    return aff[0], ok[0]


# ---- triangulation: launch geometry ---------------------------------------------------------------
def test_triangulate_launch_geometry():
    """n_pairs = 5, clip = 300 (two x-blocks, the second partial), m_cnt = [0, 1, 256, 257, 300],
    six images of different sizes, non-consecutive slots, (4, 1) and (1, 4), poisoned unused rows.
    Rows past m_cnt and the tail keep their fill, nothing is NaN, every used row agrees with
    numpy's SVD on its own pair's matrices within twice the first-order bound (both sides are
    within it), xyz[..., 2] is the z-only form bit for bit, and a second launch repeats the first.
    Measured: largest |device - SVD| / bound 5.3e-5."""
    c = ref.launch_case()
    ar = c['arena']
    args = (ar.xy, ar.kp_off, c['PROJ'], c['pair_img'], c['m_cnt'], c['m_pairs'])
    assert c['m_pairs'].shape == (5, 300, 2)
    xyz, tail3 = _triangulate_pairs(*args, xyz=True)
    z, tail1 = _triangulate_pairs(*args, xyz=False)
    assert np.all(tail3 == FILL) and np.all(tail1 == FILL)
    assert not np.isnan(xyz).any() and not np.isnan(z).any()
    PR = c['PROJ'].reshape(-1, 3, 4)
    worst = 0.0
    for p, ((a, b), n) in enumerate(zip(c['pair_img'], c['m_cnt'])):
        assert np.all(xyz[p, n:] == FILL) and np.all(z[p, n:] == FILL)
        assert not np.any(xyz[p, :n] == FILL)
        if n == 0:
            continue
        rows = c['m_pairs'][p, :n]
        want, bound, _cond, _w = ref.svd_bounds(PR[a], PR[b], ar.kp[a][rows[:, 0]], ar.kp[b][rows[:, 1]])
        err = np.abs(xyz[p, :n] - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= 2 * bound), (p, float((err / bound).max()))
    print('launch geometry: largest |device - SVD| / bound %.3g' % worst)
    assert np.array_equal(xyz[..., 2], z)
    again, _ = _triangulate_pairs(*args, xyz=True)
    assert np.array_equal(again, xyz)


# ---- triangulation: accuracy against mpmath -------------------------------------------------------
def _family_on_device(name):
    r = ref.family_reference(name)
    n = len(r['uv1'])
    xy = np.concatenate([r['uv1'], r['uv2'], np.full((1, 2), np.nan, np.float32)])
    rows = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32).reshape(1, n, 2)
    m_pairs = np.concatenate([rows, np.array([[[2 * n, n]] * 6], np.int32)], 1)      # clip = n + 6
    xyz, tail = _triangulate_pairs(xy, np.array([0, n, 2 * n], np.int64),
                                   np.stack([r['P1'].ravel(), r['P2'].ravel()]),
                                   np.array([[0, 1]], np.int32), np.array([n], np.int32), m_pairs, xyz=True)
    assert np.all(tail == FILL) and np.all(xyz[0, n:] == FILL) and not np.isnan(xyz).any()
    x = xyz[0, :n]
    ratio_m1 = np.array([float(ref.mp_residual_ratio(r['A'][i], list(x[i]) + [1.0], r['sig4'][i]) - 1)
                         for i in range(n)])
    zerr = np.abs(x[:, 2] - r['xyz_ref'][:, 2])
    zfloor = np.array([ref.z_bound(r['sig3'][i], r['sig4'][i], r['xyz_ref'][i]) for i in range(n)])
    svd_zerr = np.abs(r['svd_xyz'][:, 2] - r['xyz_ref'][:, 2]).max()
    print('%s: device ratio - 1 <= %.3g (numpy SVD %.3g), |z - z_ref| <= %.3g m (numpy SVD %.3g m, '
          'floor >= %.3g m)' % (name, ratio_m1.max(), r['svd_ratio_m1'].max(), zerr.max(), svd_zerr, zfloor.min()))
    return r, ratio_m1, zerr, zfloor, svd_zerr


@pytest.mark.parametrize('name', [n for n, f in ref.FAMILIES.items() if f[3]])
def test_triangulate_accuracy_against_mpmath(name):
    """iamx_triangulate_pairs_xyz on 64 matches of each geometry family against the 60-digit null
    vector: (a) the residual ratio, (b) |z - z_ref|, each within 8 x numpy's SVD or the floor.
    Measured (ratio - 1, |z - z_ref|; numpy's SVD in brackets): nominal 1.5e-17, 5.0e-14 m
    (3.4e-15, 1.4e-12 m); 1e3 m from the origin 3.6e-14, 8.2e-13 m (2.7e-9, 2.1e-10 m); 1e4 m
    3.4e-12, 7.6e-12 m (5.9e-5, 1.6e-8 m); 0.05 m baseline 3.9e-13, 2.7e-11 m (1.2e-9, 6.2e-10 m);
    oblique 3.5e-18, 2.5e-13 m (4.0e-15, 5.3e-12 m) -- the one-sided Jacobi is more accurate than LAPACK's bidiagonalisation on these
    matrices, whose fourth column is |NED| times the others."""
    r, ratio_m1, zerr, zfloor, svd_zerr = _family_on_device(name)
    assert np.all(ratio_m1 > -1e-30)
    assert np.all(ratio_m1 <= max(8 * r['svd_ratio_m1'].max(), 1e-9))
    assert np.all(zerr <= np.maximum(8 * svd_zerr, zfloor))


@pytest.mark.parametrize('name', [n for n, f in ref.FAMILIES.items() if not f[3]])
def test_triangulate_far_origin_figures(name):
    """the same figures 1e5 m and 1e6 m from the origin, printed and not asserted (the product
    works in a local NED frame; DESIGN.md states the supported range).  Measured (ratio - 1,
    |z - z_ref|): 1e5 m 1.3e-10, 5.9e-11 m (numpy's SVD 0.58, 1.3e-6 m); 1e6 m 2.0e-8, 9.9e-10 m
    (77, 9.6e-5 m)."""
    _family_on_device(name)


# ---- triangulation: packed form -------------------------------------------------------------------
@pytest.mark.parametrize('total', ref.PACKED_TOTALS)
def test_triangulate_packed(total):
    """m_off with an empty first pair, two empty pairs in a row and an empty last pair; every pair
    with cameras of its own.  Each match agrees with numpy's SVD on ITS pair's matrices (another
    pair's would miss by metres), equals iamx_triangulate_pairs fed the same matrices as images
    bit for bit, and rows past `total` keep their fill."""
    import torch
    c = ref.packed_case(total)
    ar = c['arena']
    n_pairs = len(c['pair_img'])
    assert c['m_off'][-1] == total == len(c['m_pairs'])
    for p, (a, b) in enumerate(c['pair_img']):
        _check_indices(ar.xy, ar.kp_off, [(a, b)], [c['m_pairs'][c['m_off'][p]:c['m_off'][p + 1]]])
    out = _filled(total)
    keep = [_dev(c['pair_img'], torch.int32), _dev(c['pair_proj'], torch.float64),
            _dev(ref.IK.ravel(), torch.float64), _dev(ar.kp_off, torch.int64), _dev(ar.xy, torch.float32),
            _dev(c['m_off'], torch.int64), _dev(c['m_pairs'], torch.int32)]
    _call('iamx_triangulate_packed', *[_ptr(t) for t in keep], n_pairs, total, _ptr(out))
    o = out.cpu().numpy()
    z, tail = o[:total], o[total:]
    assert np.all(tail == FILL) and not np.isnan(z).any()
    for p, (a, b) in enumerate(c['pair_img']):
        rows = c['rows'][p]
        if not len(rows):
            continue
        P1, P2 = c['pair_proj'][p].reshape(2, 3, 4)
        want, bound, _cond, _w = ref.svd_bounds(P1, P2, ar.kp[a][rows[:, 0]], ar.kp[b][rows[:, 1]])
        got = z[c['m_off'][p]:c['m_off'][p + 1]]
        assert np.all(np.abs(got - want[:, 2]) <= 2 * bound[:, 2]), p
        # the pair before and the pair after would put this pair's first match metres away
        for other in ((p - 1) % n_pairs, (p + 1) % n_pairs):
            O1, O2 = c['pair_proj'][other].reshape(2, 3, 4)
            wrong = ref.dlt_svd_xyz(O1, O2, ar.kp[a][rows[:1, 0]], ar.kp[b][rows[:1, 1]])
            assert abs(wrong[0, 2] - want[0, 2]) > 1.0
    # the per-image form: pair p's two matrices as image slots 2p, 2p + 1 over the same arena
    clip = int(np.diff(c['m_off']).max()) + 3
    kp_off = np.array([ar.kp_off[i] for ab in c['pair_img'] for i in ab], np.int64)
    slots = np.arange(2 * n_pairs, dtype=np.int32).reshape(-1, 2)
    table = np.zeros((n_pairs, clip, 2), np.int32)
    for p, (a, b) in enumerate(c['pair_img']):
        table[p, :, 0], table[p, :, 1] = ar.poison(a), ar.poison(b)
        table[p, :len(c['rows'][p])] = c['rows'][p]
    zi, _ = _triangulate_pairs(ar.xy, kp_off, c['pair_proj'].reshape(2 * n_pairs, 12), slots,
                               np.diff(c['m_off']).astype(np.int32), table, xyz=False)
    for p in range(n_pairs):
        assert np.array_equal(zi[p, :len(c['rows'][p])], z[c['m_off'][p]:c['m_off'][p + 1]]), p


# ---- similarity -----------------------------------------------------------------------------------
@functools.lru_cache(None)
def _similarity_launch(names, clip):
    """one launch of the named cases -> {name: (aff [2, 2, 3], ok [2])} (callers do not modify it)"""
    refs = [ref.similarity_reference(n) for n in names]
    c = ref.similarity_launch([(r['a'], r['b']) for r in refs], clip)
    aff, ok = _similarity(c['arena'].xy, c['arena'].kp_off, c['pair_img'], c['m_cnt'], c['m_pairs'])
    return {n: (aff[p], ok[p]) for p, n in enumerate(names)}


def _device_error(name, aff):
    """per direction: the device's error against longdouble and the tolerance it is held to"""
    r = ref.similarity_reference(name)
    out = []
    for d in (0, 1):
        err = ref.similarity_error(aff[d], r['M_ref'][d], r['scale'])
        tol = ref.similarity_tolerance(r['oracle_err'][d])
        print('%s dir %d: device error %.3g, fit_similarity %.3g, tolerance %.3g'
              % (name, d, err, r['oracle_err'][d], tol))
        out.append((err, tol))
    return out


def test_similarity_counts_and_degenerate_sets():
    """One launch of seven pairs, clip = 64 above every count, poisoned unused rows.  No match or
    one (be its keypoint finite or NaN): ok = [0, 0], zeros.  Two matches: the similarity through two points, ok = [1, 1].
    b's points identical: ok = [0, 1], direction 1 is a = b = 0 with b's point as translation.
    Direction 1 is always the reference with the roles swapped, and every (pair, direction)
    equals a launch of that pair alone (n_pairs = 1, clip = n) bit for bit.
    Measured: largest device error 1.0e-16 (fit_similarity 1.4e-16)."""
    got = _similarity_launch(ref.EDGE_CASES, 64)
    for name in ('none', 'one', 'one_nan'):
        aff, ok = got[name]
        assert ok.tolist() == [0, 0] and np.array_equal(aff, np.zeros((2, 2, 3)))
    aff, ok = got['two']
    two = ref.similarity_reference('two')
    assert ok.tolist() == [1, 1]
    for d, (p, q) in enumerate(((two['b'], two['a']), (two['a'], two['b']))):
        M2 = ref.two_point_similarity(p[0], p[1], q[0], q[1])
        assert ref.similarity_error(aff[d], M2, two['scale']) <= ref.SIM_FLOOR
    aff, ok = got['b_identical']
    bi = ref.similarity_reference('b_identical')
    assert ok.tolist() == [0, 1] and np.array_equal(aff[0], np.zeros((2, 3)))
    assert np.array_equal(np.asarray(bi['M_ref'][1][:, :2], np.float64), np.zeros((2, 2)))
    assert np.abs(aff[1][:, :2]).max() <= ref.SIM_FLOOR
    assert np.abs(aff[1][:, 2] - bi['b'][0]).max() <= ref.SIM_FLOOR * bi['scale']
    for name in ('two', 'plain', 'dry'):
        aff, ok = got[name]
        assert ok.tolist() == [1, 1]
        for d, (err, tol) in enumerate(_device_error(name, aff)):
            assert err <= tol
            r = ref.similarity_reference(name)
            # ... and fit_similarity itself, called with the roles as the direction has them
            assert ref.similarity_error(aff[d], r['oracle'][d], r['scale']) <= tol + r['oracle_err'][d]
    for name in ref.EDGE_CASES:
        r = ref.similarity_reference(name)
        aff1, ok1 = _similarity_single(r['a'], r['b'])
        assert np.array_equal(aff1, got[name][0]) and np.array_equal(ok1, got[name][1]), name


def test_similarity_sizes_and_outliers():
    """n in {2, 3, 64, 255, 256, 257, 1000, 4096} with 30 % graded outliers in one launch
    (clip = 4100), both directions against the longdouble reference; ok = [1, 1]; every pair equals
    its own single-pair launch bit for bit.
    Measured: largest device error 2.4e-16 (fit_similarity 2.7e-16 on these cases)."""
    got = _similarity_launch(ref.SIZE_CASES, 4100)
    for name in ref.SIZE_CASES:
        aff, ok = got[name]
        assert ok.tolist() == [1, 1]
        for err, tol in _device_error(name, aff):
            assert err <= tol
        r = ref.similarity_reference(name)
        aff1, ok1 = _similarity_single(r['a'], r['b'])
        assert np.array_equal(aff1, aff) and np.array_equal(ok1, ok), name


def test_similarity_schedule_runs_dry():
    """five hand-built matches: the reference keeps 5, 4, 0 inliers at 200, 50, 10 px
    (test_pair_geometry.py asserts it), so re-fit 3 has nothing to fit.  The device returns re-fit
    2's model with ok = 1: not zeros, not the first fit."""
    aff, ok = _similarity_launch(ref.EDGE_CASES, 64)['dry']
    r = ref.similarity_reference('dry')
    assert ok.tolist() == [1, 1]
    for d, (p, q) in enumerate(((r['b'], r['a']), (r['a'], r['b']))):
        assert len(r['trace'][d]) == 3 and not r['trace'][d][-1]['fitted']
        err, tol = _device_error('dry', aff)[d]
        assert err <= tol
        first = ref._fit(p.astype(np.longdouble), q.astype(np.longdouble), np.ones(5, np.longdouble))
        assert ref.similarity_error(aff[d], first, r['scale']) > 1e-4
        assert np.abs(aff[d]).max() > 0.5


# ---- ground intersection --------------------------------------------------------------------------
@pytest.mark.parametrize('n_feat', ref.GROUND_SIZES)
def test_triangulate_ground(n_feat):
    """1 to 7 observations per feature over five images, one of them looking above the horizon:
    n_sky counts its rays, they count in the divisor, a feature seen by them alone is exactly
    (0, 0, 0), and the output agrees with the ordered float64 restatement within
    1e-9 . max(1, |ref|), the bound of test_triangulate_smart_equals_reference.
    Bit-equality was the expectation and does not hold: measured largest difference 1.1e-14,
    2.8e-14, 5.7e-14, 2.8e-14 m (n_feat 1, 255, 256, 257; one or two units in the last place of
    coordinates of some hundred metres).  __dmul_rn / __dadd_rn are a plain * and + in this
    compiler's HIP headers and the file is built with the default contraction, so the products
    of M . [u, v, 1], of the norm and of v . factor fuse with the sums behind them into FMAs (one
    rounding where numpy has two); DESIGN.md, "pair geometry accuracy"."""
    import torch
    c = ref.ground_case(n_feat)
    want, want_sky = ref.ground_ordered(c['M'], c['ned'], c['base'], c['obs_img'], c['obs_uv'], c['feat_ptr'])
    assert want_sky == int(c['sky'].sum()) > 0 and np.diff(c['feat_ptr']).min() >= 1
    assert c['obs_img'].min() >= 0 and c['obs_img'].max() < 5 and c['feat_ptr'][-1] == len(c['obs_img'])
    out = _filled(3 * n_feat)
    n_sky = torch.zeros(1 + TAIL, dtype=torch.int32, device='cuda')
    keep = [_dev(c['M'], torch.float64), _dev(c['ned'], torch.float64), _dev(c['base'], torch.float64)]
    keep2 = [_dev(c['obs_img'], torch.int32), _dev(c['obs_uv'], torch.float64), _dev(c['feat_ptr'], torch.int64)]
    _call('iamx_triangulate_ground', *[_ptr(t) for t in keep], 5, *[_ptr(t) for t in keep2], n_feat,
          _ptr(out), _ptr(n_sky))
    o = out.cpu().numpy()
    got, tail = o[:3 * n_feat].reshape(n_feat, 3), o[3 * n_feat:]
    sky = n_sky.cpu().numpy()
    assert np.all(tail == FILL) and np.all(sky[1:] == 0)
    assert int(sky[0]) == want_sky
    for f in range(n_feat):
        if c['sky'][c['feat_ptr'][f]:c['feat_ptr'][f + 1]].all():
            assert np.array_equal(got[f], np.zeros(3))
    print('ground n_feat %d: largest |device - restatement| %.3g' % (n_feat, np.abs(got - want).max()))
    assert np.all(np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want)))
