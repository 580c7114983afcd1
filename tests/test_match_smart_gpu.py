"""The device pieces of the 'smart' strategy (csrc/match_knn3.hip, csrc/match_smart.hip,
kernels.knn3_pairs / knn3 / homography_fit / smart_pairs) against tests/smart_reference.py.  The
kernels go through the C ABI with poison-filled outputs and guard elements behind every buffer."""
import ctypes
import functools

import numpy as np
import pytest

import smart_reference as sr

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = -999
SIZES = (2, 3, 127, 128, 129, 255, 256, 257, 513)


def _abi_knn3(store, pairs):
    """iamx_knn3_l2_pairs through the C ABI -> (idx [total, 3], d2 [total, 3], out_off)"""
    import torch
    from imageanalysis_amd import _lib
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    counts = np.asarray(store.counts, np.int64)
    nq = counts[pairs[:, 0]]
    out_off = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum(nq, out=out_off[1:])
    wg = np.zeros(len(pairs) + 1, np.int32)
    np.cumsum([L.iamx_knn2_wg_per_pair(int(n)) for n in nq], out=wg[1:])
    total = int(out_off[-1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pairs, d_wg, d_out = up(pairs), up(wg), up(out_off[:-1])
    idx = torch.full((3 * total + GUARD,), POISON, dtype=torch.int32, device=dev)
    d2 = torch.full((3 * total + GUARD,), POISON, dtype=torch.int32, device=dev)
    Pt = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.iamx_knn3_l2_pairs(Pt(store.desc), Pt(store.norm_q), Pt(store.norm_t), Pt(store.img_off),
                              Pt(store.img_n), Pt(d_pairs), Pt(d_wg), Pt(d_out), len(pairs), int(wg[-1]),
                              Pt(idx), Pt(d2), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.iamx_last_error()
    torch.cuda.synchronize()
    for name, t in (('idx', idx), ('d2', d2)):
        assert (t[3 * total:].cpu().numpy() == POISON).all(), "guard behind %s written" % name
    return (idx[:3 * total].cpu().numpy().reshape(-1, 3), d2[:3 * total].cpu().numpy().reshape(-1, 3), out_off)


@functools.lru_cache(maxsize=None)
def _images(mode):
    """one image per size of SIZES.  'wide': rows over the whole value range, with an all-0 and an
    all-255 row (the largest distance there is: 128 * 255^2); 'ties': 0 / 1 rows in 8 dimensions, so
    that every query has many train rows at each of a few distances"""
    rng = np.random.default_rng(11 if mode == 'wide' else 12)
    out = []
    for n in SIZES:
        if mode == 'wide':
            a = rng.integers(0, 256, (n, 128)).astype(np.uint8)
            a[0] = 0
            a[-1] = 255
        else:
            a = np.zeros((n, 128), np.uint8)
            a[:, :8] = rng.integers(0, 2, (n, 8))
        out.append(a)
    return out


@functools.lru_cache(maxsize=None)
def _store(mode):
    from imageanalysis_amd import kernels
    return kernels.DescriptorStore.from_arrays(_images(mode))


@functools.lru_cache(maxsize=None)
def _want(mode, q, t):
    return sr.knn3_exact(_images(mode)[q], _images(mode)[t])


ALL_PAIRS = [(q, t) for q in range(len(SIZES)) for t in range(len(SIZES))]


@pytest.mark.parametrize('mode', ['wide', 'ties'])
def test_knn3_every_size_against_every_size_in_one_launch(mode):
    idx, d2, off = _abi_knn3(_store(mode), ALL_PAIRS)
    for p, (q, t) in enumerate(ALL_PAIRS):
        want_idx, want_d2 = _want(mode, q, t)
        where = (mode, SIZES[q], SIZES[t])
        assert np.array_equal(d2[off[p]:off[p + 1]], want_d2), where
        assert np.array_equal(idx[off[p]:off[p + 1]], want_idx), where
    if mode == 'wide':
        assert max(int(_want(mode, q, t)[1][:, :2].max()) for q, t in ALL_PAIRS) == 128 * 255 * 255
    else:
        w = _want(mode, 8, 8)[1]
        assert (w[:, 0] == w[:, 2]).sum() > 100          # (three train rows at the nearest distance)


def test_knn3_train_image_of_two_rows():
    idx, d2, off = _abi_knn3(_store('wide'), [(6, 0), (0, 0)])
    assert (idx[:, 2] == -1).all() and (d2[:, 2] == sr.D2_NONE).all()
    assert (np.sort(idx[:, :2], axis=1) == [0, 1]).all() and (d2[:, :2] <= 128 * 255 * 255).all()
    assert len(idx) == SIZES[6] + SIZES[0]


def test_knn3_first_two_columns_are_the_top2_kernel():
    from imageanalysis_amd import kernels
    for mode in ('wide', 'ties'):
        idx, d2, off = _abi_knn3(_store(mode), ALL_PAIRS)
        idx2, d22, off2 = kernels.knn2_pairs(_store(mode), ALL_PAIRS)
        assert np.array_equal(off, off2)
        assert np.array_equal(idx[:, :2], idx2.cpu().numpy()) and np.array_equal(d2[:, :2], d22.cpu().numpy())


def test_knn3_equal_distances_across_epochs_and_lane_halves():
    from imageanalysis_amd import kernels
    des_q, des_t = sr.knn3_edges()
    store = kernels.DescriptorStore.from_arrays([des_q, des_t])
    idx, d2, _off = _abi_knn3(store, [(0, 1)])
    want_idx, want_d2 = sr.knn3_exact(des_q, des_t)
    assert want_idx.tolist() == [list(w) for w in sr.KNN3_EDGE_WANT]
    assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)
    for (what, rows), got in zip(sr.KNN3_EDGES, d2):
        assert got.tolist() == sorted(o * o for _r, o in rows)[:3], what


def test_knn3_python_surface():
    from imageanalysis_amd import kernels
    imgs = _images('wide')
    pairs = [(8, 5), (3, 8), (0, 1)]
    idx, d2, off = kernels.knn3_pairs(_store('wide'), pairs)
    assert idx.shape == d2.shape == (513 + 128 + 2, 3) and off.tolist() == [0, 513, 641, 643]
    for p, (q, t) in enumerate(pairs):
        assert np.array_equal(idx[off[p]:off[p + 1]].cpu().numpy(), _want('wide', q, t)[0])
        assert np.array_equal(d2[off[p]:off[p + 1]].cpu().numpy(), _want('wide', q, t)[1])
    one_idx, one_d2 = kernels.knn3(imgs[4].astype(np.float32), imgs[7])
    assert np.array_equal(one_idx.cpu().numpy(), _want('wide', 4, 7)[0])
    assert np.array_equal(one_d2.cpu().numpy(), _want('wide', 4, 7)[1])
    with pytest.raises(ValueError):
        kernels.knn3_pairs(kernels.DescriptorStore.from_arrays([imgs[0], imgs[0][:1]]), [(0, 1)])
    empty = kernels.knn3_pairs(_store('wide'), np.zeros((0, 2), np.int32))
    assert empty[0].shape == (0, 3) and empty[2].tolist() == [0]


# ---------------------------------------------------------------------------------------------
# iamx_homography_fit
# ---------------------------------------------------------------------------------------------
def _abi_fit(segments, masks=None):
    """iamx_homography_fit over `segments` (float32 [n, 4] each) -> (H [n_seg, 3, 3], status [n_seg])"""
    import torch
    from imageanalysis_amd import _lib
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    S = len(segments)
    off = np.zeros(S + 1, np.int64)
    np.cumsum([len(s) for s in segments], out=off[1:])
    total = int(off[-1])
    pts = torch.full((4 * total + GUARD,), 777.0, dtype=torch.float32, device=dev)
    pts[:4 * total] = torch.from_numpy(np.concatenate(segments).astype(np.float32).ravel()).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    d_mask = None
    if masks is not None:
        d_mask = torch.from_numpy(np.concatenate(masks).astype(np.uint8)).to(dev)
    H = torch.full((9 * S + GUARD,), -7.0, dtype=torch.float64, device=dev)
    status = torch.full((S + GUARD,), POISON, dtype=torch.int32, device=dev)
    Pt = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    rc = L.iamx_homography_fit(Pt(pts), Pt(d_off), Pt(d_mask), S, total, Pt(H), Pt(status),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.iamx_last_error()
    torch.cuda.synchronize()
    assert (H[9 * S:].cpu().numpy() == -7.0).all() and (status[S:].cpu().numpy() == POISON).all()
    return H[:9 * S].cpu().numpy().reshape(S, 3, 3), status[:S].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fit_segments():
    """4 points (exact), 5, 81 (the prior's grid), 2049: float32 [n, 4] each, and a mask per segment
    that keeps at least 4"""
    rng = np.random.default_rng(31)
    grid = np.array([[u, v] for v in np.linspace(0, sr.H_PX, 9) for u in np.linspace(0, sr.W_PX, 9)])
    g = np.concatenate([grid, np.ones((81, 1))], axis=1) @ sr.H_TRUE.T
    segs = [sr.vr.scene(4, 1.0, 0.0, 41)[0], sr.vr.scene(5, 1.0, 0.0, 42)[0],
            np.concatenate([grid, g[:, :2] / g[:, 2:]], axis=1).astype(np.float32),
            sr.vr.scene(2049, 1.0, 0.0, 43)[0]]
    masks = []
    for s in segs:
        m = rng.uniform(size=len(s)) < 0.6
        m[rng.permutation(len(s))[:4]] = True
        masks.append(m)
    return segs, masks


def fit_bound(pts, mask=None):
    """(allowed transfer error in pixels, float64-vs-longdouble transfer error): 64 x the difference of
    the float64 restatement from its longdouble form over the segment's points, floor 1e-9 px"""
    H64, s64 = sr.fit(pts, mask)
    Hld, sld = sr.fit(pts, mask, np.longdouble)
    assert s64 == sld == sr.FIT_OK
    own = sr.transfer_error(H64, Hld, pts if mask is None else pts[mask])
    return max(64 * own, 1e-9), own, H64


@pytest.mark.parametrize('masked', [False, True])
def test_homography_fit_sizes(masked):
    segs, masks = _fit_segments()
    H, status = _abi_fit(segs, masks if masked else None)
    assert status.tolist() == [0, 0, 0, 0]
    for s, m, h in zip(segs, masks, H):
        bound, own, H64 = fit_bound(s, m if masked else None)
        used = s[m] if masked else s
        got = sr.transfer_error(h, H64, used)
        print("fit n = %4d%s: float64 vs longdouble %.3g px, device vs float64 %.3g px (allowed %.3g)"
              % (len(used), ' masked' if masked else '', own, got, bound))
        assert h[2, 2] == 1.0 and got <= bound
        if len(used) == 4:                                      # four points: the fit goes through them
            x = np.concatenate([used[:, :2], np.ones((4, 1))], axis=1) @ h.T
            assert np.abs(x[:, :2] / x[:, 2:] - used[:, 2:]).max() < 1e-6


def test_homography_fit_status():
    good = sr.vr.scene(30, 1.0, 0.0, 44)[0]
    nan = good.copy()
    nan[7, 2] = np.nan
    one_side = good.copy()
    one_side[:, :2] = one_side[0, :2]
    segs = [good[:3], sr.vr.identical(12), nan, one_side, good, good[:0]]
    H, status = _abi_fit(segs)
    assert status.tolist() == [sr.FIT_TOO_FEW, sr.FIT_DEGENERATE, sr.FIT_DEGENERATE, sr.FIT_DEGENERATE,
                               sr.FIT_OK, sr.FIT_TOO_FEW]
    assert [sr.fit(s)[1] for s in segs] == status.tolist()
    assert np.isnan(H[[0, 1, 2, 3, 5]]).all() and np.isfinite(H[4]).all()
    # a mask that leaves three points
    m = np.zeros(30, bool)
    m[[1, 8, 20]] = True
    assert _abi_fit([good], [m])[1].tolist() == [sr.FIT_TOO_FEW]


def test_homography_fit_python_surface():
    from imageanalysis_amd import kernels
    segs, masks = _fit_segments()
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    H, status = kernels.homography_fit(np.concatenate(segs), off, np.concatenate(masks))
    H2, _s = _abi_fit(segs, masks)
    assert status.cpu().numpy().tolist() == [0, 0, 0, 0] and np.array_equal(H.cpu().numpy(), H2)
    assert kernels.FIT_OK == sr.FIT_OK and kernels.FIT_TOO_FEW == sr.FIT_TOO_FEW
    assert kernels.FIT_DEGENERATE == sr.FIT_DEGENERATE and kernels.homography_fit(segs[0][:0], [0])[0].shape[0] == 0


# ---------------------------------------------------------------------------------------------
# iamx_smart_stats / iamx_smart_select
# ---------------------------------------------------------------------------------------------
NB = len(sr.CUTOFFS)


def _device_ransac(hypotheses=sr.HYPOTHESES, seed=sr.SEED):
    """kernels.verify_pairs on one bin's points as one segment: the consensus callable of the restatement"""
    from imageanalysis_amd import kernels

    def run(pts, tol):
        mask, model, _b, status = kernels.verify_pairs(pts, np.array([0, len(pts)], np.int64), 'homography',
                                                       float(tol), hypotheses=hypotheses, seed=seed)
        if int(status.cpu()[0]) != kernels.VERIFY_OK:
            return None
        return mask.cpu().numpy().astype(bool), model.cpu().numpy().reshape(9)
    return run


class _Batch(object):
    """a batch of pairs held on the device for iamx_smart_stats -> iamx_verify_pairs -> iamx_smart_select
    through the C ABI: the k = 3 neighbours (restated), the keypoint arena, the pairs' state"""

    def __init__(self, pairs, min_pairs, tol):
        import torch
        from imageanalysis_amd import matcher
        self.dev = dev = torch.device('cuda', 0)
        self.pairs, self.min_pairs, self.tol = pairs, min_pairs, tol
        P = self.P = len(pairs)
        top3 = [sr.knn3_exact(p['des1'], p['des2']) for p in pairs]
        n = np.array([len(p['des1']) for p in pairs], np.int64)
        self.row_off = np.zeros(P + 1, np.int64)
        np.cumsum(n, out=self.row_off[1:])
        self.total, self.stride = int(self.row_off[-1]), int(n.max())
        self.tab = 64
        while self.tab < 2 * self.stride:
            self.tab *= 2
        self.cap = NB * self.total
        images = [a for p in pairs for a in (p['xy1'], p['xy2'])]
        kp_off = np.zeros(2 * P, np.int64)
        np.cumsum([len(x) for x in images[:-1]], out=kp_off[1:])
        xy = np.ascontiguousarray(np.concatenate(images), np.float32)
        size = np.concatenate([a for p in pairs for a in (p['size1'], p['size2'])]).astype(np.float32)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        self.idx, self.d2 = up(np.concatenate([t[0] for t in top3]), np.int32), up(np.concatenate([t[1] for t in top3]), np.int32)
        self.d_row, self.d_kp, self.d_xy = up(self.row_off, np.int64), up(kp_off, np.int64), up(xy, np.float32)
        self.d_pairs = up(np.arange(2 * P).reshape(P, 2), np.int32)
        self.d_size, self.d_key = up(size, np.float32), up(matcher.kp_key2(xy), np.int32)
        # the state the passes carry: poison where a pass must not write
        self.H = torch.full((9 * P + GUARD,), -7.0, dtype=torch.float64, device=dev)
        self.H[:9 * P] = up(np.stack([p['H0'] for p in pairs]).ravel(), np.float64)
        self.best = torch.full((2 * P + GUARD,), POISON, dtype=torch.int32, device=dev)
        self.best[:2 * P] = up(np.tile([sr.MIN_UNIQUE, 0], P), np.int32)
        self.slots = torch.full((P * self.stride * 2 + GUARD,), POISON, dtype=torch.int32, device=dev)
        self.cnt = torch.full((P + GUARD,), POISON, dtype=torch.int32, device=dev)
        self.cnt[:P] = 0
        self.stats = torch.full((P * NB * 3 + GUARD,), POISON, dtype=torch.int32, device=dev)
        self.fit_status = torch.full((P + GUARD,), POISON, dtype=torch.int32, device=dev)
        self.flag = torch.zeros(2 + GUARD, dtype=torch.int32, device=dev)

    def run(self, active, hypotheses=sr.HYPOTHESES, seed=sr.SEED):
        """one pass -> dict of host arrays"""
        import torch
        from imageanalysis_amd import _lib
        L, dev, P, cap, total = _lib.lib(), self.dev, self.P, self.cap, self.total
        poison = lambda count, dt=torch.int32: torch.full((count + GUARD,), POISON if dt != torch.uint8 else 0xAB,
                                                          dtype=dt, device=dev)
        Pt = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        d_act = None if active is None else torch.from_numpy(np.asarray(active, np.int32)).to(dev)
        bin_cnt, seg_cnt, seg_off = poison(P * NB), poison(P * NB), poison(P * NB + 1, torch.int64)
        pts = torch.full((4 * cap + GUARD,), 777.0, dtype=torch.float32, device=dev)
        rows = poison(2 * cap)
        rc = L.iamx_smart_stats(Pt(self.idx), Pt(self.d2), Pt(self.d_row), Pt(self.d_pairs), Pt(self.d_kp),
                                Pt(self.d_xy), Pt(self.d_size), Pt(self.H), Pt(d_act), P, sr.MATCH_RATIO,
                                float(self.min_pairs), cap, Pt(bin_cnt), Pt(seg_cnt), Pt(seg_off), Pt(pts),
                                Pt(rows), Pt(self.flag), st)
        assert rc == 0, L.iamx_last_error()
        mask = poison(cap, torch.uint8)
        d_tol = torch.full((P * NB,), float(self.tol), dtype=torch.float64, device=dev)
        model = torch.empty((P * NB, 9), dtype=torch.float64, device=dev)
        vbest, vstatus = poison(2 * P * NB), poison(P * NB)
        rc = L.iamx_verify_pairs(Pt(pts), Pt(seg_off), P * NB, cap, 0, Pt(d_tol), hypotheses, seed, Pt(mask),
                                 Pt(model), Pt(vbest), Pt(vstatus), st)
        assert rc == 0, L.iamx_last_error()
        work = poison(P * (6 * self.stride + 2 * self.tab))
        improved, out_off, out_rows = poison(P), poison(P + 1, torch.int64), poison(2 * total)
        rc = L.iamx_smart_select(Pt(self.d_pairs), Pt(self.d_kp), Pt(self.d_key), Pt(d_act), P, float(self.min_pairs),
                                 Pt(bin_cnt), Pt(seg_cnt), Pt(seg_off), Pt(pts), Pt(rows), Pt(mask), Pt(vstatus),
                                 Pt(model), cap, self.stride, self.tab, Pt(work), Pt(self.best), Pt(improved),
                                 Pt(self.slots), Pt(self.cnt), Pt(out_off), Pt(out_rows), total, Pt(self.stats),
                                 Pt(self.H), Pt(self.fit_status), Pt(self.flag), st)
        assert rc == 0, L.iamx_last_error()
        torch.cuda.synchronize()
        for name, t, used in (('bin_cnt', bin_cnt, P * NB), ('seg_cnt', seg_cnt, P * NB), ('seg_off', seg_off, P * NB + 1),
                              ('rows', rows, 2 * cap), ('mask', mask, cap), ('vstatus', vstatus, P * NB),
                              ('work', work, P * (6 * self.stride + 2 * self.tab)), ('improved', improved, P),
                              ('out_off', out_off, P + 1), ('out_rows', out_rows, 2 * total),
                              ('best', self.best, 2 * P), ('slots', self.slots, P * self.stride * 2),
                              ('cnt', self.cnt, P), ('stats', self.stats, P * NB * 3),
                              ('fit_status', self.fit_status, P)):
            tail = t[used:].cpu().numpy()
            assert (tail == (0xAB if t.dtype == torch.uint8 else POISON)).all(), "guard behind %s written" % name
        assert (pts[4 * cap:].cpu().numpy() == 777.0).all() and (self.flag[2:].cpu().numpy() == 0).all()
        assert (self.H[9 * P:].cpu().numpy() == -7.0).all()
        h = lambda t, used: t[:used].cpu().numpy()
        so, sc = h(seg_off, P * NB + 1), h(seg_cnt, P * NB).reshape(P, NB)
        assert np.array_equal(so, np.concatenate([[0], np.cumsum(sc.ravel())]))
        cnt, off = h(self.cnt, P), h(out_off, P + 1)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(cnt)]))
        packed = h(out_rows, 2 * total).reshape(-1, 2)
        assert (packed[int(off[-1]):] == POISON).all()
        slots = h(self.slots, P * self.stride * 2).reshape(P, self.stride, 2)
        for p in range(P):
            assert np.array_equal(packed[off[p]:off[p] + cnt[p]], slots[p, :cnt[p]])
        rows_h, pts_h = h(rows, 2 * cap).reshape(-1, 2), pts[:4 * cap].cpu().numpy().reshape(-1, 4)
        members = [[rows_h[so[p * NB + b]:so[p * NB + b + 1]] for b in range(NB)] for p in range(P)]
        for p, pr in enumerate(self.pairs):                      # the materialised points are kp.pt of both ends
            for seg in members[p]:
                assert (np.diff(seg[:, 0]) > 0).all()
            a, b = so[p * NB], so[(p + 1) * NB]
            assert np.array_equal(pts_h[a:b], np.concatenate([pr['xy1'][rows_h[a:b, 0]], pr['xy2'][rows_h[a:b, 1]]], axis=1))
        return dict(bin_cnt=h(bin_cnt, P * NB).reshape(P, NB), seg_cnt=sc, members=members,
                    improved=h(improved, P), best=h(self.best, 2 * P).reshape(P, 2), cnt=cnt, slots=slots,
                    stats=h(self.stats, P * NB * 3).reshape(P, NB, 3), H=h(self.H, 9 * P).reshape(P, 3, 3),
                    fit_status=h(self.fit_status, P), flag=h(self.flag, 2))


def _check_pass(got, p, want, pair, min_pairs, where):
    """pair p of a device pass against one_pass()' dict"""
    assert np.array_equal(got['stats'][p], want['stats']), (where, got['stats'][p], want['stats'])
    assert np.array_equal(got['bin_cnt'][p], want['stats'][:, 0]), where
    assert got['improved'][p] == want['taken'], where
    prev = -1
    for b, mem in enumerate(want['members']):                    # the bins, where they were materialised
        looked = len(mem) >= min_pairs and len(mem) >= 4
        assert got['seg_cnt'][p, b] == (len(mem) if looked and len(mem) != prev else 0), (where, b)
        if got['seg_cnt'][p, b]:
            assert np.array_equal(got['members'][p][b], np.asarray(mem, np.int32).reshape(-1, 2)), (where, b)
        if looked:
            prev = len(mem)
    if want['taken']:
        uniq = sr.dedupe(pair['xy1'], pair['xy2'], want['fit'])
        assert got['best'][p].tolist() == [len(uniq), len(want['fit'])] == [want['best'], len(want['fit'])], where
        assert np.array_equal(got['slots'][p, :len(uniq)], np.asarray(uniq, np.int32)), where
        assert got['cnt'][p] == (len(uniq) if min(len(uniq), len(want['fit'])) >= min_pairs else 0), where
        assert got['fit_status'][p] == want['fit_status'] == sr.FIT_OK, where
        m = np.asarray(want['fit'], np.int64)
        pts = np.concatenate([pair['xy1'][m[:, 0]], pair['xy2'][m[:, 1]]], axis=1)
        bound, _own, _h = fit_bound(pts)
        assert sr.transfer_error(got['H'][p], want['H'], pts) <= bound, where


@functools.lru_cache(maxsize=None)
def _case_restated(name):
    return sr.restate(sr.case(name), _device_ransac())


BATCHED = ('clean', 'two_pass', 'second_nn', 'sizes', 'cuts', 'dups', 'gates')      # min_pairs 25


def test_smart_passes_of_a_batch_of_unequal_pairs():
    """every pair of the cases at min_pairs = 25 in ONE launch per pass, pass after pass until none
    improves: bins, stats, improved, lists, H and pass counts against the restatement; a pair that is
    not active in a pass keeps everything"""
    pairs, want = [], []
    for name in BATCHED:
        pairs += sr.case(name)['pairs']
        want += _case_restated(name)
    assert len(set(len(p['des1']) for p in pairs)) > 4
    B = _Batch(pairs, 25, sr.TOL)
    active = np.ones(len(pairs), np.int32)
    k, before = 0, None
    while active.any():
        got = B.run(None if k == 0 else active)
        assert got['flag'].tolist() == [0, 0]
        for p, (pr, w) in enumerate(zip(pairs, want)):
            if active[p]:
                assert k < len(w['passes']), (p, k)
                _check_pass(got, p, w['passes'][k], pr, 25, (p, k))
                if not w['passes'][k]['taken']:                  # no gain: the list of the pass before stays
                    for key in ('best', 'cnt', 'slots', 'H', 'fit_status'):
                        assert before is None or np.array_equal(got[key][p], before[key][p]), (p, k, key)
            else:
                assert len(w['passes']) <= k and got['improved'][p] == 0
                assert (got['bin_cnt'][p] == 0).all() and (got['seg_cnt'][p] == 0).all()
                for key in ('best', 'cnt', 'slots', 'H', 'fit_status', 'stats'):
                    assert np.array_equal(got[key][p], before[key][p]), (p, k, key)
        active = (got['improved'] > 0).astype(np.int32)
        before, k = got, k + 1
    assert k == max(len(w['passes']) for w in want) == 3
    for p, w in enumerate(want):                                 # the lists after the gates
        assert np.array_equal(before['slots'][p, :before['cnt'][p]], w['fwd']), p


@pytest.mark.parametrize('name', ['below20', 'twentyone', 'two_rows'])
def test_smart_pass_small_cases(name):
    inp = sr.case(name)
    want = _case_restated(name)[0]
    B = _Batch(inp['pairs'], inp['min_pairs'], sr.TOL)
    for k, w in enumerate(want['passes']):
        got = B.run(None)
        _check_pass(got, 0, w, inp['pairs'][0], inp['min_pairs'], (name, k))
    assert got['improved'][0] == 0 and np.array_equal(got['slots'][0, :got['cnt'][0]], want['fwd'])
    assert len(want['fwd']) == (21 if name == 'twentyone' else 0)


def test_smart_stats_flags_a_zero_distance():
    inp = sr.case('zero')
    B = _Batch(inp['pairs'], inp['min_pairs'], sr.TOL)
    assert B.run(None)['flag'].tolist() == [1, 0]
    B2 = _Batch(inp['pairs'], inp['min_pairs'], sr.TOL)
    assert B2.run([0])['flag'].tolist() == [0, 0]                # an inactive pair raises nothing


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def _arena(pairs):
    """(store, slots [P, 2], kp_off, xy, size, key2) of a list of case pairs, two images each"""
    import torch
    from imageanalysis_amd import kernels, matcher
    dev = torch.device('cuda', 0)
    des = [a for p in pairs for a in (p['des1'], p['des2'])]
    des = [np.zeros((0, 128), np.uint8) if a is None else a for a in des]
    store = kernels.DescriptorStore.from_arrays(des)
    images = [a for p in pairs for a in (p['xy1'], p['xy2'])]
    kp_off = np.zeros(len(images), np.int64)
    np.cumsum([len(x) for x in images[:-1]], out=kp_off[1:])
    xy = np.ascontiguousarray(np.concatenate(images), np.float32)
    size = np.concatenate([a for p in pairs for a in (p['size1'], p['size2'])]).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return store, np.arange(len(images)).reshape(-1, 2), up(kp_off), up(xy), up(size), up(matcher.kp_key2(xy))


def test_smart_pairs_equals_the_restatement_on_every_case():
    from imageanalysis_amd import kernels
    for min_pairs, names in ((25, BATCHED), (10, ('below20', 'twentyone', 'two_rows', 'guards'))):
        pairs, want = [], []
        for name in names:
            pairs += [dict(p, des1=p['des1'] if p['des1'] is not None else np.zeros((0, 128), np.uint8),
                           des2=p['des2'] if p['des2'] is not None else np.zeros((0, 128), np.uint8))
                      for p in sr.case(name)['pairs']]
            want += _case_restated(name)
        store, slots, kp_off, xy, size, key2 = _arena(pairs)
        r = kernels.smart_pairs(store, slots, kp_off, xy, size, key2, np.stack([p['H0'] for p in pairs]), sr.TOL,
                                min_pairs, sr.MATCH_RATIO, hypotheses=sr.HYPOTHESES, seed=sr.SEED)
        assert r.flag.tolist() == [0, 0]
        off, cnt, rows = r.off.cpu().numpy(), r.cnt.cpu().numpy(), r.rows.cpu().numpy()
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(cnt)]))
        for p, w in enumerate(want):
            assert np.array_equal(rows[off[p]:off[p + 1]], w['fwd']), p
            assert r.passes[p] == len(w['passes']), p
            assert r.best[p].tolist() == list(w['best']), p
            for k, wp in enumerate(w['passes']):
                assert np.array_equal(r.stats[k][p], wp['stats']) and r.taken[k][p] == wp['taken'], (p, k)
            for k in range(len(w['passes']), len(r.stats)):
                assert (r.stats[k][p] == -2).all() and r.taken[k][p] == 0


def test_smart_pairs_equals_every_pair_golden():
    """kernels.smart_pairs on the goldens' own inputs, from the H0 the reference's prior produced:
    the reference's lists, the per-pass figures it printed, the bins it took and its pass counts"""
    from imageanalysis_amd import kernels
    empty = np.zeros((0, 128), np.uint8)
    for name in sr.PAIR_CASES + ('guards',):
        g = sr.load_golden(name)
        pairs = [dict(p, des1=p['des1'] if p['des1'] is not None else empty,
                      des2=p['des2'] if p['des2'] is not None else empty) for p in g['pairs']]
        store, slots, kp_off, xy, size, key2 = _arena(pairs)
        r = kernels.smart_pairs(store, slots, kp_off, xy, size, key2, np.stack([p['H0'] for p in pairs]), g['tol'],
                                g['min_pairs'], g['match_ratio'], hypotheses=g['hypotheses'], seed=g['seed'])
        assert r.flag.tolist() == [0, 0]
        off, rows = r.off.cpu().numpy(), r.rows.cpu().numpy()
        for p, want in enumerate(g['results']):
            assert np.array_equal(rows[off[p]:off[p + 1]], want['fwd']), (name, p)
            assert r.passes[p] == len(want['passes']), (name, p)
            for k, wp in enumerate(want['passes']):
                assert np.array_equal(r.stats[k][p], wp['stats']) and r.taken[k][p] == wp['taken'], (name, p, k)


@pytest.fixture
def fresh_matcher():
    """a DeviceMatcher of its own per test (the cases re-use the image names A and B)"""
    from imageanalysis_amd import matcher
    saved = {n: getattr(matcher, n) for n in ('the_matcher', 'max_distance', 'min_pairs')}
    yield matcher
    for n, v in saved.items():
        setattr(matcher, n, v)
    matcher.matcher_node.__dict__.pop('ground_m', None)


@pytest.mark.parametrize('name', sr.ALL_CASES)
def test_smart_pair_matches_equals_the_reference_function(fresh_matcher, name):
    """matcher.smart_pair_matches -- the prior from the poses, the k = 3 search, the passes on the
    device -- against the golden of the reference's own function"""
    from test_match_smart import attach, pose_pair
    matcher = fresh_matcher
    g = sr.load_golden(name)
    for p, want in zip(g['pairs'], g['results']):
        i1, i2 = pose_pair(p['pose'], g['min_pairs'])
        matcher.the_matcher = None
        matcher.configure()
        attach(i1, p['des1'], p['xy1'], p['size1'])
        attach(i2, p['des2'], p['xy2'], p['size2'])
        if want['raised']:
            with pytest.raises(ZeroDivisionError):
                matcher.smart_pair_matches(i1, i2, False, True, hypotheses=g['hypotheses'], seed=g['seed'])
            continue
        fwd, rev = matcher.smart_pair_matches(i1, i2, False, True, hypotheses=g['hypotheses'], seed=g['seed'])
        assert np.array_equal(np.asarray(fwd, np.int32).reshape(-1, 2), want['fwd']), name
        assert np.array_equal(np.asarray(rev, np.int32).reshape(-1, 2), want['rev']), name
        if want['passes']:
            last = matcher.smart_last
            assert last['passes'] == len(want['passes']) and last['taken'] == [q['taken'] for q in want['passes']]
            for a, b in zip(last['stats'], want['passes']):
                assert np.array_equal(a, b['stats']), name
            assert sr.transfer_error(last['H0'], want['H0'], want['reproj']) <= max(1e-6, 1000 * want['prior_noise'])


@pytest.mark.parametrize('sort', [False, True])
def test_smart_matches_equals_the_reference_loop(fresh_matcher, sort):
    """the shipped pair loop end to end, nothing replaced: against the reference's
    find_matches(strategy='smart') on the strip, and a second call on the same project"""
    from test_match_smart import strip_project
    matcher = fresh_matcher
    g, s, proj, loop = strip_project(device=True)
    for call in range(2):
        matcher.smart_matches(proj, None, sort=sort)
        loop.check_against(g, s['runs'][sort], call, proj)


def test_smart_pairs_raises_the_flag_of_the_zero_case():
    from imageanalysis_amd import kernels
    pairs = sr.case('zero')['pairs']
    store, slots, kp_off, xy, size, key2 = _arena(pairs)
    r = kernels.smart_pairs(store, slots, kp_off, xy, size, key2, [pairs[0]['H0']], sr.TOL, 10, sr.MATCH_RATIO,
                            hypotheses=sr.HYPOTHESES)
    assert r.flag.tolist() == [1, 0] and len(r.stats) == 1
