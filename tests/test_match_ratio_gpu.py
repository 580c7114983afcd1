"""The 'bestratio' strategy on the device (csrc/match_ratio.hip, kernels.ratio_pairs,
matcher.ratio_pair_matches, find_matches(strategy='bestratio')) against tests/ratio_reference.py and
the goldens of the reference's own function.  The kernel edges go through the C ABI with
poison-filled outputs and guard bytes behind every buffer."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

import ratio_reference as rr
import verify_reference as vr

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = -999
NB = len(rr.CUTOFFS)


def _device_ransac(hypotheses, seed):
    """kernels.verify_pairs on one bin's points as one segment: the RANSAC callable of the restatement"""
    from imageanalysis_amd import kernels

    def run(pts, tol):
        mask, _m, _b, status = kernels.verify_pairs(pts, np.array([0, len(pts)], np.int64), 'homography',
                                                    float(tol), hypotheses=hypotheses, seed=seed)
        return None if int(status.cpu()[0]) != kernels.VERIFY_OK else mask.cpu().numpy().astype(bool)
    return run


def _abi(top2, images, slots, tol, min_pairs, hypotheses=256, seed=0, cutoffs=rr.CUTOFFS):
    """iamx_ratio_bins -> iamx_verify_pairs -> iamx_ratio_select through the C ABI.  top2: per pair
    (idx [n, 2], d2 [n, 2]); images: per slot xy float32 [m, 2]; slots: per pair (query, train);
    cutoffs: the launch's bins.  -> (per pair dict(fwd, chosen, stats, bin_cnt), flag [2])"""
    import torch
    from imageanalysis_amd import _lib, matcher
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    P, NB = len(top2), len(cutoffs)
    n = np.array([len(t[0]) for t in top2], np.int64)
    row_off = np.zeros(P + 1, np.int64)
    np.cumsum(n, out=row_off[1:])
    total, stride = int(row_off[-1]), max(int(n.max()), 1)
    tab = 64
    while tab < 2 * stride:
        tab *= 2
    cap = NB * total
    kp_off = np.zeros(len(images), np.int64)
    np.cumsum([len(x) for x in images[:-1]], out=kp_off[1:])
    xy = np.ascontiguousarray(np.concatenate(images), np.float32)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    cat = lambda k: np.concatenate([t[k] for t in top2] + [np.zeros((0, 2), np.int32)])
    d_idx, d_d2 = up(cat(0), np.int32), up(cat(1), np.int32)
    if not total:
        d_idx = d_d2 = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    d_row, d_pairs, d_kp, d_xy = up(row_off, np.int64), up(slots, np.int32), up(kp_off, np.int64), up(xy, np.float32)
    d_key = up(matcher.kp_key2(xy), np.int32)
    cut = np.asarray(cutoffs, np.float64)
    poison = lambda count, dt=torch.int32: torch.full((count + GUARD,), POISON if dt != torch.uint8 else 0xAB,
                                                      dtype=dt, device=dev)
    bin_cnt, seg_cnt, seg_off = poison(P * NB), poison(P * NB), poison(P * NB + 1, torch.int64)
    pts = torch.full((4 * cap + GUARD,), 777.0, dtype=torch.float32, device=dev)
    rows, flag = poison(2 * cap), torch.zeros(2 + GUARD, dtype=torch.int32, device=dev)
    Pt = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.iamx_ratio_bins(Pt(d_idx), Pt(d_d2), Pt(d_row), Pt(d_pairs), Pt(d_kp), Pt(d_xy), P, NB,
                           ctypes.c_void_p(cut.ctypes.data), float(min_pairs), cap, Pt(bin_cnt), Pt(seg_cnt),
                           Pt(seg_off), Pt(pts), Pt(rows), Pt(flag), st)
    assert rc == 0, L.iamx_last_error()
    mask = poison(cap, torch.uint8)
    d_tol = torch.full((P * NB,), float(tol), dtype=torch.float64, device=dev)
    model = torch.empty((P * NB, 9), dtype=torch.float64, device=dev)
    best, vstatus = poison(2 * P * NB), poison(P * NB)
    rc = L.iamx_verify_pairs(Pt(pts), Pt(seg_off), P * NB, cap, 0, Pt(d_tol), hypotheses, seed, Pt(mask),
                             Pt(model), Pt(best), Pt(vstatus), st)
    assert rc == 0, L.iamx_last_error()
    work = poison(P * (6 * stride + 2 * tab))
    out_slots, out_cnt, out_off = poison(P * stride * 2), poison(P), poison(P + 1, torch.int64)
    out_rows, chosen, stats = poison(2 * total), poison(P), poison(P * NB * 3)
    rc = L.iamx_ratio_select(Pt(d_pairs), Pt(d_kp), Pt(d_key), P, NB, float(min_pairs), rr.MIN_UNIQUE,
                             Pt(bin_cnt), Pt(seg_cnt), Pt(seg_off), Pt(rows), Pt(mask), Pt(vstatus), cap,
                             stride, tab, Pt(work), Pt(out_slots), Pt(out_cnt), Pt(out_off), Pt(out_rows),
                             total, Pt(chosen), Pt(stats), Pt(flag), st)
    assert rc == 0, L.iamx_last_error()
    torch.cuda.synchronize()
    for name, t, used in (('bin_cnt', bin_cnt, P * NB), ('seg_cnt', seg_cnt, P * NB), ('seg_off', seg_off, P * NB + 1),
                          ('rows', rows, 2 * cap), ('mask', mask, cap), ('best', best, 2 * P * NB),
                          ('vstatus', vstatus, P * NB), ('work', work, P * (6 * stride + 2 * tab)),
                          ('out_slots', out_slots, P * stride * 2), ('out_cnt', out_cnt, P),
                          ('out_off', out_off, P + 1), ('out_rows', out_rows, 2 * total), ('chosen', chosen, P),
                          ('stats', stats, P * NB * 3)):
        tail = t[used:].cpu().numpy()
        assert (tail == (0xAB if t.dtype == torch.uint8 else POISON)).all(), "guard behind %s written" % name
    assert (pts[4 * cap:].cpu().numpy() == 777.0).all() and (flag[2:].cpu().numpy() == 0).all()
    h = lambda t, used: t[:used].cpu().numpy()
    bc, sc, so = h(bin_cnt, P * NB).reshape(P, NB), h(seg_cnt, P * NB).reshape(P, NB), h(seg_off, P * NB + 1)
    assert np.array_equal(so, np.concatenate([[0], np.cumsum(sc.ravel())]))
    cnt, off, packed = h(out_cnt, P), h(out_off, P + 1), h(out_rows, 2 * total).reshape(-1, 2)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(cnt)]))
    assert (packed[int(off[-1]):] == POISON).all()
    slot_rows = h(out_slots, P * stride * 2).reshape(P, stride, 2)
    ch, stt = h(chosen, P), h(stats, P * NB * 3).reshape(P, NB, 3)
    # the materialised bins: members in query-row order, points = kp.pt of both ends
    rows_h, pts_h = h(rows, 2 * cap).reshape(-1, 2), pts[:4 * cap].cpu().numpy().reshape(-1, 4)
    out = []
    for p in range(P):
        fwd = packed[off[p]:off[p] + cnt[p]].copy()
        assert np.array_equal(fwd, slot_rows[p, :cnt[p]])
        x1, x2 = images[slots[p][0]], images[slots[p][1]]
        for b in range(NB):
            seg = rows_h[so[p * NB + b]:so[p * NB + b + 1]]
            assert (np.diff(seg[:, 0]) > 0).all() and len(seg) in (0, bc[p, b])
            assert np.array_equal(pts_h[so[p * NB + b]:so[p * NB + b + 1]],
                                  np.concatenate([x1[seg[:, 0]], x2[seg[:, 1]]], axis=1))
        assert np.array_equal(stt[p, :, 0], bc[p])
        out.append(dict(fwd=fwd, chosen=int(ch[p]), stats=stt[p].copy(), bin_cnt=bc[p].copy(), seg_cnt=sc[p].copy()))
    return out, h(flag, 2)


# ---------------------------------------------------------------------------------------------
# hand-built top-2 arrays
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge(n, seed, mode='mixed', twins=0):
    """(idx, d2, xy1, xy2): n query rows on the flat field, a fifth of them false matches displaced by
    >= 5 tol (mode 'mixed'); ratios spread over and beyond the bins, or all in bin 0 / in no bin;
    twins: rows that report the pixel of the row before them"""
    rng = np.random.default_rng(seed)
    pts = vr.scene(n, 1.0, 0.0, seed + 1)[0].astype(np.float64)
    nt = n + 5
    train = rng.permutation(nt)[:n]
    xy2 = np.stack([rng.uniform(40, rr.W_PX - 40, nt), rng.uniform(40, rr.H_PX - 40, nt)], axis=1)
    xy2[train] = pts[:, 2:]
    xy1 = pts[:, :2].copy()
    if mode == 'mixed':
        for i in np.nonzero(rng.uniform(size=n) < 0.2)[0]:
            ang = rng.uniform(0, 2 * np.pi)
            cand = pts[i, 2:] + (5 * rr.TOL + 5) * np.array([np.cos(ang), np.sin(ang)])
            xy2[train[i]] = np.clip(cand, 1, [rr.W_PX - 2, rr.H_PX - 2])
        a = np.array([rr.for_ratio(r) for r in rng.uniform(0.3, 0.95, n)])
        d2 = np.stack([a, np.full(n, 10000)], axis=1)
    else:
        d2 = np.tile([[1, 100]] if mode == 'all0' else [[99, 100]], (n, 1))
    for k in rng.permutation(np.arange(1, n))[:twins]:       # the same pixel, still on the plane
        xy1[k] = xy1[k - 1]
        xy2[train[k]] = xy2[train[k - 1]] + [0.37, -0.21]
    idx = np.stack([train, (train + 1) % nt], axis=1)
    return idx.astype(np.int32), d2.astype(np.int32), xy1.astype(np.float32), xy2.astype(np.float32)


def _restated(e, min_pairs, hypotheses=256, seed=0):
    idx, d2, xy1, xy2 = e
    return rr.ratio_pair(idx, d2, xy1, xy2, len(xy1), len(xy2), rr.TOL, min_pairs, _device_ransac(hypotheses, seed))


def _same(got, want, where=''):
    assert np.array_equal(got['fwd'], want['fwd']), where
    assert got['chosen'] == want['chosen'], where
    assert np.array_equal(got['stats'], want['stats']), (where, got['stats'], want['stats'])


EDGE_ROWS = (2, 63, 64, 65, 255, 256, 257, 513)


@pytest.mark.parametrize('n', EDGE_ROWS)
def test_query_row_edges(n):
    e = _edge(n, 500 + n, twins=min(3, n // 8))
    (got,), flag = _abi([e[:2]], [e[2], e[3]], [(0, 1)], rr.TOL, 4)
    assert flag.tolist() == [0, 0]
    want = _restated(e, 4)
    _same(got, want, n)
    if n >= 63:
        assert want['chosen'] >= 0 and len(want['fwd']) > rr.MIN_UNIQUE
        assert (np.diff(want['stats'][:, 0]) > 0).any()
    else:
        assert want['chosen'] == -1 and (want['stats'][:, 1] == -1).all()


@pytest.mark.parametrize('nb', (1, 3))
def test_fewer_bins_than_the_most(nb):
    """n_bins below the 8 the bin kernels and the walk are compiled for: the tables are [n_pairs][nb],
    the bins past nb hold no row and the walk stops at nb.  At 257 rows the widest bin of the launch wins
    with a list; at 65 rows one cutoff takes no bin (restated with rr.host_ransac(256, 0): 68 and 105
    unique at 257 rows, none and 25 at 65)"""
    cutoffs = rr.CUTOFFS[:nb]
    for n in (65, 257):
        idx, d2, xy1, xy2 = e = _edge(n, 500 + n, twins=min(3, n // 8))
        (got,), flag = _abi([e[:2]], [xy1, xy2], [(0, 1)], rr.TOL, 4, cutoffs=cutoffs)
        assert flag.tolist() == [0, 0]
        want = rr.ratio_pair(idx, d2, xy1, xy2, len(xy1), len(xy2), rr.TOL, 4, _device_ransac(256, 0),
                             cutoffs=cutoffs)
        assert got['stats'].shape == want['stats'].shape == (nb, 3)
        _same(got, want, (nb, n))
        if n == 257:
            assert want['chosen'] == nb - 1 and len(want['fwd']) > rr.MIN_UNIQUE


@pytest.mark.parametrize('n', (2001, 4097))
def test_lists_with_no_clip(n):
    """every row in bin 0 and on the plane: a list as long as the query image (past the 2000 of the
    traditional path and the 4096-slot table of its de-duplication), with repeated pixels to replay"""
    e = _edge(n, 900 + n, mode='all0', twins=7)
    (got,), flag = _abi([e[:2]], [e[2], e[3]], [(0, 1)], rr.TOL, 25)
    assert flag.tolist() == [0, 0]
    want = _restated(e, 25)
    _same(got, want, n)
    assert got['chosen'] == 0 and (got['bin_cnt'] == n).all()
    assert got['seg_cnt'].tolist() == [n] + [0] * (NB - 1)          # the later bins ARE the first
    assert (got['stats'][:, 1] == got['stats'][0, 1]).all() and len(got['fwd']) == got['stats'][0, 2]
    # (the fitted list is the one past 2000 / 4096 entries; its repeated pixels then drop out)
    assert n - 14 <= len(got['fwd']) < got['stats'][0, 1] == n


def test_all_rows_in_the_first_bin_none_in_any_and_a_batch():
    full, none = _edge(300, 41, mode='all0'), _edge(257, 42, mode='none')
    mixed = [_edge(n, 500 + n, twins=min(3, n // 8)) for n in (65, 256, 513)]
    small = _edge(2, 502)
    cases = [none, full, mixed[0], small, mixed[1], none, mixed[2]]
    images, slots = [], []
    for e in cases:
        slots.append((len(images), len(images) + 1))
        images += [e[2], e[3]]
    batch, flag = _abi([e[:2] for e in cases], images, slots, rr.TOL, 4)
    assert flag.tolist() == [0, 0]
    for k, e in enumerate(cases):
        (single,), _f = _abi([e[:2]], [e[2], e[3]], [(0, 1)], rr.TOL, 4)
        _same(batch[k], single, k)                               # a pair's place in a launch changes nothing
        _same(batch[k], _restated(e, 4), k)
    again, _f = _abi([e[:2] for e in cases], images, slots, rr.TOL, 4)
    for a, b in zip(batch, again):
        _same(a, b)
    assert (batch[0]['bin_cnt'] == 0).all() and batch[0]['chosen'] == -1 and not len(batch[0]['fwd'])
    assert (batch[1]['bin_cnt'] == 300).all() and batch[1]['chosen'] == 0 and len(batch[1]['fwd']) == 300


def test_zero_distances():
    idx, d2, xy1, xy2 = _edge(64, 77, mode='none')
    d2 = d2.copy()
    d2[:40] = [0, 50]                                            # d0 == 0: ratio 0, the first bin
    (got,), flag = _abi([(idx, d2)], [xy1, xy2], [(0, 1)], rr.TOL, 25)
    assert flag.tolist() == [0, 0] and (got['bin_cnt'] == 40).all() and len(got['fwd']) == 40
    _same(got, _restated((idx, d2, xy1, xy2), 25))
    d2[50] = [0, 0]                                              # d1 == 0: python divides by it
    d2[51] = [0, 0]
    _got, flag = _abi([(idx, d2)], [xy1, xy2], [(0, 1)], rr.TOL, 25)
    assert flag.tolist() == [2, 0]
    with pytest.raises(ZeroDivisionError):
        _restated((idx, d2, xy1, xy2), 25)


# ---------------------------------------------------------------------------------------------
# kernels.ratio_pairs and matcher.ratio_pair_matches on the goldens' inputs
# ---------------------------------------------------------------------------------------------
class KP(object):
    def __init__(self, x, y):
        self.pt = (float(x), float(y))


def _image(name, des, xy):
    from imageanalysis_amd.hostlib.image_pose import PoseImage
    im = PoseImage(name)
    im.des_list = np.asarray(des).astype(np.float32).reshape(-1, 128)
    im.kp_list = [KP(x, y) for x, y in xy]
    return im


def _configure(min_pairs=25, w=rr.W_PX, h=rr.H_PX):
    from imageanalysis_amd import matcher
    from imageanalysis_amd.hostlib import camera
    matcher.detector_node.setString('detector', 'SIFT')
    matcher.detector_node.setFloat('scale', 0.4)
    matcher.matcher_node.setFloat('match_ratio', 0.75)
    matcher.matcher_node.setInt('min_pairs', min_pairs)
    matcher.matcher_node.__dict__.pop('schedule', None)
    camera.set_image_params(w, h)
    camera.set_K(3666.6665, 3666.6665, 2736.0, 1824.0)
    matcher.configure()
    return matcher


def _ratio_pairs(pairs, min_pairs, hypotheses, seed, batch_bytes=None):
    """kernels.ratio_pairs over [dict(des1, xy1, des2, xy2)] -> per pair dict(fwd, chosen, stats)"""
    import torch
    from imageanalysis_amd import kernels, matcher
    dev = torch.device('cuda', 0)
    arrays, xy = [], []
    for p in pairs:
        arrays += [p['des1'], p['des2']]
        xy += [p['xy1'], p['xy2']]
    store = kernels.DescriptorStore.from_arrays([np.ascontiguousarray(a) for a in arrays])
    kp_off = np.zeros(len(xy), np.int64)
    np.cumsum([len(x) for x in xy[:-1]], out=kp_off[1:])
    allxy = np.ascontiguousarray(np.concatenate(xy), np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kw = {} if batch_bytes is None else dict(batch_bytes=batch_bytes)
    r = kernels.ratio_pairs(store, [(2 * k, 2 * k + 1) for k in range(len(pairs))], up(kp_off), up(allxy),
                            up(matcher.kp_key2(allxy)), rr.TOL, min_pairs, hypotheses, seed, **kw)
    assert r.flag.cpu().tolist() == [0, 0]
    off, rows = r.off.cpu().numpy(), r.rows.cpu().numpy()
    cnt, chosen, stats = r.cnt.cpu().numpy(), r.chosen.cpu().numpy(), r.stats.cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(cnt)]))
    return [dict(fwd=rows[off[k]:off[k + 1]], chosen=int(chosen[k]), stats=stats[k]) for k in range(len(pairs))]


@pytest.mark.parametrize('name', rr.CASES)
def test_composition_equals_restatement_on_golden_inputs(name):
    inp = rr.case(name)
    for hypotheses, seed in ((256, 0), (64, 12345)):
        got = _ratio_pairs(inp['pairs'], inp['min_pairs'], hypotheses, seed)
        want = rr.restate(inp, _device_ransac(hypotheses, seed))
        for k, (g, w) in enumerate(zip(got, want)):
            _same(g, w, (name, k))


def test_batched_launch_equals_single_launches_and_repeats():
    by_mp = {}
    for name in ('dups', 'early', 'gates', 'guards', 'exact', 'twentyone'):
        inp = rr.case(name)
        by_mp.setdefault(inp['min_pairs'], []).extend(inp['pairs'])
    for m, group in by_mp.items():
        batch = _ratio_pairs(group, m, 256, 0)
        again = _ratio_pairs(group, m, 256, 0)
        chunked = _ratio_pairs(group, m, 256, 0, batch_bytes=1)      # one launch per pair
        for k, p in enumerate(group):
            (single,) = _ratio_pairs([p], m, 256, 0)
            for other in (again[k], chunked[k], single):
                _same(batch[k], other, (m, k))


@pytest.mark.parametrize('name', rr.CASES)
def test_ratio_pair_matches_equals_the_reference(name):
    gold = rr.load_golden(name)
    matcher = _configure(int(gold['min_pairs']), int(gold['width']), int(gold['height']))
    for p, want in zip(gold['pairs'], gold['results']):
        i1, i2 = _image('A', p['des1'], p['xy1']), _image('B', p['des2'], p['xy2'])
        fwd, rev = matcher.ratio_pair_matches(i1, i2, hypotheses=gold['hypotheses'], seed=gold['seed'])
        assert isinstance(fwd, list) and isinstance(rev, list)
        assert np.array_equal(np.array(fwd, np.int32).reshape(-1, 2), want['fwd'])
        assert np.array_equal(np.array(rev, np.int32).reshape(-1, 2), want['rev'])
        if len(p['des1']) > 1 and len(p['des2']) > 1:
            assert np.array_equal(matcher.ratio_last['stats'], want['stats'])
            assert matcher.ratio_last['chosen'] == want['chosen']
        else:
            assert matcher.ratio_last is None and fwd == [] and rev == []


def test_zero_second_distance_raises_like_python():
    matcher = _configure(25)
    d = np.zeros((40, 128), np.uint8)
    xy = np.stack([np.arange(40) * 50.0 + 100, np.arange(40) * 30.0 + 100], axis=1).astype(np.float32)
    with pytest.raises(ZeroDivisionError):
        matcher.ratio_pair_matches(_image('A', d, xy), _image('B', d, xy))


# ---------------------------------------------------------------------------------------------
# find_matches(strategy='bestratio')
# ---------------------------------------------------------------------------------------------
def _sift_like(rng, n):
    g = rng.gamma(0.6, 1.0, size=(n, 128))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g = np.minimum(g, 0.2)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return np.clip(np.rint(g * 512.0), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _strip(n_img=8, n=600, k=300):
    """a strip of images: rows 0..k-1 of image i are rows k..2k-1 of image i - 1, shifted by
    (+250, -120) px (a camera step of 3.27 m south and 6.82 m west at 100 m, which the poses say);
    the last image has a single row (raw_matches' guards)"""
    rng = np.random.default_rng(29)
    des, xy = [], []
    for i in range(n_img):
        d = _sift_like(rng, n)
        p = np.stack([rng.uniform(600, rr.W_PX - 600, n), rng.uniform(400, rr.H_PX - 400, n)], 1)
        if i:
            d[:k] = np.clip(des[i - 1][k:2 * k].astype(int) + rng.integers(-5, 6, (k, 128)), 0, 255)
            p[:k] = xy[i - 1][k:2 * k] + [250.0, -120.0] + rng.normal(0, 0.6, (k, 2))
        des.append(d)
        xy.append(np.clip(p, 0, [rr.W_PX - 1, rr.H_PX - 1]).astype(np.float32))
    des.append(des[0][:1])
    xy.append(xy[0][:1])
    return des, xy


def _project(tag, directory):
    from imageanalysis_amd import image as iamx_image
    from imageanalysis_amd.hostlib.image_pose import PoseProject
    des, xy = _strip()
    names = ['%s%02d' % (tag, i) for i in range(len(des))]
    os.makedirs(os.path.join(directory, 'meta'), exist_ok=True)
    proj = PoseProject(names, analysis_dir=str(directory))
    for i, im in enumerate(proj.image_list):
        im.set_camera_pose([-3.2727 * i, -6.8182 * i, -100.0], 0.0, -90.0, 0.0)
        fresh = _image(names[i], des[i], xy[i])
        im.des_list, im.kp_list = fresh.des_list, fresh.kp_list
        im.match_file = os.path.join(directory, 'meta', names[i] + '.match')
        im.save_matches = types.MethodType(iamx_image.save_matches, im)
        im.load_matches = types.MethodType(iamx_image.load_matches, im)
    return proj, names


def _lists(proj):
    return {(a.name[1:], b[1:]): np.array(list(v), np.int32).reshape(-1, 2)
            for a in proj.image_list for b, v in a.match_list.items()}


def test_find_matches_bestratio(tmp_path):
    matcher = _configure(25)
    des, xy = _strip()
    n_img = len(des)
    said = []
    from imageanalysis_amd import _deps
    old_ppb, old_logger = matcher.PAIRS_PER_BATCH, _deps.logger

    class Log(object):
        def log(self, *a):
            said.append(' '.join(str(x) for x in a))

        def qlog(self, *a):
            pass
    try:
        proj, names = _project('A', tmp_path / 'one')
        matcher.find_matches(proj, None, strategy='bestratio', sort=True)          # one round
        one = _lists(proj)
        # (the schedule holds the pairs within the work list's range: four steps of the strip)
        scheduled = [(i, j) for i in range(n_img) for j in range(i + 1, n_img)
                     if (names[i][1:], names[j][1:]) in one]
        n_pairs = len(scheduled)
        assert len(one) == 2 * n_pairs and all((i, i + 1) in scheduled for i in range(n_img - 1))
        hits = 0
        for i, j in scheduled:
            a, b = proj.image_list[i], proj.image_list[j]
            fwd, rev = one[(names[i][1:], names[j][1:])], one[(names[j][1:], names[i][1:])]
            assert np.array_equal(rev, fwd[:, ::-1])                           # the mirror
            want, _r = matcher.ratio_pair_matches(a, b)
            if len(fwd) or not len(want):             # (a pair the std >= 50 rule emptied is excepted)
                assert np.array_equal(fwd, np.array(want, np.int32).reshape(-1, 2)), (i, j)
            hits += len(fwd) > 0
            if j == i + 1 and j < n_img - 1:
                assert len(want) >= 250, (i, j, len(want))                     # the planted overlap
        assert hits >= n_img - 3
        # the .match files load back
        files = {}
        for im in proj.image_list:
            files[im.name[1:]] = open(im.match_file, 'rb').read()
            kept = {k[1:]: np.array(list(v), np.int32).reshape(-1, 2) for k, v in im.match_list.items()}
            im.match_list = None
            im.load_matches()
            for k, v in im.match_list.items():
                assert np.array_equal(np.array(v, np.int32).reshape(-1, 2), kept[k[1:]])
        # a second call skips the finished pairs and retries the empty ones
        _deps.logger = lambda: Log()
        matcher.find_matches(proj, None, strategy='bestratio', sort=True)
        _deps.logger = old_logger
        assert sum(s.startswith('Skipping:') for s in said) == min(hits, 50)
        assert sum(s.startswith('Retrying:') for s in said) == min(n_pairs - hits, 50)
        two = _lists(proj)
        assert one.keys() == two.keys() and all(np.array_equal(one[k], two[k]) for k in one)
        # many rounds (the batch bound forced small) write the same files as one round
        matcher.PAIRS_PER_BATCH = 3
        many, _names = _project('B', tmp_path / 'many')
        matcher.find_matches(many, None, strategy='bestratio', sort=True)
        for im in many.image_list:
            text = open(im.match_file, 'rb').read()
            assert text.replace(b'B0', b'A0') == files[im.name[1:]], im.name
    finally:
        matcher.PAIRS_PER_BATCH, _deps.logger = old_ppb, old_logger
