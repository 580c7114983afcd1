"""The 'bruteforce' strategy on the device: iamx_brute_bins and iamx_brute_select through the C ABI
(poison-filled outputs, guard elements behind every buffer) against the numpy restatement
(tests/brute_reference.py), by equality; kernels.brute_pairs and the matcher's entries against the
goldens of the reference's own function and loop (tools/gen_brute_golden.py)."""
import ctypes
import functools

import numpy as np
import pytest

import brute_reference as br

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = -999
NC = br.NC


def _device():
    import torch
    return torch.device('cuda', 0)


def _tab(stride):
    t = 64
    while t < 2 * stride:
        t *= 2
    return t


def _guards_intact(named):
    import torch
    for name, t, used in named:
        tail = t[used:].cpu().numpy()
        want = 0xAB if t.dtype == torch.uint8 else (777.0 if t.dtype == torch.float32 else POISON)
        assert (tail == want).all(), "guard behind %s written" % name


def run_bins(pairs, top3, min_pairs, match_ratio=br.MATCH_RATIO, step_d=br.STEP_D):
    """iamx_brute_bins through the C ABI.  pairs: [dict(xy1, xy2, size1, size2)]; top3: per pair (idx
    [n, 3], d2 [n, 3]).  -> dict of host arrays; the exclusive scan, the materialised points and the
    member order are checked here for every call"""
    import torch
    from imageanalysis_amd import _lib
    L, dev, P = _lib.lib(), _device(), len(pairs)
    n = np.array([len(t[0]) for t in top3], np.int64)
    row_off = np.zeros(P + 1, np.int64)
    np.cumsum(n, out=row_off[1:])
    total = int(row_off[-1])
    cap = 9 * total
    images = [a for p in pairs for a in (p['xy1'], p['xy2'])]
    kp_off = np.zeros(2 * P, np.int64)
    np.cumsum([len(x) for x in images[:-1]], out=kp_off[1:])
    xy = np.ascontiguousarray(np.concatenate(images), np.float32)
    size = np.concatenate([a for p in pairs for a in (p['size1'], p['size2'])]).astype(np.float32)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    poison = lambda count, dt=torch.int32: torch.full((count + GUARD,), POISON, dtype=dt, device=dev)
    Pt = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = up(np.concatenate([t[0] for t in top3]).reshape(-1, 3), np.int32)
    d2 = up(np.concatenate([t[1] for t in top3]).reshape(-1, 3), np.int32)
    d_row, d_kp, d_xy, d_size = up(row_off, np.int64), up(kp_off, np.int64), up(xy, np.float32), up(size, np.float32)
    d_pairs = up(np.arange(2 * P).reshape(P, 2), np.int32)
    bin_cnt, seg_cnt, seg_off = poison(P * NC), poison(P * NC), poison(P * NC + 1, torch.int64)
    pts = torch.full((4 * cap + GUARD,), 777.0, dtype=torch.float32, device=dev)
    rows = poison(2 * cap)
    flag = torch.zeros(2 + GUARD, dtype=torch.int32, device=dev)
    rc = L.iamx_brute_bins(Pt(idx), Pt(d2), Pt(d_row), Pt(d_pairs), Pt(d_kp), Pt(d_xy), Pt(d_size), P,
                           float(match_ratio), float(min_pairs), float(step_d), br.STEP_A, cap, Pt(bin_cnt),
                           Pt(seg_cnt), Pt(seg_off), Pt(pts), Pt(rows), Pt(flag), st)
    assert rc == 0, L.iamx_last_error()
    torch.cuda.synchronize()
    _guards_intact((('bin_cnt', bin_cnt, P * NC), ('seg_cnt', seg_cnt, P * NC), ('seg_off', seg_off, P * NC + 1),
                    ('rows', rows, 2 * cap), ('pts', pts, 4 * cap)))
    assert (flag[2:].cpu().numpy() == 0).all()
    h = lambda t, used: t[:used].cpu().numpy()
    so, sc = h(seg_off, P * NC + 1), h(seg_cnt, P * NC).reshape(P, NC)
    assert np.array_equal(so, np.concatenate([[0], np.cumsum(sc.ravel())]))
    used = int(so[-1])
    rows_h, pts_h = h(rows, 2 * cap).reshape(-1, 2), h(pts, 4 * cap).reshape(-1, 4)
    assert (rows_h[used:] == POISON).all() and (pts_h[used:] == 777.0).all()      # nothing past the segments
    for p, pr in enumerate(pairs):
        a, b = so[p * NC], so[(p + 1) * NC]
        assert np.array_equal(pts_h[a:b], np.concatenate([np.asarray(pr['xy1'], np.float32)[rows_h[a:b, 0]],
                                                          np.asarray(pr['xy2'], np.float32)[rows_h[a:b, 1]]], axis=1))
        for c in np.nonzero(sc[p])[0]:                           # member order: query rows strictly ascend
            seg = rows_h[so[p * NC + c]:so[p * NC + c + 1]]
            assert (np.diff(seg[:, 0]) > 0).all(), (p, c)
    return dict(bin_cnt=h(bin_cnt, P * NC).reshape(P, NC), seg_cnt=sc, seg_off=so, rows=rows_h[:used],
                pts=pts_h[:used], flag=h(flag, 2))


def check_bins(got, p, want):
    """pair p of run_bins() against brute_reference.bins()"""
    assert np.array_equal(got['bin_cnt'][p], want['bin_cnt']), p
    assert np.array_equal(got['seg_cnt'][p], want['seg_cnt']), p
    a, b = got['seg_off'][p * NC], got['seg_off'][(p + 1) * NC]
    assert np.array_equal(got['rows'][a:b], want['rows']), p
    assert np.array_equal(got['pts'][a:b], want['pts']), p


def run_select(pairs, seg_cnt, rows, mask, vstatus, min_pairs, stride):
    """iamx_brute_select through the C ABI on hand-made segments.  pairs: [dict(xy1, xy2)]; seg_cnt
    [P, NC]; rows [m, 2] / mask [m] back to back; vstatus [P, NC].  -> dict of host arrays"""
    import torch
    from imageanalysis_amd import _lib, matcher
    L, dev, P = _lib.lib(), _device(), len(pairs)
    images = [a for p in pairs for a in (p['xy1'], p['xy2'])]
    kp_off = np.zeros(2 * P, np.int64)
    np.cumsum([len(x) for x in images[:-1]], out=kp_off[1:])
    xy = np.ascontiguousarray(np.concatenate(images), np.float32)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    poison = lambda count, dt=torch.int32: torch.full((count + GUARD,), POISON, dtype=dt, device=dev)
    Pt = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    seg_cnt = np.asarray(seg_cnt, np.int32).reshape(P, NC)
    seg_off = np.concatenate([[0], np.cumsum(seg_cnt.ravel())]).astype(np.int64)
    cap = max(int(seg_off[-1]), 1)
    tab = _tab(stride)
    d_rows = up(np.asarray(rows, np.int32).reshape(-1, 2) if len(rows) else np.zeros((1, 2), np.int32), np.int32)
    d_mask = up(np.asarray(mask, np.uint8) if len(mask) else np.zeros(1, np.uint8), np.uint8)
    work = poison(P * (6 * stride + 2 * tab))
    slots, cnt, out_off = poison(P * stride * 2), poison(P), poison(P + 1, torch.int64)
    out_cap = P * stride
    out_rows, chosen, stats, fit_cnt = poison(2 * out_cap), poison(P), poison(4 * P), poison(P * NC)
    flag = torch.zeros(2 + GUARD, dtype=torch.int32, device=dev)
    # (every input is held by a name until the synchronize below: a temporary's block goes back to the
    #  allocator at once and the next upload may land in it before the kernel has run)
    d_pairs, d_kp, d_key = up(np.arange(2 * P).reshape(P, 2), np.int32), up(kp_off, np.int64), up(matcher.kp_key2(xy), np.int32)
    d_cnt, d_off, d_vs = up(seg_cnt, np.int32), up(seg_off, np.int64), up(vstatus, np.int32)
    rc = L.iamx_brute_select(Pt(d_pairs), Pt(d_kp), Pt(d_key), P, float(min_pairs), Pt(d_cnt), Pt(d_off), Pt(d_rows),
                             Pt(d_mask), Pt(d_vs), cap, stride, tab, Pt(work), Pt(slots), Pt(cnt), Pt(out_off),
                             Pt(out_rows), out_cap, Pt(chosen), Pt(stats), Pt(fit_cnt), Pt(flag), st)
    assert rc == 0, L.iamx_last_error()
    torch.cuda.synchronize()
    _guards_intact((('work', work, P * (6 * stride + 2 * tab)), ('slots', slots, P * stride * 2), ('cnt', cnt, P),
                    ('out_off', out_off, P + 1), ('out_rows', out_rows, 2 * out_cap), ('chosen', chosen, P),
                    ('stats', stats, 4 * P), ('fit_cnt', fit_cnt, P * NC)))
    h = lambda t, used: t[:used].cpu().numpy()
    assert h(flag, 2 + GUARD).tolist() == [0] * (2 + GUARD)
    c, off = h(cnt, P), h(out_off, P + 1)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(c)]))
    packed = h(out_rows, 2 * out_cap).reshape(-1, 2)
    assert (packed[int(off[-1]):] == POISON).all()
    sl = h(slots, P * stride * 2).reshape(P, stride, 2)
    lists = []
    for p in range(P):
        assert np.array_equal(packed[off[p]:off[p] + c[p]], sl[p, :c[p]])
        lists.append(sl[p, :c[p]].copy())
    return dict(lists=lists, chosen=h(chosen, P), stats=h(stats, 4 * P).reshape(P, 4),
                fit_cnt=h(fit_cnt, P * NC).reshape(P, NC))


# ---------------------------------------------------------------------------------------------
# iamx_brute_bins
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', br.PAIR_CASES + ('zero',))
def test_bins_equal_the_restatement_on_the_constructed_cases(name):
    inp = br.case(name)
    for min_pairs in sorted(set(p['min_pairs'] for p in inp['pairs'])):
        pairs = [p for p in inp['pairs'] if p['min_pairs'] == min_pairs]
        top3 = [br.knn3_exact(p['des1'], p['des2']) for p in pairs]
        got = run_bins(pairs, top3, min_pairs)
        zeros = 0
        for k, (p, t) in enumerate(zip(pairs, top3)):
            want = br.bins(t[0], t[1], p['xy1'], p['xy2'], p['size1'], p['size2'], br.MATCH_RATIO, min_pairs, br.STEP_D)
            check_bins(got, k, want)
            zeros += want['zeros']
        assert got['flag'].tolist() == [zeros, 0] and zeros == (1 if name == 'zero' else 0)


def _random_pair(rng, nq, nt, mode='mixed'):
    """fabricated top-3 rows and keypoints: motions in a few clusters (cells that fill up) and anywhere,
    distances on both sides of every cut, sizes on both sides of 1.25"""
    xy2 = np.stack([rng.uniform(0, br.W_PX, nt), rng.uniform(0, br.H_PX, nt)], 1).astype(np.float32)
    idx = np.stack([rng.permutation(nt)[:3] if nt >= 3 else np.concatenate([rng.permutation(nt), [-1]])
                    for _ in range(nq)]).astype(np.int32)
    d2 = np.sort(rng.integers(1, 120000, (nq, 3)), axis=1).astype(np.int32)
    near = rng.uniform(size=nq) < 0.6                           # all three within the ratio
    d2[near, 1] = d2[near, 0] + rng.integers(0, 200, near.sum())
    d2[near, 2] = d2[near, 1] + rng.integers(0, 200, near.sum())
    d2[rng.uniform(size=nq) < 0.05, 1] = 84100
    d2[rng.uniform(size=nq) < 0.05, 1] = 84099
    d2 = np.sort(d2, axis=1)
    if nt < 3:
        d2[:, 2] = br.D2_NONE
    centres = np.array([[400, 150], [-300, 20], [300, -20], [0, 0], [3616, 0], [20, 5]], np.float64)
    v = centres[rng.integers(0, len(centres), nq)] + rng.uniform(-40, 40, (nq, 2))
    wild = rng.uniform(size=nq) < 0.3
    v[wild] = np.stack([rng.uniform(-4000, 4000, wild.sum()), rng.uniform(-3000, 3000, wild.sum())], 1)
    xy1 = (xy2[np.maximum(idx[:, 0], 0)].astype(np.float64) - v).astype(np.float32)
    size1 = (np.round(rng.uniform(2.0, 3.2, nq) * 64) / 64).astype(np.float32)
    size2 = (np.round(rng.uniform(2.0, 3.2, nt) * 64) / 64).astype(np.float32)
    if mode == 'no choice':                                     # every nearest neighbour at 290 or past it
        d2 = np.sort(84100 + rng.integers(0, 1000, (nq, 3)), axis=1).astype(np.int32)
    if mode == 'sizes':                                         # every neighbour fails the size test
        size1[:], size2[:] = 2.0, 2.5 + 1.0 / 64
    return dict(xy1=xy1, xy2=xy2, size1=size1, size2=size2), (idx, d2)


@functools.lru_cache(maxsize=None)
def _size_sweep():
    rng = np.random.default_rng(77)
    made = [_random_pair(rng, nq, nt) for nq in (2, 3, 63, 64, 65, 255, 256, 257, 513) for nt in (2, 3, 513)]
    # the chunk of rows the fill kernel keeps in LDS is 2048 rows: either side of it, and three chunks
    made += [_random_pair(rng, nq, 513) for nq in (2047, 2048, 2049, 4100)]
    made += [_random_pair(rng, 300, 513, 'no choice'), _random_pair(rng, 300, 513, 'sizes')]
    pairs, top3 = [m[0] for m in made], [m[1] for m in made]
    want = [br.bins(t[0], t[1], p['xy1'], p['xy2'], p['size1'], p['size2'], br.MATCH_RATIO, 4, br.STEP_D)
            for p, t in zip(pairs, top3)]
    return pairs, top3, want


def test_bins_every_size_in_one_launch():
    """query images of 2 .. 513 rows against train images of 2, 3 and 513 rows, the chunk edges, a pair
    without a choice and a pair every neighbour of which fails the size test: one launch, by equality"""
    pairs, top3, want = _size_sweep()
    got = run_bins(pairs, top3, 4)
    assert got['flag'].tolist() == [0, 0]
    for k, w in enumerate(want):
        check_bins(got, k, w)
    assert not want[-1]['bin_cnt'].any() and not want[-2]['bin_cnt'].any()
    assert sum(int((w['seg_cnt'] > 0).sum()) for w in want) > 200          # (cells do fill up)
    assert any(w['bin_cnt'][40 * br.NA:].any() for w in want) and any(w['bin_cnt'][:br.NA].any() for w in want)


# ---------------------------------------------------------------------------------------------
# iamx_brute_select
# ---------------------------------------------------------------------------------------------
def _hand_pair(rng, cells, n_q=120, n_t=400, dup=()):
    """a pair from a list of (cell, members, fitted, status): query rows ascend within a cell, the
    first `fitted` members in a seeded choice carry the mask.  dup: query rows moved onto row 0's pixel"""
    xy1 = np.stack([rng.uniform(0, 4000, n_q), rng.uniform(0, 3000, n_q)], 1).astype(np.float32)
    xy2 = np.stack([rng.uniform(0, 4000, n_t), rng.uniform(0, 3000, n_t)], 1).astype(np.float32)
    for q in dup:
        xy1[q] = xy1[0]
    seg_cnt, vstatus = np.zeros(NC, np.int32), np.zeros(NC, np.int32)
    rows, mask = [], []
    for cell, members, fitted, status in sorted(cells):
        seg_cnt[cell], vstatus[cell] = members, status
        q = np.sort(rng.choice(n_q, members, replace=False))
        rows.append(np.stack([q, rng.choice(n_t, members, replace=False)], 1))
        m = np.zeros(members, np.uint8)
        m[rng.choice(members, fitted, replace=False)] = 1 + rng.integers(0, 200)   # (any non-zero byte)
        mask.append(m)
    return (dict(xy1=xy1, xy2=xy2), seg_cnt, np.concatenate(rows + [np.zeros((0, 2), np.int64)]),
            np.concatenate(mask + [np.zeros(0, np.uint8)]), vstatus)


def test_select_walks_hand_made_masks():
    """every branch of the walk with no consensus in between: the early exit firing at (51, 9) and on a
    distance bin without a looked-at cell, not firing at best 50 nor at best_of_bin 10, a strictly
    larger fit needed, a status other than OK, an all-zero mask, a list that de-duplication drops
    below min_pairs, no cell at all"""
    rng = np.random.default_rng(3)
    c = lambda d, a: d * br.NA + a
    specs = [
        [(c(1, 3), 60, 51, 0), (c(2, 0), 30, 9, 0), (c(5, 5), 90, 80, 0)],        # fires after bin 2: 51 kept
        [(c(1, 3), 60, 50, 0), (c(2, 0), 30, 9, 0), (c(5, 5), 90, 80, 0)],        # best 50: on to the 80
        [(c(1, 3), 60, 51, 0), (c(2, 0), 30, 10, 0), (c(3, 20), 90, 80, 0)],      # best_of_bin 10: on to the 80
        [(c(0, 0), 60, 51, 0), (c(2, 7), 90, 80, 0)],                             # bin 1 has nothing: fires there
        [(c(4, 4), 40, 30, 0), (c(4, 5), 40, 30, 0), (c(9, 1), 40, 31, 0)],       # equal fit: the first stays; 31 wins
        [(c(3, 3), 70, 70, 2), (c(3, 4), 50, 0, 0), (c(6, 6), 40, 26, 0)],        # no model; an all-zero mask
        [(c(7, 7), 40, 24, 0)],                                                   # fitted 24 < 25
        [],
        [(c(40, 20), 100, 100, 0), (c(0, 0), 4, 4, 0)],                           # the last cell of all
    ]
    made = [_hand_pair(rng, s) for s in specs]
    # fitted 26 >= 25, two of them on one pixel: unique 25 stays; four on one pixel: 23 < 25 empties it
    for dups in ((1,), (1, 2, 3)):
        pr, sc, rw, mk, vs = _hand_pair(rng, [(c(2, 2), 26, 26, 0)], n_q=26, dup=dups)
        made.append((pr, sc, rw, mk, vs))
    pairs = [m[0] for m in made]
    got = run_select(pairs, np.stack([m[1] for m in made]), np.concatenate([m[2] for m in made]),
                     np.concatenate([m[3] for m in made]), np.stack([m[4] for m in made]), 25, 120)
    for p, (pr, sc, rw, mk, vs) in enumerate(made):
        want = br.select(sc, rw, mk, vs, pr['xy1'], pr['xy2'], 25)
        assert got['chosen'][p] == want['chosen'], p
        assert got['stats'][p].tolist() == want['stats'].tolist(), (p, got['stats'][p], want['stats'])
        assert np.array_equal(got['fit_cnt'][p], want['fit_cnt']), p
        assert np.array_equal(got['lists'][p], want['fwd']), p
    st = got['stats']
    assert st[0].tolist() == [51, 51, 3, 2] and st[1, 0] == 80 and st[2, 0] == 80 and st[3].tolist() == [51, 51, 2, 1]
    assert got['chosen'][4] == c(9, 1) and got['fit_cnt'][4, c(4, 5)] == 30
    assert got['fit_cnt'][5, c(3, 3)] == 0 and got['fit_cnt'][5, c(3, 4)] == 0 and got['chosen'][5] == c(6, 6)
    assert st[6].tolist() == [24, -1, 41, 1] and not len(got['lists'][6]) and got['chosen'][6] == c(7, 7)
    assert st[7].tolist() == [0, -1, 41, 0] and got['chosen'][7] == -1
    assert got['chosen'][8] == c(40, 20) and st[8, 2] == 41
    assert st[9].tolist()[:2] == [26, 25] and len(got['lists'][9]) == 25
    assert st[10].tolist()[:2] == [26, 23] and len(got['lists'][10]) == 0
    assert got['fit_cnt'][0, c(5, 5)] == -1                                      # not reached


def test_select_random_masks():
    rng = np.random.default_rng(11)
    made = []
    for _ in range(24):
        cells = [(int(cl), int(rng.integers(4, 70)), 0, int(rng.uniform() < 0.1) * 2)
                 for cl in rng.choice(NC, 30, replace=False)]
        cells = [(cl, n, int(rng.integers(0, n + 1)), s) for cl, n, _f, s in cells]
        made.append(_hand_pair(rng, cells, n_q=70, n_t=300, dup=(5, 9, 11)))
    got = run_select([m[0] for m in made], np.stack([m[1] for m in made]), np.concatenate([m[2] for m in made]),
                     np.concatenate([m[3] for m in made]), np.stack([m[4] for m in made]), 10, 70)
    for p, (pr, sc, rw, mk, vs) in enumerate(made):
        want = br.select(sc, rw, mk, vs, pr['xy1'], pr['xy2'], 10)
        assert got['chosen'][p] == want['chosen'] and got['stats'][p].tolist() == want['stats'].tolist(), p
        assert np.array_equal(got['fit_cnt'][p], want['fit_cnt']) and np.array_equal(got['lists'][p], want['fwd']), p


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def _arena(pairs):
    """(store, slots [P, 2], kp_off, xy, size, key2) of a list of case pairs, two images each"""
    import torch
    from imageanalysis_amd import kernels, matcher
    dev = _device()
    empty = np.zeros((0, 128), np.uint8)
    store = kernels.DescriptorStore.from_arrays([empty if a is None else a for p in pairs for a in (p['des1'], p['des2'])])
    images = [a for p in pairs for a in (p['xy1'], p['xy2'])]
    kp_off = np.zeros(len(images), np.int64)
    np.cumsum([len(x) for x in images[:-1]], out=kp_off[1:])
    xy = np.ascontiguousarray(np.concatenate(images), np.float32)
    size = np.concatenate([a for p in pairs for a in (p['size1'], p['size2'])]).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return store, np.arange(len(images)).reshape(-1, 2), up(kp_off), up(xy), up(size), up(matcher.kp_key2(xy))


def _check_golden_pair(where, fwd, chosen, stats, fit_cnt, bin_cnt, want):
    """one pair's device figures against what the reference's function did"""
    assert np.array_equal(fwd, want['fwd']), where
    cells = [int(c) for c in np.nonzero(fit_cnt >= 0)[0]]                     # in walk order
    assert [(int(bin_cnt[c]), int(fit_cnt[c])) for c in cells] == want['calls'], where
    assert chosen == (cells[want['taken'][-1]] if want['taken'] else -1), where
    assert stats[0] == (want['filtered'][-1][1] if want['filtered'] else 0), where
    assert stats[2] == len(want['lines']) and stats[3] == len(want['calls']), where


def test_brute_pairs_equals_every_golden():
    """kernels.brute_pairs on the goldens' own inputs: the reference's lists, every cell it handed to
    findHomography with the fitted count, the cells it took, the bins it walked"""
    from imageanalysis_amd import kernels
    for name in br.PAIR_CASES + ('guards',):
        g = br.load_golden(name)
        for min_pairs in sorted(set(p['min_pairs'] for p in g['pairs'])):
            sel = [k for k, p in enumerate(g['pairs']) if p['min_pairs'] == min_pairs]
            store, slots, kp_off, xy, size, key2 = _arena([g['pairs'][k] for k in sel])
            r = kernels.brute_pairs(store, slots, kp_off, xy, size, key2, g['tol'], min_pairs, g['match_ratio'],
                                    g['step_d'], g['hypotheses'], g['seed'])
            assert r.flag.tolist() == [0, 0]
            off, rows = r.off.cpu().numpy(), r.rows.cpu().numpy()
            chosen, stats = r.chosen.cpu().numpy(), r.stats.cpu().numpy()
            fit_cnt, bin_cnt = r.fit_cnt.cpu().numpy(), r.bin_cnt.cpu().numpy()
            for p, k in enumerate(sel):
                want = g['results'][k]
                if name == 'guards':
                    assert off[p] == off[p + 1] and chosen[p] == -1 and (fit_cnt[p] == -1).all(), (name, k)
                    continue
                _check_golden_pair((name, k), rows[off[p]:off[p + 1]], chosen[p], stats[p], fit_cnt[p], bin_cnt[p], want)


def test_brute_pairs_raises_the_flag_of_the_zero_case():
    from imageanalysis_amd import kernels
    g = br.load_golden('zero')
    store, slots, kp_off, xy, size, key2 = _arena(g['pairs'])
    r = kernels.brute_pairs(store, slots, kp_off, xy, size, key2, g['tol'], 3, g['match_ratio'], g['step_d'],
                            g['hypotheses'], g['seed'])
    assert r.flag.tolist() == [1, 0]


def test_launch_splitting_changes_nothing():
    """one launch and launches split by a small batch_bytes: identical results, field by field"""
    from imageanalysis_amd import kernels
    pairs = [p for name in ('clean', 'choice', 'cuts', 'dists', 'dups', 'gates', 'guards') for p in br.case(name)['pairs']]
    store, slots, kp_off, xy, size, key2 = _arena(pairs)
    run = lambda bb: kernels.brute_pairs(store, slots, kp_off, xy, size, key2, br.TOL, 25, br.MATCH_RATIO, br.STEP_D,
                                         br.HYPOTHESES, br.SEED, batch_bytes=bb)
    one, many = run(1 << 40), run(kernels.brute_bytes([400, 100]))
    assert many.slots is None                                   # (several launches: no common slot layout)
    for field in ('off', 'cnt', 'chosen', 'stats', 'fit_cnt', 'bin_cnt', 'flag'):
        assert np.array_equal(getattr(one, field).cpu().numpy(), getattr(many, field).cpu().numpy()), field
    total = int(one.off[-1])
    assert total > 400 and np.array_equal(one.rows[:total].cpu().numpy(), many.rows[:total].cpu().numpy())
    assert len(one.cnt) == len(pairs) and int((one.cnt > 0).sum()) >= 5


class _Kp(object):
    __slots__ = ('pt', 'size')

    def __init__(self, x, y, s):
        self.pt, self.size = (float(x), float(y)), float(s)


class _Image(object):
    def __init__(self, name, des, xy, size):
        self.name = name
        self.des_list = None if des is None else np.asarray(des).astype(np.float32)
        self.kp_list = [_Kp(x, y, s) for (x, y), s in zip(np.asarray(xy, np.float32), np.asarray(size, np.float32))]
        self.match_list = {}


@pytest.fixture
def fresh_matcher():
    from imageanalysis_amd import matcher
    from imageanalysis_amd.hostlib import camera
    saved = {n: getattr(matcher, n) for n in ('the_matcher', 'max_distance', 'min_pairs')}
    size = camera.get_image_params()
    yield matcher
    for n, v in saved.items():
        setattr(matcher, n, v)
    camera.set_image_params(*size)


@pytest.mark.parametrize('name', br.ALL_CASES)
def test_bruteforce_pair_matches_equals_the_reference_function(fresh_matcher, name, monkeypatch):
    """matcher.bruteforce_pair_matches -- guards, the k = 3 search, cells, consensus and walk on the
    device -- against the golden of the reference's own function, and the lines it logs against the
    lines the reference printed"""
    from imageanalysis_amd import _deps
    from imageanalysis_amd.hostlib import camera
    matcher = fresh_matcher
    g = br.load_golden(name)
    said = []

    class Log(object):
        def log(self, *a):
            said.append(' '.join(str(x) for x in a))
        qlog = log
    monkeypatch.setattr(_deps, 'logger', lambda: Log())
    for k, (p, want) in enumerate(zip(g['pairs'], g['results'])):
        camera.set_image_params(int(g['width']), int(g['height']))
        matcher.detector_node.setString('detector', 'SIFT')
        matcher.detector_node.setFloat('scale', 0.4)
        matcher.matcher_node.setFloat('match_ratio', g['match_ratio'])
        matcher.matcher_node.setInt('min_pairs', int(p['min_pairs']))
        matcher.the_matcher = None
        matcher.configure()
        i1, i2 = _Image('A', p['des1'], p['xy1'], p['size1']), _Image('B', p['des2'], p['xy2'], p['size2'])
        del said[:]
        if want['raised']:
            with pytest.raises(ZeroDivisionError):
                matcher.bruteforce_pair_matches(i1, i2, hypotheses=g['hypotheses'], seed=g['seed'])
            continue
        fwd, rev = matcher.bruteforce_pair_matches(i1, i2, hypotheses=g['hypotheses'], seed=g['seed'])
        assert np.array_equal(np.asarray(fwd, np.int32).reshape(-1, 2), want['fwd']), (name, k)
        assert np.array_equal(np.asarray(rev, np.int32).reshape(-1, 2), want['rev']), (name, k)
        if name == 'guards':
            assert matcher.brute_last is None
            continue
        last = matcher.brute_last
        cells = [int(c) for c in np.nonzero(last['fit_cnt'] >= 0)[0]]
        assert [int(last['fit_cnt'][c]) for c in cells] == [f for _n, f in want['calls']], (name, k)
        assert last['chosen'] == (cells[want['taken'][-1]] if want['taken'] else -1), (name, k)
        assert last['stats'][2] == len(want['lines'])
        second = [s for s in said if s.startswith('bin:') and len(s.split()) == 6]
        assert second == ['bin: %d len: %d %d %d' % l[1:] for l in want['lines']], (name, k)
        assert [s for s in said if s.startswith('Filtered')] == \
            ['Filtered matches: %d Fitted matches: %d' % f for f in want['filtered']], (name, k)
        assert [s for s in said if 'initial matches' in s] == \
            (['  initial matches = %d' % len(want['fwd'])] if len(want['fwd']) else []), (name, k)


def _strip_project():
    """the project of find_matches_strip.pkl with the keypoint sizes and the ground of brute_strip"""
    import os
    import pickle
    from conftest import GOLDEN
    from imageanalysis_amd import matcher, smart
    from imageanalysis_amd.hostlib import camera
    import test_find_matches_loop as loop
    with open(os.path.join(GOLDEN, 'find_matches_strip.pkl'), 'rb') as f:
        g = pickle.load(f)
    s = br.load_golden('strip')
    proj = loop.make_project(g, True)
    camera.set_dist_coeffs([0.0, 0.0, 0.0, 0.0, 0.0])
    matcher.matcher_node.__dict__.pop('ground_m', None)
    for im, des, xy, size in zip(proj.image_list, g['des'], g['xy'], s['sizes']):
        im.des_list = np.asarray(des).astype(np.float32)
        im.kp_list = [_Kp(x, y, z) for (x, y), z in zip(np.asarray(xy, np.float32), size)]
        smart.smart_node.getChild(im.name, True).setFloat('srtm_surface_m', s['srtm_surface_m'])
    return g, s, proj, loop


@pytest.mark.parametrize('rounds', ['one', 'many'])
@pytest.mark.parametrize('sort', [False, True])
def test_bruteforce_matches_equals_the_reference_loop(fresh_matcher, sort, rounds, monkeypatch):
    """the shipped pair loop end to end, nothing replaced: against the reference's
    find_matches(strategy='bruteforce') on the strip, and a second call on the same project; in one
    round and in rounds of seven pairs (the pose feedback crosses round boundaries)"""
    from imageanalysis_amd import kernels
    matcher = fresh_matcher
    g, s, proj, loop = _strip_project()
    monkeypatch.setattr(matcher, 'BRUTE_HYPOTHESES', s['hypotheses'])
    if rounds == 'many':
        rows = max(len(x) for x in g['xy'])
        monkeypatch.setattr(matcher, 'BRUTE_BATCH_BYTES', 7 * kernels.brute_bytes([rows]) + 1)
        assert matcher._strategy_pairs_per_batch('bruteforce', rows) == 7
    for call in range(2):
        matcher.bruteforce_matches(proj, None, sort=sort)
        loop.check_against(g, s['runs'][sort], call, proj)
