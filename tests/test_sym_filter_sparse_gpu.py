"""GPU: the symmetric filter stage where nearly every pair has no candidate (a survey launch), where
single pairs hold 0, 1, 63, 64, 65 and nearly all of their rows, and on a workspace that the batch
before left dirty.

  * the candidate set of iamx_knn2sym_candidates == the candidate rule restated in numpy from the
    sweep's own outputs (`col`, `rowp`): the merge of (L, U1, U2) over the workgroups, the saturated
    16-bit offsets, the float32 / float64 metric of the bounds -- per ordered pair the count, the
    list (ascending original rows) and the bound left in d2[., 1];
  * the whole stage == oracle/cpu_ref (survivor rows, train rows, metrics, squared distances), with
    the narrow exact stage and without it;
  * a workspace that held a batch full of candidates, then one with hardly any, then the first
    again == a fresh workspace, in one PairWorkspace and in the two of OverlappedSweeps;
  * a launch of unrelated images: every count 0, the flags untouched.

Sizes.  Form 0 (256-row workgroups): images of 2, 31, 33, 255, 257, 1000 and 1300 rows -- odd
sizes, pairs whose slice of the bit map starts and ends inside a word, up to 6 row partials per
row (a one-row image cannot be in a PairBatch: a train image needs two rows, so the smallest is 2).
Form 2 (1024-row workgroups, items of 3 pairs): 4096, 4097 and 4224 rows.  A batch of 4096, 4097 and
1025 rows is swept in form 0 (the form follows the smallest image): up to 17 partials per row, the
loop behind the unrolled four."""
import numpy as np
import pytest

from test_match_sym_gpu import _oracle_survivors, _sift_like

pytestmark = pytest.mark.gpu

THRESH = 270.0 * 0.75
NO_BOUND = 0x7F000000


def _plant(rng, imgs, used, a, b, m, src_first=(), dst_first=()):
    """m noisy copies of rows of image a in image b: m candidates in both directions of the pair.
    Rows already used by a planting are not used again (no chains of copies between other pairs)."""
    def pick(k, first):
        free = np.setdiff1d(np.arange(len(imgs[k])), np.fromiter(used[k], np.int64, len(used[k])))
        first = [r % len(imgs[k]) for r in first]
        assert not set(first) & used[k]
        rest = rng.permutation(np.setdiff1d(free, first))[:m - len(first)]
        rows = np.concatenate([np.asarray(first, np.int64), rest]).astype(np.int64)
        assert len(rows) == m
        used[k].update(rows.tolist())
        return rows
    src, dst = pick(a, src_first), pick(b, dst_first)
    imgs[b][dst] = np.clip(imgs[a][src].astype(int) + rng.integers(-6, 7, (m, 128)), 0, 255)


def _case(name):
    """images and the candidate counts the plantings aim at, per unordered pair"""
    rng = np.random.default_rng({'form0': 11, 'form2': 12, 'mixed': 13, 'dense': 14, 'none': 15}[name])
    if name == 'form0':
        sizes = [2, 31, 33, 255, 257, 1000, 1300]
        plan = [(6, 5, 900, (), ()), (6, 4, 64, (0, -1), (-1,)), (6, 3, 65, (), (0,)),
                (5, 4, 63, (), ()), (4, 3, 1, (0,), (-1,))]
    elif name == 'form2':
        sizes = [4096, 4097, 4224]
        plan = [(0, 1, 65, (0, -1), (0, -1)), (1, 2, 4000, (), ())]
    elif name == 'mixed':
        sizes = [4096, 4097, 1025]
        plan = [(0, 2, 64, (0, -1), (0, -1)), (1, 2, 1, (-1,), (1,)), (0, 1, 63, (), ())]
    elif name == 'dense':
        sizes = [1100, 1300, 1024, 1500]
        plan = [(0, 1, 400, (), ()), (0, 2, 300, (), ()), (0, 3, 300, (), ()), (1, 2, 300, (), ()),
                (1, 3, 400, (), ()), (2, 3, 150, (), ())]
    else:
        sizes = [300, 257, 1000, 640]
        plan = []
    imgs = [_sift_like(rng, n) for n in sizes]
    used = [set() for _ in sizes]
    for a, b, m, sf, df in plan:
        _plant(rng, imgs, used, a, b, m, sf, df)
    want = {(a, b): m for a, b, m, _, _ in plan}
    return imgs, want


def _rule(tab, pairs, counts, caps3, off3, sn2, sperm, col, rowp, thresh):
    """today's candidate rule from the sweep's outputs: per ordered pair (candidate rows in
    ascending original order, their bound for d2[., 1])"""
    out = []
    for p, (qi, _ti) in enumerate(pairs):
        u, role = int(tab['osrc'][p][0]), int(tab['osrc'][p][1])
        n, cap, o = int(counts[qi]), int(caps3[qi]), int(off3[qi])
        n2 = sn2[o:o + n].astype(np.int64)
        par, cq = n2 & 1, n2 >> 1
        if role == 0:
            v = col[tab['col_off'][u]:tab['col_off'][u] + n].astype(np.int64)
            Lb, Ub = 2 * (v[:, 0] + cq) + par, 2 * (v[:, 1] + cq) + par + 1
        else:
            nwg = int(tab['wg'][u + 1] - tab['wg'][u])
            e = rowp[tab['rowp_off'][u]:tab['rowp_off'][u] + nwg * cap].reshape(nwg, cap, 2)[:, :n]
            L = e[..., 0].astype(np.int64)
            pk = e[..., 1].astype(np.int64) & 0xFFFFFFFF
            d1, d2 = pk & 0xFFFF, pk >> 16
            U = np.concatenate([np.where(d1 == 0xFFFF, NO_BOUND, L + d1), np.where(d2 == 0xFFFF, NO_BOUND, L + d2)])
            U2 = np.sort(U, axis=0)[1]                   # (the merge of the sorted pairs (U1, U2))
            Lb, Ub = 2 * L.min(axis=0) + par, 2 * U2 + par + 1
        Lb = np.maximum(Lb, 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            f0 = np.sqrt(Lb.astype(np.float64)).astype(np.float32).astype(np.float64)
            f1 = np.sqrt(Ub.astype(np.float64)).astype(np.float32).astype(np.float64)
            k = (f1 == 0) | (f0 * (f0 / f1) < thresh)
        orig = sperm[o:o + n][k].astype(np.int64)
        order = np.argsort(orig)
        out.append((orig[order], np.minimum(Ub[k], 0x7FFFFFFF)[order]))
    return out


def _all_pairs(n):
    return [(i, j) for i in range(n) for j in range(n) if i != j]


_built = {}


def _setup(name):
    """store, batch and the oracle's survivors of a case, made once"""
    if name not in _built:
        from imageanalysis_amd import kernels
        imgs, want = _case(name)
        store = kernels.DescriptorStore.from_arrays(imgs)
        pairs = _all_pairs(len(imgs))
        oracle = [_oracle_survivors(imgs[i], imgs[j], THRESH) for i, j in pairs]
        _built[name] = (imgs, want, store, pairs, oracle)
    return _built[name]


def _call_candidates(pb, ws, thresh):
    from imageanalysis_amd.kernels import _ptr
    from imageanalysis_amd._lib import check, lib, stream_ptr
    st = pb.store
    check(lib().iamx_knn2sym_candidates(_ptr(st.sn2), _ptr(st.sperm), _ptr(st.img_off3), _ptr(st.img_n),
                                        _ptr(pb.d_pairs), _ptr(pb.d_osrc), _ptr(pb.d_sym_wg),
                                        _ptr(pb.d_col_off), _ptr(pb.d_rowp_off), _ptr(pb.d_out),
                                        _ptr(ws.col), _ptr(ws.rowp), pb.n_pairs, float(thresh),
                                        _ptr(ws.keep), _ptr(ws.seg_count), _ptr(ws.surv_q),
                                        _ptr(ws.task_total), _ptr(ws.tasks), _ptr(ws.d2),
                                        _ptr(ws.colmask), _ptr(ws.nar), ws.max_rows, pb.max_query_rows,
                                        pb.sym_form, stream_ptr()), 'iamx_knn2sym_candidates')


@pytest.mark.parametrize('name,form', [('form0', 0), ('form2', 2), ('mixed', 0)])
def test_candidate_set_equals_the_rule(name, form):
    import torch
    from imageanalysis_amd import kernels
    imgs, want, store, pairs, _ = _setup(name)
    pb = kernels.PairBatch(store, np.asarray(pairs, np.int32), sym=True)
    assert pb.sym_form == form
    ws = kernels.PairWorkspace(pb.rows, pb.n_pairs)
    ws.seg_count.fill_(12345)                            # (the stage clears its own counters)
    ws.keep.fill_(0xFF)
    pb.run_sym_sweep(ws)
    torch.cuda.synchronize()
    tab = kernels.sym_tables(pb.pairs, store.counts, store.caps3)
    assert tab['form'] == form
    rule = _rule(tab, pairs, store.counts, store.caps3, store.img_off3.cpu().numpy(), store.sn2.cpu().numpy(),
                 store.sperm.cpu().numpy(), ws.col.cpu().numpy(), ws.rowp.cpu().numpy(), THRESH)
    _call_candidates(pb, ws, THRESH)
    torch.cuda.synchronize()
    cnt = ws.seg_count[:pb.n_pairs].cpu().numpy()
    cq = ws.surv_q.cpu().numpy()
    d2 = ws.d2.cpu().numpy()
    got = {}
    for p, (i, j) in enumerate(pairs):
        rows, ub = rule[p]
        ob = int(pb.out_off[p])
        print('%s pair %d (%d -> %d): %d candidates of %d rows, first bit %d' % (name, p, i, j, len(rows), len(imgs[i]), ob & 31))
        assert cnt[p] == len(rows), (p, i, j)
        assert np.array_equal(cq[ob:ob + cnt[p]], rows), (p, i, j)
        assert np.array_equal(d2[ob + rows, 1], ub), (p, i, j)
        got[(i, j)] = len(rows)
    # what the plantings aimed at is what the rule found: 0, 1, 63, 64, 65 and nearly all rows
    for (a, b), m in want.items():
        assert got[(a, b)] == m and got[(b, a)] == m, (a, b, m, got[(a, b)], got[(b, a)])
    if name == 'form0':
        assert {0, 1, 63, 64, 65} <= set(got.values())
        assert got[(5, 6)] == 900 and len(imgs[5]) == 1000
        # (a train image of 2, 31 or 33 rows leaves most of the sweep's eight groups empty: no second
        #  bound, every query row is a candidate)
        assert got[(6, 0)] == 1300 and got[(3, 1)] == 255 and got[(4, 2)] == 257
        # the first and the last row of an image as its pair's only candidate
        assert rule[pairs.index((4, 3))][0].tolist() == [0] and rule[pairs.index((3, 4))][0].tolist() == [254]
        assert len({int(pb.out_off[p]) & 31 for p in range(pb.n_pairs)}) > 4      # slices off the word boundaries


def _stage(pb, ws, thresh):
    import torch
    pb.run(ws, thresh)
    torch.cuda.synchronize()
    n = pb.n_pairs
    first, count, q, t, m = ws.survivors(n)
    assert np.array_equal(first, pb.out_off[:n])
    nar = ws.nar[:256 + 4 * n].cpu().numpy()
    return dict(seg=ws.seg_count[:n].cpu().numpy(), cnt=count, q=[q[f:f + c] for f, c in zip(first, count)],
                t=[t[f:f + c] for f, c in zip(first, count)], m=[m[f:f + c] for f, c in zip(first, count)],
                d2=ws.d2[:pb.rows].cpu().numpy(), ctl=nar[:12].view(np.int32), narrow=nar[256:].view(np.int32) >= 0,
                task_total=ws.task_total.cpu().numpy(), flags=ws.flags.cpu().numpy())


def _same_stage(a, b):
    assert np.array_equal(a['seg'], b['seg']) and np.array_equal(a['cnt'], b['cnt'])
    assert np.array_equal(a['narrow'], b['narrow'])
    for k in ('q', 't', 'm'):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k


@pytest.mark.parametrize('name,narrow', [('form0', '1'), ('form2', '1'), ('mixed', '1'), ('form2', '0')],
                         ids=['form0', 'form2', 'mixed', 'form2-full-scan'])
def test_whole_stage_against_the_oracle(name, narrow, monkeypatch):
    from imageanalysis_amd import kernels
    if narrow == '0':
        monkeypatch.setenv('IAMX_EXACT_NARROW', '0')
    imgs, want, store, pairs, oracle = _setup(name)
    pb = kernels.PairBatch(store, np.asarray(pairs, np.int32), sym=True)
    ws = kernels.PairWorkspace(pb.rows, pb.n_pairs)
    r = _stage(pb, ws, THRESH)
    assert not r['ctl'].any() and not r['task_total'].any() and r['flags'][1] == 0
    # (with the narrow stage switched off nobody writes its table of pairs: a fresh workspace's zeros
    #  say nothing; mixed: no pair with more than 64 candidates)
    if narrow == '1':
        assert r['narrow'].any() == (name != 'mixed')
    for p, (i, j) in enumerate(pairs):
        keep, tr, mt, d2, _zd = oracle[p]
        assert np.array_equal(r['q'][p], keep), (i, j)
        assert np.array_equal(r['t'][p], tr), (i, j)
        assert np.array_equal(r['m'][p], mt), (i, j)
        assert np.array_equal(r['d2'][pb.out_off[p] + keep], d2), (i, j)
        assert r['seg'][p] >= len(keep)
    for (a, b), m in want.items():                      # the planted copies survive
        assert r['cnt'][pairs.index((a, b))] >= m * 9 // 10


def _dirty_batches():
    from imageanalysis_amd import kernels
    if 'dirty' not in _built:
        # one store for both batches: the dense images and, behind them, the sparse case's
        nd = len(_case('dense')[0])
        imgs = _case('dense')[0] + _case('none')[0] + _case('form0')[0][3:]
        store = kernels.DescriptorStore.from_arrays(imgs)
        dense = np.asarray(_all_pairs(nd), np.int32)
        sparse = np.asarray(_all_pairs(len(imgs) - nd), np.int32) + nd
        _built['dirty'] = (store, dense, sparse)
    store, dense, sparse = _built['dirty']
    return (kernels.PairBatch(store, dense, sym=True), kernels.PairBatch(store, sparse, sym=True))


def test_dirty_workspace_equals_fresh_one():
    import torch
    from imageanalysis_amd import kernels
    dense, sparse = _dirty_batches()
    rows, np_ = max(dense.rows, sparse.rows), max(dense.n_pairs, sparse.n_pairs)
    fresh = {id(b): _stage(b, kernels.PairWorkspace(rows, np_), THRESH) for b in (dense, sparse)}
    assert fresh[id(dense)]['seg'].min() > 64 and (fresh[id(sparse)]['seg'] == 0).sum() > sparse.n_pairs // 2
    assert fresh[id(dense)]['narrow'].any()
    ws = kernels.PairWorkspace(rows, np_)
    for b in (dense, sparse, dense):
        r = _stage(b, ws, THRESH)
        _same_stage(r, fresh[id(b)])
        assert not r['ctl'].any() and not r['task_total'].any() and r['flags'][1] == 0
    # the two workspaces of the overlapped schedule: each sees dense, sparse, dense
    seq = [dense, dense, sparse, sparse, dense, dense]
    ov = kernels.OverlappedSweeps(rows, np_)
    snaps = []

    def snap(b, w):
        n = b.n_pairs
        snaps.append((b, w.seg_count[:n].clone(), w.surv_cnt[:n].clone(), w.surv_q.clone(), w.surv_t.clone(),
                      w.surv_metric.clone(), w.nar[:256 + 4 * n].clone(), w.task_total.clone()))
    ov.run(seq, THRESH, after_filter=snap)
    torch.cuda.synchronize()
    assert len(snaps) == len(seq)
    for b, seg, cnt, q, t, m, nar, task_total in snaps:
        f = fresh[id(b)]
        nar = nar.cpu().numpy()
        assert np.array_equal(seg.cpu().numpy(), f['seg']) and np.array_equal(cnt.cpu().numpy(), f['cnt'])
        assert not nar[:12].view(np.int32).any() and not task_total.cpu().numpy().any()
        assert np.array_equal(nar[256:].view(np.int32) >= 0, f['narrow'])
        q, t, m = q.cpu().numpy(), t.cpu().numpy(), m.cpu().numpy()
        for p in range(b.n_pairs):
            o, c = int(b.out_off[p]), int(f['cnt'][p])
            assert np.array_equal(q[o:o + c], f['q'][p]) and np.array_equal(t[o:o + c], f['t'][p])
            assert np.array_equal(m[o:o + c], f['m'][p])


def test_launch_without_any_candidate():
    import torch
    from imageanalysis_amd import kernels
    imgs, _, store, pairs, oracle = _setup('none')
    assert all(len(o[0]) == 0 for o in oracle)
    pb = kernels.PairBatch(store, np.asarray(pairs, np.int32), sym=True)
    ws = kernels.PairWorkspace(pb.rows, pb.n_pairs)
    ws.seg_count.fill_(7)
    ws.surv_cnt.fill_(7)
    ws.flags.copy_(torch.tensor([5, 9], dtype=torch.int32))
    r = _stage(pb, ws, THRESH)
    assert not r['seg'].any() and not r['cnt'].any() and not r['narrow'].any()
    assert not r['ctl'].any() and not r['task_total'].any()
    assert r['flags'].tolist() == [5, 9]
