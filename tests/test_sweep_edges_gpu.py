"""GPU: the form-2 sweep at the edges of its chunk pipeline.  The stage of chunk + 2 and the merge of
the previous chunk ride in the gaps behind the chunk's barrier; what can go wrong there goes wrong
where the pipeline fills and drains: streamed (A) images of exactly 2, 3 and 4 chunks (256, 257, 384
and 385 rows), against register-resident (B) images of 1024 and 1025 rows (one workgroup, and a second
one with a single row).

* the one-pair kernel's `col`, `rowp` and `colmask` equal the numpy model of test_sweep_raw_gpu.py bit
  for bit;
* the item kernel writes what the one-pair kernel writes, for items of 4 pairs that cross a change
  of the B image, with the A image growing across the change in one item and shrinking in the other;
* 16 launches of either kernel, each into a workspace refilled with 0xFF, write the same bytes: a
  stage that lands before another wave's last read of the buffer would show as a difference."""
import numpy as np
import pytest

from test_sweep_raw_gpu import _model, _rows

pytestmark = pytest.mark.gpu

A_SIZES = (256, 257, 384, 385)
B_SIZES = (1024, 1025)
LAUNCHES = 16
# the A images of the four B images of one size, by index into A_SIZES: items of 4 pairs are (a, a, b, b)
# and (c, c, d, d) -- across the change of B the A image shrinks (385 -> 257) and grows (256 -> 384)
A_OF_B = ((0, 3), (1, 2), (3, 0), (2, 1))


@pytest.fixture(scope='module')
def setup():
    import torch
    from imageanalysis_amd import kernels
    rng = np.random.default_rng(131)
    b_imgs = [_rows(rng, n) for n in B_SIZES for _ in A_OF_B]
    a_imgs = [_rows(rng, n) for n in A_SIZES]
    imgs = b_imgs + a_imgs
    store = kernels.DescriptorStore.from_arrays(imgs)
    counts = np.asarray(store.counts, np.int64)
    caps = np.asarray(store.caps3, np.int64)
    na0 = len(b_imgs)
    up = np.array([(b, na0 + a) for b in range(na0) for a in A_OF_B[b % len(A_OF_B)]], np.int32)    # sorted by B
    nwg = (counts[up[:, 0]] + 1023) // 1024
    wg = np.concatenate([[0], np.cumsum(nwg)])
    col_off = np.concatenate([[0], np.cumsum(caps[up[:, 0]])])
    rowp_off = np.concatenate([[0], np.cumsum(nwg * caps[up[:, 1]])])
    items = kernels.sym_items(up, counts, 4)
    # every item holds 4 pairs of two B images
    for f, c, _ in items:
        assert c == 4 and len(set(up[f:f + c, 0])) == 2
    dev = torch.device('cuda')
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    s = dict(store=store, imgs=imgs, up=up, col_off=col_off, rowp_off=rowp_off, d_up=t(up, torch.int32),
             d_wg=t(wg, torch.int32), d_items=t(items, torch.int32), n_items=len(items),
             d_col_off=t(col_off[:-1], torch.int64), d_rowp_off=t(rowp_off[:-1], torch.int64),
             total_wg=int(wg[-1]))
    s['one'] = _launches(s, False)
    s['items'] = _launches(s, True)
    return s


def _launches(s, items):
    """LAUNCHES launches into a workspace refilled with 0xFF: the first launch's (col, rowp, colmask) as
    numpy arrays, and whether every later launch wrote the same bytes"""
    import torch
    from imageanalysis_amd import kernels
    from imageanalysis_amd._lib import check, lib, stream_ptr
    dev, p, st = torch.device('cuda'), kernels._ptr, s['store']
    col = torch.empty((int(s['col_off'][-1]), 2), dtype=torch.int32, device=dev)
    rowp = torch.empty((int(s['rowp_off'][-1]), 2), dtype=torch.int32, device=dev)
    colmask = torch.empty((int(s['col_off'][-1]),), dtype=torch.uint8, device=dev)
    first, same = None, []
    for _ in range(LAUNCHES):
        col.fill_(-1)
        rowp.fill_(-1)
        colmask.fill_(0xFF)
        if items:
            check(lib().iamx_knn2sym_sweep_items(p(st.desc3), p(st.sn2), p(st.sct), p(st.img_off3), p(st.img_n),
                                                 p(s['d_up']), p(s['d_items']), p(s['d_col_off']), p(s['d_rowp_off']),
                                                 len(s['up']), s['n_items'], p(col), p(rowp), p(colmask),
                                                 stream_ptr()), 'iamx_knn2sym_sweep_items')
        else:
            check(lib().iamx_knn2sym_sweep(p(st.desc3), p(st.sn2), p(st.sct), p(st.img_off3), p(st.img_n),
                                           p(s['d_up']), p(s['d_wg']), p(s['d_col_off']), p(s['d_rowp_off']),
                                           len(s['up']), s['total_wg'], 2, p(col), p(rowp), p(colmask),
                                           stream_ptr()), 'iamx_knn2sym_sweep')
        if first is None:
            first = (col.clone(), rowp.clone(), colmask.clone())
        else:
            same.append(all(bool(torch.equal(a, b)) for a, b in zip(first, (col, rowp, colmask))))
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in first), same


def test_one_pair_sweep_equals_numpy_at_2_3_4_chunks(setup):
    s = setup
    (col, rowp, colmask), _ = s['one']
    seen = set()
    for u, (bi, ai) in enumerate(s['up']):
        xa, xb = s['imgs'][ai], s['imgs'][bi]
        mcol, mmask, mrowp, _nwg, _cap = _model(xa, xb, 2)
        nb, c0, r0, r1 = len(xb), s['col_off'][u], s['rowp_off'][u], s['rowp_off'][u + 1]
        what = 'A %d rows, B %d rows' % (len(xa), nb)
        seen.add((len(xa), nb))
        assert r1 - r0 == len(mrowp), what
        np.testing.assert_array_equal(col[c0:c0 + nb], mcol, err_msg='col ' + what)
        np.testing.assert_array_equal(colmask[c0:c0 + nb], mmask, err_msg='colmask ' + what)
        np.testing.assert_array_equal(rowp[r0:r1], mrowp, err_msg='rowp ' + what)
    assert seen == {(a, b) for a in A_SIZES for b in B_SIZES}


def test_item_sweep_equals_one_pair_sweep_across_b_changes(setup):
    s = setup
    na = np.array([len(s['imgs'][a]) for a in s['up'][:, 1]])
    steps = {(int(na[i]), int(na[i + 1])) for i in range(len(na) - 1) if s['up'][i, 0] != s['up'][i + 1, 0] and i % 4 == 1}
    assert {(385, 257), (256, 384)} <= steps, steps          # inside an item, A shrinks and grows across the change of B
    for name, a, b in zip(('col', 'rowp', 'colmask'), s['one'][0], s['items'][0]):
        np.testing.assert_array_equal(b, a, err_msg=name)


@pytest.mark.parametrize('kernel', ['one', 'items'])
def test_repeated_launches_write_the_same_bytes(setup, kernel):
    same = setup[kernel][1]
    assert len(same) == LAUNCHES - 1 and all(same), same
