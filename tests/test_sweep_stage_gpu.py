"""The form-2 sweep's LDS stages, on inputs where a stage read too early or a piece written to the wrong
slot must show: `col`, `colmask` and `rowp` of the one-pair kernel and of the item kernel, through the
C ABI, bit for bit against the numpy model of tests/test_sweep_raw_gpu.py.

The streamed (A) rows come in value bands.  Sorted row p of an A image (the store sorts by n2) has every
element in {-(b + 1), -b} around the offset, b = p // 32: band b's n2 lies in [128 b^2, 128 (b + 1)^2], so
the sorted image holds band b in rows 32 b .. 32 b + 31 -- every 128-row chunk its own four bands, every
quarter of a chunk (the rows one stage piece of the workgroup carries) its own band, and Ct = sct
distinct from chunk to chunk.  A chunk or a piece that reaches the MFMAs from the wrong stage, or a
Ct piece from the wrong chunk, moves every distance of its rows by far more than the band's width.
The CPU test asserts that on the model alone: neighbouring pieces and chunks have different row
partials in more than nine rows of ten, and no two chunks share a Ct value.

A images of 128, 256, 384, 641 and 4096 rows (1, 2, 3, 5 + one ragged row and 32 chunks), B images of
1024 and 1025 rows (one workgroup; two, the second with one valid row), and items of four pairs whose
A image changes with every pair and whose B image changes once.  Eight launches into one workspace
first filled with 0x5A must leave the same bytes."""
import numpy as np
import pytest

from test_sweep_raw_gpu import _model, _rows, _sorted

A_SIZES = (128, 256, 384, 641, 4096)
B_SIZES = (1024, 1024, 1025, 1025)            # two images of each size: an item's B image changes once
LAUNCHES = 8


def _band_rows(rng, n):
    b = np.arange(n) // 32
    s = -(b[:, None] + rng.integers(0, 2, size=(n, 128)))
    return rng.permutation((s + 128).astype(np.uint8))          # (any order: the store sorts)


@pytest.fixture(scope='module')
def images():
    rng = np.random.default_rng(160)
    return [_rows(rng, n) for n in B_SIZES] + [_band_rows(rng, n) for n in A_SIZES]


@pytest.fixture(scope='module')
def models(images):
    cache = {}

    def get(bi, ai):
        if (bi, ai) not in cache:
            cache[bi, ai] = _model(images[ai], images[bi], 2)
        return cache[bi, ai]
    return get


def test_model_separates_bands(images, models):
    nbi = len(B_SIZES)
    for ai, na in enumerate(A_SIZES):
        s, n2, _ = _sorted(images[nbi + ai])
        band = np.arange(na) // 32
        assert (s.min(1) >= -(band + 1)).all() and (s.max(1) <= -band).all()       # the sorted rows are the bands
        ct = (n2 + 2 * s.sum(1)) >> 1
        chunks = [set(ct[c:c + 128].tolist()) for c in range(0, na, 128)]
        for i in range(len(chunks)):
            for j in range(i + 1, len(chunks)):
                assert not (chunks[i] & chunks[j]), (na, i, j)
        for bi in (0, 2):
            rowp = models(bi, nbi + ai)[2]
            L = rowp[:models(bi, nbi + ai)[4], 0]                  # the first workgroup's lower bounds
            full = na // 32 * 32
            pieces = L[:full].reshape(-1, 32)
            # a piece or a chunk swapped with its neighbour changes most rows of both
            assert ((pieces[1:] != pieces[:-1]).mean(axis=1) > 0.9).all(), (na, bi)
            if full >= 256:
                ch = L[:full // 128 * 128].reshape(-1, 128)
                assert ((ch[1:] != ch[:-1]).mean(axis=1) > 0.9).all(), (na, bi)


def _tables(store, up):
    counts = np.asarray(store.counts, np.int64)
    caps = np.asarray(store.caps3, np.int64)
    nwg = (counts[up[:, 0]] + 1023) // 1024
    wg = np.concatenate([[0], np.cumsum(nwg)])
    col_off = np.concatenate([[0], np.cumsum(caps[up[:, 0]])])
    rowp_off = np.concatenate([[0], np.cumsum(nwg * caps[up[:, 1]])])
    return counts, wg, col_off, rowp_off


def _run_and_check(images, models, up, items_S):
    import torch
    from imageanalysis_amd import kernels
    from imageanalysis_amd._lib import check, lib, stream_ptr
    store = kernels.DescriptorStore.from_arrays(images)
    up = np.asarray(up, np.int32)
    counts, wg, col_off, rowp_off = _tables(store, up)
    dev = torch.device('cuda')
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    d_up, d_wg = t(up, torch.int32), t(wg, torch.int32)
    d_col_off, d_rowp_off = t(col_off[:-1], torch.int64), t(rowp_off[:-1], torch.int64)
    col = torch.full((int(col_off[-1]), 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    rowp = torch.full((int(rowp_off[-1]), 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    colmask = torch.full((int(col_off[-1]),), 0x5A, dtype=torch.uint8, device=dev)
    p = kernels._ptr
    if items_S:
        items = kernels.sym_items(up, counts, items_S)
        d_items = t(items, torch.int32)
    first = None
    for launch in range(LAUNCHES):
        if items_S:
            check(lib().iamx_knn2sym_sweep_items(p(store.desc3), p(store.sn2), p(store.sct), p(store.img_off3),
                                                 p(store.img_n), p(d_up), p(d_items), p(d_col_off), p(d_rowp_off),
                                                 len(up), len(items), p(col), p(rowp), p(colmask), stream_ptr()),
                  'iamx_knn2sym_sweep_items')
        else:
            check(lib().iamx_knn2sym_sweep(p(store.desc3), p(store.sn2), p(store.sct), p(store.img_off3),
                                           p(store.img_n), p(d_up), p(d_wg), p(d_col_off), p(d_rowp_off), len(up),
                                           int(wg[-1]), 2, p(col), p(rowp), p(colmask), stream_ptr()),
                  'iamx_knn2sym_sweep')
        torch.cuda.synchronize()
        out = (col.cpu().numpy(), rowp.cpu().numpy(), colmask.cpu().numpy())
        if first is None:
            first = out
        else:
            for name, a, b in zip(('col', 'rowp', 'colmask'), first, out):
                np.testing.assert_array_equal(b, a, err_msg='%s, launch %d against launch 0' % (name, launch))
    col, rowp, colmask = first
    for u, (bi, ai) in enumerate(up):
        mcol, mmask, mrowp, _nwg, _cap = models(int(bi), int(ai))
        nb = len(images[bi])
        what = 'A %d rows, B %d rows (pair %d)' % (len(images[ai]), nb, u)
        np.testing.assert_array_equal(col[col_off[u]:col_off[u] + nb], mcol, err_msg='col ' + what)
        np.testing.assert_array_equal(colmask[col_off[u]:col_off[u] + nb], mmask, err_msg='colmask ' + what)
        np.testing.assert_array_equal(rowp[rowp_off[u]:rowp_off[u + 1]], mrowp, err_msg='rowp ' + what)
    return store, up


@pytest.mark.gpu
def test_one_pair_sweep_on_banded_stages(images, models):
    nbi = len(B_SIZES)
    _run_and_check(images, models, [(bi, nbi + ai) for bi in (0, 2) for ai in range(len(A_SIZES))], 0)


@pytest.mark.gpu
def test_item_sweep_on_banded_stages(images, models):
    from imageanalysis_amd import kernels
    nbi = len(B_SIZES)
    a = lambda i: nbi + i  # noqa: E731
    # (B, A) sorted by B: one item of four pairs on the 1024-row images, one per slice on the 1025-row ones;
    # the A image -- and its chunk count -- changes with every pair, the B image once inside each item
    up = [(0, a(4)), (0, a(0)), (1, a(3)), (1, a(1)),
          (2, a(2)), (2, a(4)), (3, a(0)), (3, a(3))]
    store, up = _run_and_check(images, models, up, 4)
    items = kernels.sym_items(up, np.asarray(store.counts, np.int64), 4)
    assert items.tolist() == [[0, 4, 0], [4, 4, 0], [4, 4, 1]]
