"""GPU: the pair tail of the item sweep on v_mfma_i32_16x16x64_i8 (knn2sym16_kernel) -- the column
epilogue on v_permlane32_swap / v_permlane16_swap, every lane storing four consecutive queries --
through iamx_knn2sym_sweep_items16 as test_sweep16_raw_gpu.py launches it: `col`, `colmask` and
`rowp` bit for bit against the numpy model of form 2 (test_sweep_raw_gpu._model), at the sizes
where the exchanges and the stores can go wrong:

* register-resident (B) images of 1, 15, 16, 17, 31, 33, 255, 256, 257, 1023, 1024, 1025 and 2049
  rows: a partial block of four queries, a partial wave, waves past the end, the slice edge;
* streamed (A) images of 1, 16, 128, 129 and 300 rows: fewer tiles than column groups, so that
  groups stay at the sentinel;
* items of S = 4 pairs that cross a change of B.

Every B image is a prefix of one pool of rows, and the A images hold copies of pool rows (distance
0 to the query that is that row, so the copies are its smallest group minima): 6 copies in the
16-row image, the 128-row image is 128 copies, 40 copies in the 129-row image and 130 in the
300-row one (equal norms are neighbours in the sorted order: 128 of them cover all eight groups).
The test checks on the model's own distances that the planted cases are there: queries with
v1 == v2, equal minima on both sides of the xor-32 merge (train row bit 3) and of the xor-16 merge
(train row bit 2), a query with mask 0xFF.  A second launch into the refilled workspace writes the
same bytes."""
import numpy as np
import pytest

from test_sweep16_raw_gpu import S, _launch, _workspace
from test_sweep_raw_gpu import BIG, _model, _rows, _sorted

pytestmark = pytest.mark.gpu

B_SIZES = (1, 15, 16, 17, 31, 33, 255, 256, 257, 1023, 1024, 1025, 2049)
A_SIZES = (1, 16, 128, 129, 300)


def _images():
    rng = np.random.default_rng(2020)
    pool = _rows(rng, max(B_SIZES))
    bs = [pool[:n].copy() for n in B_SIZES]
    a = [_rows(rng, n) for n in A_SIZES]
    a[1][3:9] = pool[0]
    a[2][:] = pool[0]
    a[3][50:90] = pool[0]
    a[4][100:230] = pool[5]
    a[4][7] = a[4][250]                        # (and a duplicate that is no row of B)
    return bs, a


def _sides(xa, xb):
    """the accumulators' minima per (k, g, train row bit 3) and B row: [4][2][2][nb]"""
    sa, n2a, _ = _sorted(xa)
    sb, n2b, _ = _sorted(xb)
    d2 = n2a[:, None] + n2b[None, :] - 2 * (sa @ sb.T)
    cap = (len(xa) + 127) // 128 * 128
    E = np.full((cap, len(xb)), BIG, np.int64)
    E[:len(xa)] = (d2 - n2b[None, :] - (n2a & 1)[:, None]) // 2
    return E.reshape(cap // 128, 4, 2, 2, 2, 4, len(xb)).min(axis=(0, 2, 5)).transpose(0, 2, 1, 3)


@pytest.fixture(scope='module')
def setup():
    import torch
    from imageanalysis_amd import kernels
    bs, as_ = _images()
    imgs = bs + as_
    store = kernels.DescriptorStore.from_arrays(imgs)
    nbi = len(bs)
    perm = store.sperm.cpu().numpy()
    offs = store.img_off3.cpu().numpy()
    for i, x in enumerate(imgs):               # the store's row order is the model's
        assert (perm[offs[i]:offs[i] + len(x)] == _sorted(x)[2]).all()
    up, col_off, rowp_off, models = [], [0], [0], []
    for bi in range(nbi):                      # (B, A), sorted by B
        for ai in range(len(as_)):
            m = _model(imgs[nbi + ai], imgs[bi], 2)
            models.append(m)
            up.append((bi, nbi + ai))
            col_off.append(col_off[-1] + int(store.caps3[bi]))
            rowp_off.append(rowp_off[-1] + m[3] * m[4])
    up = np.array(up, np.int32)
    counts = np.asarray(store.counts, np.int64)
    items = kernels.sym_items(up, counts, S)
    nb = counts[up[:, 0]]
    assert any(nb[f] != nb[f + c - 1] for f, c, _ in items), 'no item crosses a change of B'
    dev = torch.device('cuda')
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    return dict(store=store, up=up, models=models, col_off=col_off, rowp_off=rowp_off, n_items=len(items),
                imgs=imgs, nbi=nbi,
                d_up=t(up, torch.int32), d_items=t(items, torch.int32),
                d_col_off=t(col_off[:-1], torch.int64), d_rowp_off=t(rowp_off[:-1], torch.int64))


@pytest.fixture(scope='module')
def first(setup):
    ws = _workspace(setup)
    return ws, _launch(setup, ws)


def test_the_planted_cases_are_in_the_model(setup):
    s = setup
    tie12 = tie32 = tie16 = full = 0
    for (bi, ai), (mcol, mmask, _rowp, _nwg, _cap) in zip(s['up'], s['models']):
        if len(s['imgs'][ai]) < 16:
            continue
        sd = _sides(s['imgs'][ai], s['imgs'][bi])              # [k][g][bit 3][b]
        gm = sd.min(axis=2)
        real = mcol[:, 1] < BIG
        tie12 += int((real & (mcol[:, 0] == mcol[:, 1])).sum())
        full += int((real & (mmask == 0xFF)).sum())
        # a group that decides (its minimum is v1) with the same minimum on both sides of the xor-32 merge
        tie32 += int(((sd[:, :, 0] == sd[:, :, 1]) & (gm == mcol[:, 0][None, None, :]) & real[None, None, :]).any(axis=(0, 1)).sum())
        # both halves g hold v1: the xor-16 merge sees a1 == b1
        tie16 += int((real & (gm[:, 0].min(axis=0) == gm[:, 1].min(axis=0))).sum())
    assert tie12 and tie32 and tie16 and full, (tie12, tie32, tie16, full)


def test_sweep16_tail_outputs_equal_numpy(setup, first):
    s = setup
    col, rowp, colmask = first[1]
    col_off, rowp_off, nbi = s['col_off'], s['rowp_off'], s['nbi']
    for u, ((bi, ai), (mcol, mmask, mrowp, _nwg, _cap)) in enumerate(zip(s['up'], s['models'])):
        nb = B_SIZES[bi]
        what = 'A %d rows, B %d rows' % (A_SIZES[ai - nbi], nb)
        np.testing.assert_array_equal(col[col_off[u]:col_off[u] + nb], mcol, err_msg='col ' + what)
        np.testing.assert_array_equal(colmask[col_off[u]:col_off[u] + nb], mmask, err_msg='colmask ' + what)
        np.testing.assert_array_equal(rowp[rowp_off[u]:rowp_off[u + 1]], mrowp, err_msg='rowp ' + what)
        # nothing past the image's rows
        cap = col_off[u + 1] - col_off[u]
        assert (col[col_off[u] + nb:col_off[u] + cap] == -7).all(), 'col past the end, ' + what
        assert (colmask[col_off[u] + nb:col_off[u] + cap] == 0xEE).all(), 'colmask past the end, ' + what


def test_sweep16_tail_second_launch_into_the_refilled_workspace(setup, first):
    ws, out1 = first
    ws[0].fill_(-7)
    ws[1].fill_(-7)
    ws[2].fill_(0xEE)
    out2 = _launch(setup, ws)
    for name, a, b in zip(('col', 'rowp', 'colmask'), out1, out2):
        np.testing.assert_array_equal(b, a, err_msg=name)
