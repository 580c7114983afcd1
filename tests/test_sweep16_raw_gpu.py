"""GPU: the raw outputs of the item sweep on v_mfma_i32_16x16x64_i8 (iamx_knn2sym_sweep_items16) --
`col` (v1, v2), `colmask` and the row partials `rowp` -- bit for bit against the numpy model of
form 2 (test_sweep_raw_gpu._model), at that test's sizes and planted ties: streamed (A) images of 1,
127, 128, 129, 4096 and 5000 rows, register-resident (B) images of 1, 1000, 1024 and 4100 rows.
Items of S = 4 pairs: items that cross a change of B image, and runs of pairs shorter than S.  A
second launch into the refilled workspace writes what the first wrote."""
import numpy as np
import pytest

from test_sweep_raw_gpu import A_SIZES, B_SIZES, _model, _rows, _sorted

pytestmark = pytest.mark.gpu

S = 4


@pytest.fixture(scope='module')
def setup():
    import torch
    from imageanalysis_amd import kernels
    rng = np.random.default_rng(42)
    imgs = [_rows(rng, n) for n in B_SIZES + A_SIZES]
    store = kernels.DescriptorStore.from_arrays(imgs)
    nbi = len(B_SIZES)
    perm = store.sperm.cpu().numpy()
    offs = store.img_off3.cpu().numpy()
    for i, x in enumerate(imgs):               # the store's row order is the model's
        assert (perm[offs[i]:offs[i] + len(x)] == _sorted(x)[2]).all()
    up, col_off, rowp_off, models = [], [0], [0], []
    for bi in range(nbi):                      # (B, A), sorted by B
        for ai in range(len(A_SIZES)):
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
    assert any(c < S for _, c, _ in items), 'no run of pairs shorter than S'
    dev = torch.device('cuda')
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    return dict(store=store, up=up, models=models, col_off=col_off, rowp_off=rowp_off, n_items=len(items),
                d_up=t(up, torch.int32), d_items=t(items, torch.int32),
                d_col_off=t(col_off[:-1], torch.int64), d_rowp_off=t(rowp_off[:-1], torch.int64))


def _workspace(s):
    import torch
    dev = torch.device('cuda')
    return (torch.full((s['col_off'][-1], 2), -7, dtype=torch.int32, device=dev),
            torch.full((s['rowp_off'][-1], 2), -7, dtype=torch.int32, device=dev),
            torch.full((s['col_off'][-1],), 0xEE, dtype=torch.uint8, device=dev))


def _launch(s, ws):
    import torch
    from imageanalysis_amd import kernels
    from imageanalysis_amd._lib import check, lib, stream_ptr
    p, st = kernels._ptr, s['store']
    check(lib().iamx_knn2sym_sweep_items16(p(st.desc3), p(st.sn2), p(st.sct), p(st.img_off3), p(st.img_n),
                                           p(s['d_up']), p(s['d_items']), p(s['d_col_off']), p(s['d_rowp_off']),
                                           len(s['up']), s['n_items'], p(ws[0]), p(ws[1]), p(ws[2]),
                                           stream_ptr()), 'iamx_knn2sym_sweep_items16')
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in ws]


@pytest.fixture(scope='module')
def first(setup):
    ws = _workspace(setup)
    return ws, _launch(setup, ws)


def test_sweep16_raw_outputs_equal_numpy(setup, first):
    s = setup
    col, rowp, colmask = first[1]
    col_off, rowp_off, nbi = s['col_off'], s['rowp_off'], len(B_SIZES)
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


def test_sweep16_second_launch_into_the_refilled_workspace(setup, first):
    ws, out1 = first
    ws[0].fill_(-7)
    ws[1].fill_(-7)
    ws[2].fill_(0xEE)
    out2 = _launch(setup, ws)
    for name, a, b in zip(('col', 'rowp', 'colmask'), out1, out2):
        np.testing.assert_array_equal(b, a, err_msg=name)
