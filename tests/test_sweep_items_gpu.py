"""GPU: the form-2 sweep walking items (iamx_knn2sym_sweep_items) writes exactly what the one-pair
sweep (iamx_knn2sym_sweep, form 2) writes -- col, colmask and rowp bit for bit, and nothing else --
for items of S = 1, 2, 3 and 5 pairs: streamed (A) images of 1, 127, 128, 129, 4096 and 5000 rows
mixed inside one item, register-resident (B) images of 4096, 5000, 4100 and 5001 rows (items that
cross a change of B image between images of the same slice count in both directions: waves of
slice 4 that turn invalid -- they refill their row minima with BIG -- and valid again; slices
whose last waves lie past the end of B)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A_SIZES = (1, 127, 128, 129, 4096, 5000)
B_SIZES = (4096, 5000, 4100, 5001)


def _rows(rng, n):
    g = rng.gamma(0.6, 1.0, size=(n, 128))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    x = np.clip(np.rint(np.minimum(g, 0.2) * 640.0), 0, 255).astype(np.uint8)
    if n > 8:                                  # equal rows and equal norms: ties
        x[n // 2:n // 2 + 3] = x[1]
    return x


@pytest.fixture(scope='module')
def setup():
    import torch
    from imageanalysis_amd import kernels
    rng = np.random.default_rng(81)
    imgs = [_rows(rng, n) for n in B_SIZES + A_SIZES]
    store = kernels.DescriptorStore.from_arrays(imgs)
    nbi = len(B_SIZES)
    counts = np.asarray(store.counts, np.int64)
    caps = np.asarray(store.caps3, np.int64)
    # (B, A), sorted by B; A sizes in a different order for every B
    up = np.array([(b, nbi + a) for b in range(nbi) for a in rng.permutation(len(A_SIZES))], np.int32)
    nwg = (counts[up[:, 0]] + 1023) // 1024
    wg = np.concatenate([[0], np.cumsum(nwg)])
    col_off = np.concatenate([[0], np.cumsum(caps[up[:, 0]])])
    rowp_off = np.concatenate([[0], np.cumsum(nwg * caps[up[:, 1]])])
    dev = torch.device('cuda')
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    return dict(store=store, up=up, counts=counts, d_up=t(up, torch.int32), d_wg=t(wg, torch.int32),
                d_col_off=t(col_off[:-1], torch.int64), d_rowp_off=t(rowp_off[:-1], torch.int64),
                n_col=int(col_off[-1]), n_rowp=int(rowp_off[-1]), total_wg=int(wg[-1]), t=t)


def _outputs(s):
    import torch
    dev = torch.device('cuda')
    return (torch.full((s['n_col'], 2), -7, dtype=torch.int32, device=dev),
            torch.full((s['n_rowp'], 2), -7, dtype=torch.int32, device=dev),
            torch.full((s['n_col'],), 0xEE, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize('S', [1, 2, 3, 5])
def test_item_sweep_equals_one_pair_sweep(setup, S):
    import torch
    from imageanalysis_amd import kernels
    from imageanalysis_amd._lib import check, lib, stream_ptr
    s, p = setup, kernels._ptr
    st = s['store']
    items = kernels.sym_items(s['up'], s['counts'], S)
    if S == 5:        # items that go from 5000 to 4100 rows of B and from 4100 to 5001
        nb = s['counts'][s['up'][:, 0]]
        crossings = {(int(nb[f]), int(nb[f + c - 1])) for f, c, _ in items if nb[f] != nb[f + c - 1]}
        assert {(5000, 4100), (4100, 5001)} <= crossings, crossings
    d_items = s['t'](items, torch.int32)
    ref, out = _outputs(s), _outputs(s)
    check(lib().iamx_knn2sym_sweep(p(st.desc3), p(st.sn2), p(st.sct), p(st.img_off3), p(st.img_n),
                                   p(s['d_up']), p(s['d_wg']), p(s['d_col_off']), p(s['d_rowp_off']),
                                   len(s['up']), s['total_wg'], 2, p(ref[0]), p(ref[1]), p(ref[2]),
                                   stream_ptr()), 'iamx_knn2sym_sweep')
    check(lib().iamx_knn2sym_sweep_items(p(st.desc3), p(st.sn2), p(st.sct), p(st.img_off3), p(st.img_n),
                                         p(s['d_up']), p(d_items), p(s['d_col_off']), p(s['d_rowp_off']),
                                         len(s['up']), len(items), p(out[0]), p(out[1]), p(out[2]),
                                         stream_ptr()), 'iamx_knn2sym_sweep_items')
    torch.cuda.synchronize()
    for name, a, b in zip(('col', 'rowp', 'colmask'), ref, out):
        np.testing.assert_array_equal(b.cpu().numpy(), a.cpu().numpy(), err_msg='%s, S = %d' % (name, S))
    assert (ref[0].cpu().numpy() != -7).any()
