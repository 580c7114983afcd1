"""CPU: the launch tables of the form-2 item walk (kernels.sym_tables, kernels.sym_items) and the
argument checks of its entry point, iamx_knn2sym_sweep_items."""
import numpy as np
import pytest


def _train_major(n_img):
    ii, jj = np.triu_indices(n_img, k=1)
    o = np.lexsort((ii, jj))
    return np.stack([ii[o], jj[o]], 1).astype(np.int32)


def _cover(items):
    return sorted((k, sl) for f, c, sl in items for k in range(f, f + c))


@pytest.mark.parametrize('S', [1, 2, 3, 4, 5])
def test_items_cover_every_pair_and_slice_once(S):
    from imageanalysis_amd import kernels
    rng = np.random.default_rng(S)
    counts = rng.choice([300, 1024, 1025, 4096, 4100, 5000, 9000], size=40)
    und = _train_major(40)[rng.permutation(780)[:300]]
    pairs = np.concatenate([und, und[:, ::-1]])
    t = kernels.sym_tables(pairs, counts, (counts + 127) // 128 * 128)
    up = t['upairs']
    items = kernels.sym_items(up, counts, S, kernels.SYM_ROWS_PER_WG[t['form']])
    nwg = (counts[up[:, 0]] + kernels.SYM_ROWS_PER_WG[t['form']] - 1) // kernels.SYM_ROWS_PER_WG[t['form']]
    assert _cover(items) == [(k, sl) for k in range(len(up)) for sl in range(nwg[k])]
    assert (items[:, 1] >= 1).all() and (items[:, 1] <= S).all()
    for f, c, _ in items:                       # one slice count per item
        assert (nwg[f:f + c] == nwg[f]).all()
    # slices of one run of pairs are consecutive items
    assert (items[1:, 2] == np.where(items[1:, 0] == items[:-1, 0], items[:-1, 2] + 1, 0)).all()


def test_roles_follow_the_register_resident_image():
    from imageanalysis_amd import kernels
    counts = np.full(30, 4096)
    und = _train_major(30)
    pairs = np.concatenate([und, und[:, ::-1]])
    t = kernels.sym_tables(pairs, counts, counts)
    up, osrc = t['upairs'], t['osrc']
    # B = the train image of the forward pair, sorted by (B, A)
    assert (np.lexsort((up[:, 1], up[:, 0])) == np.arange(len(up))).all()
    for p, (q, tr) in enumerate(pairs):
        u, role = osrc[p]
        assert sorted(up[u]) == sorted((q, tr))
        assert up[u][role] == q              # role 0: the query image is B, 1: it is A
    fwd = osrc[:len(und)]
    assert (fwd[:, 1] == 1).all() and (up[fwd[:, 0], 0] == und[:, 1]).all()


def test_headline_launches_fill_whole_rounds():
    """2812 images of 4096 rows, launches of 4096 image pairs (bench.py's schedule): S = 4, and the
    items of every full launch are a multiple of the 256 CUs"""
    from imageanalysis_amd import kernels
    counts = np.full(2812, 4096)
    und = _train_major(2812)
    for s0 in (0, 4096 * 37, 4096 * 500, len(und) // 4096 * 4096 - 4096):
        u = und[s0:s0 + 4096]
        t = kernels.sym_tables(np.concatenate([u, u[:, ::-1]]), counts, counts)
        S = kernels.sym_item_pairs(counts[t['upairs'][:, 1]])
        items = kernels.sym_items(t['upairs'], counts, S)
        assert S == 4 and len(items) == 4096 and len(items) % 256 == 0


def test_item_pairs_rule():
    from imageanalysis_amd import kernels
    assert kernels.sym_item_pairs([4096, 4000]) == 4
    assert kernels.sym_item_pairs([8192]) == 2
    assert kernels.sym_item_pairs([16384]) == 1
    assert kernels.sym_item_pairs([37000, 4096]) == 1


def test_item_sweep_argument_checks_do_not_need_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    assert L.iamx_knn2sym_sweep_items(*([None] * 9), 1, 1, None, None, None, None) == -1
    assert b'null pointer' in L.iamx_last_error()
    assert L.iamx_knn2sym_sweep_items(*([1] * 9), -1, 1, *([1] * 3), None, None) == -1
    assert b'negative count' in L.iamx_last_error()
    assert L.iamx_knn2sym_sweep_items(*([1] * 9), 0, 0, *([1] * 3), None, None) == 0
    assert L.iamx_knn2sym_kernel_id(2) == b'knn2sym_kernel<8, 4, 1, 5, 2, 0, true, 128, 1>'
