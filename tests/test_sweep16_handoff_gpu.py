"""From one pair of an item to the next in the item sweep on v_mfma_i32_16x16x64_i8 (knn2sym16_kernel):
a pair's first two stages are issued right behind the pair's top barrier, in front of the B slice's
loads, while the waves may still hold values of the pair before; where B changes, the stage, the
squared norms and the slice are in flight together.  (Written for the hand-off -- a pair staging the
NEXT pair's chunks 0 and 1 behind its own chunk loops --, which was measured and taken out, DESIGN.md
section 4, K2, round 32; the shapes are the ones at which either can go wrong.)  Through
iamx_knn2sym_sweep_items16 with hand-made tables as test_sweep16_rowred_gpu.py launches it: `rowp`,
`col` and `colmask` bit for bit against the numpy model of form 2 (test_sweep_raw_gpu._model) and
against the 32x32x32 item kernel (iamx_knn2sym_sweep_items) on the same tables, and sixteen launches
back to back into workspaces filled with 0x7F bytes.

* consecutive chunk counts: streamed (A) images of 2, 128, 129, 256, 257 and 384 rows -- one, two and
  three chunks -- in an order that puts every ordered pair of chunk counts (1,1), (1,2), (2,1), (2,3),
  (3,2), (3,3) (and (1,3), (3,1)) INSIDE an item: the parity of the last chunk's buffer, and chunk 1
  absent (buffer 1 a second copy of chunk 0) on either side;
* a stale stage: every A image is a disjoint slice of one pool of rows, so a stage left from the pair
  before, or a chunk of the wrong image, changes `rowp` and `col`;
* a change of B inside an item, twice: register-resident (B) images of 257 rows -> 1024 rows (waves 2
  and 3 wholly past the end before the change) and 1024 rows -> 1 row (waves 1 to 3 past the end
  behind it); a B image of 1025 rows runs as two slices, the second with one row;
* short items: an item of one pair, and items whose last pair is their fourth; the next workgroup
  starts clean.

`test_the_planted_sequences_are_in_the_item_table` computes the item table with kernels.sym_items and
checks on it that all of this is there; it needs no GPU."""
import numpy as np
import pytest

from test_sweep_raw_gpu import BIG, _model, _sorted  # noqa: F401  (BIG: the sentinel the model's rows past the end hold)

S = 4
B_SIZES = (257, 1024, 1, 1025)
A_SIZES = (2, 128, 129, 256, 257, 384)
# the pairs of every B image in order, as indices into A_SIZES.  B images 0 .. 2 are one slice each and form one
# run of items of four: [0..3] [4..7: B 0 -> B 1 behind its second pair] [8..11] [12..15: B 1 -> B 2 behind
# its second pair] [16]; B image 3 has two slices: an item of four and an item of one for each
A_ORDER = ((3, 5, 2, 4, 5, 4),
           (0, 2, 4, 1, 5, 3, 2, 0),
           (1, 2, 0),
           (4, 0, 5, 1, 2))
WANTED = {(1, 1), (1, 2), (2, 1), (2, 3), (3, 2), (3, 3)}


def _images():
    rng = np.random.default_rng(3232)

    def rows(n):
        g = rng.gamma(0.6, 1.0, size=(n, 128))
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        return np.clip(np.rint(np.minimum(g, 0.2) * 640.0 * rng.uniform(0.35, 1.0, size=(n, 1))), 0, 255).astype(np.uint8)
    pool_b = rows(max(B_SIZES))
    bs = [pool_b[:k].copy() for k in B_SIZES]
    pool_a = rows(sum(A_SIZES))                          # the A images: disjoint slices of one pool
    cuts = np.concatenate([[0], np.cumsum(A_SIZES)])
    as_ = [pool_a[cuts[i]:cuts[i + 1]].copy() for i in range(len(A_SIZES))]
    return bs, as_


def _tables():
    """(upairs (B, A) sorted by B, row counts of the images, the item table)"""
    from imageanalysis_amd import kernels
    nbi = len(B_SIZES)
    up = np.array([(bi, nbi + ai) for bi, order in enumerate(A_ORDER) for ai in order], np.int32)
    counts = np.array(B_SIZES + A_SIZES, np.int64)
    return up, counts, kernels.sym_items(up, counts, S)


def test_the_planted_sequences_are_in_the_item_table():
    up, counts, items = _tables()
    nb, chunks = counts[up[:, 0]], (counts[up[:, 1]] + 127) // 128
    inside, changes = set(), []
    for f, c, _ in items:
        for u in range(f, f + c - 1):                    # pair u + 1 follows pair u in one workgroup
            inside.add((int(chunks[u]), int(chunks[u + 1])))
            if up[u, 0] != up[u + 1, 0]:
                changes.append((int(nb[u]), int(nb[u + 1])))
    assert WANTED <= inside, WANTED - inside
    # a change of B inside an item with waves wholly past the end in front of it, and behind it
    assert (257, 1024) in changes and (1024, 1) in changes, changes
    lengths = sorted({int(c) for _, c, _ in items})
    assert lengths == [1, S], lengths
    # the one-pair items: the end of the one-slice run, and both slices of the 1025-row image
    assert sum(int(c) == 1 for _, c, _ in items) == 3
    assert {int(w) for f, _, w in items if nb[f] == 1025} == {0, 1}
    # every A image is used, with 1, 2 and 3 chunks
    assert set(up[:, 1]) == set(range(len(B_SIZES), len(B_SIZES) + len(A_SIZES)))
    assert sorted(set(chunks)) == [1, 2, 3]


@pytest.fixture(scope='module')
def setup():
    import torch
    from imageanalysis_amd import kernels
    bs, as_ = _images()
    imgs = bs + as_
    store = kernels.DescriptorStore.from_arrays(imgs)
    perm = store.sperm.cpu().numpy()
    offs = store.img_off3.cpu().numpy()
    for i, x in enumerate(imgs):               # the store's row order is the model's
        assert (perm[offs[i]:offs[i] + len(x)] == _sorted(x)[2]).all()
    up, counts, items = _tables()
    assert (counts == np.asarray(store.counts, np.int64)).all()
    known, models, col_off, rowp_off = {}, [], [0], [0]
    for bi, ai in up:
        if (bi, ai) not in known:
            known[bi, ai] = _model(imgs[ai], imgs[bi], 2)
        m = known[bi, ai]
        models.append(m)
        col_off.append(col_off[-1] + int(store.caps3[bi]))
        rowp_off.append(rowp_off[-1] + m[3] * m[4])
    dev = torch.device('cuda')
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    return dict(store=store, up=up, models=models, col_off=col_off, rowp_off=rowp_off, n_items=len(items),
                d_up=t(up, torch.int32), d_items=t(items, torch.int32),
                d_col_off=t(col_off[:-1], torch.int64), d_rowp_off=t(rowp_off[:-1], torch.int64))


def _workspace(s, byte):
    import torch
    dev = torch.device('cuda')
    return (torch.full((s['col_off'][-1], 2 * 4), byte, dtype=torch.uint8, device=dev).view(torch.int32),
            torch.full((s['rowp_off'][-1], 2 * 4), byte, dtype=torch.uint8, device=dev).view(torch.int32),
            torch.full((s['col_off'][-1],), byte, dtype=torch.uint8, device=dev))


def _launch(s, ws, entry='iamx_knn2sym_sweep_items16', times=1):
    import torch
    from imageanalysis_amd import kernels
    from imageanalysis_amd._lib import check, lib, stream_ptr
    p, st = kernels._ptr, s['store']
    for _ in range(times):
        check(getattr(lib(), entry)(p(st.desc3), p(st.sn2), p(st.sct), p(st.img_off3), p(st.img_n),
                                    p(s['d_up']), p(s['d_items']), p(s['d_col_off']), p(s['d_rowp_off']),
                                    len(s['up']), s['n_items'], p(ws[0]), p(ws[1]), p(ws[2]),
                                    stream_ptr()), entry)
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in ws]


def _assert_model(s, out, byte):
    col, rowp, colmask = out
    word = np.frombuffer(bytes([byte] * 4), np.int32)[0]
    col_off, rowp_off, nbi = s['col_off'], s['rowp_off'], len(B_SIZES)
    for u, ((bi, ai), (mcol, mmask, mrowp, _nwg, _cap)) in enumerate(zip(s['up'], s['models'])):
        nb = B_SIZES[bi]
        what = 'pair %d: A %d rows, B %d rows' % (u, A_SIZES[ai - nbi], nb)
        np.testing.assert_array_equal(rowp[rowp_off[u]:rowp_off[u + 1]], mrowp, err_msg='rowp ' + what)
        np.testing.assert_array_equal(col[col_off[u]:col_off[u] + nb], mcol, err_msg='col ' + what)
        np.testing.assert_array_equal(colmask[col_off[u]:col_off[u] + nb], mmask, err_msg='colmask ' + what)
        # nothing past the image's rows
        cap = col_off[u + 1] - col_off[u]
        assert (col[col_off[u] + nb:col_off[u] + cap] == word).all(), 'col past the end, ' + what
        assert (colmask[col_off[u] + nb:col_off[u] + cap] == byte).all(), 'colmask past the end, ' + what


@pytest.fixture(scope='module')
def first(setup):
    return _launch(setup, _workspace(setup, 0xEE))


@pytest.mark.gpu
def test_a_stale_stage_would_show(setup):
    """the A images differ where it matters: no two pairs of one B image have the same row bounds, so a chunk
    of the wrong image cannot pass"""
    seen = {}
    for (bi, ai), m in zip(setup['up'], setup['models']):
        for other, rowp in seen.get(bi, {}).items():
            if other != ai and rowp.shape == m[2].shape:
                assert (rowp != m[2]).any(), (bi, ai, other)
        seen.setdefault(bi, {})[ai] = m[2]


@pytest.mark.gpu
def test_handoff_outputs_equal_numpy(setup, first):
    _assert_model(setup, first, 0xEE)


@pytest.mark.gpu
def test_handoff_outputs_equal_the_32x32x32_item_kernel(setup, first):
    ref = _launch(setup, _workspace(setup, 0xEE), entry='iamx_knn2sym_sweep_items')
    for name, a, b in zip(('col', 'rowp', 'colmask'), ref, first):
        np.testing.assert_array_equal(b, a, err_msg=name)


@pytest.mark.gpu
def test_handoff_sixteen_launches_into_a_workspace_of_0x7f(setup):
    _assert_model(setup, _launch(setup, _workspace(setup, 0x7F), times=16), 0x7F)
