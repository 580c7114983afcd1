"""GPU: the row direction of the item sweep on v_mfma_i32_16x16x64_i8 (knn2sym16_kernel) -- a wave's
raw row minima written to LDS, read back by the wave itself, the group floors added on the reader's
side -- and its chunk loop without spare stages, through iamx_knn2sym_sweep_items16 with hand-made
tables as test_sweep16_tail_gpu.py launches it: `rowp`, `col` and `colmask` bit for bit against the
numpy model of form 2 (test_sweep_raw_gpu._model) and against the 32x32x32 item kernel
(iamx_knn2sym_sweep_items) on the same tables.

* register-resident (B) images of 1, 255, 256, 257, 1023, 1024, 1025 and 2049 rows: wave and slice
  edges, a wave wholly past the end;
* streamed (A) images of 2, 127, 128, 129, 256, 257 and 384 rows: one, two and three chunks, ragged
  last chunks, pairs on which no chunk stages a later one;
* items of S = 4 pairs in the order 2, 384, 256, 127, 128, 129, 257 rows of A: the item that starts
  a B image walks pairs of 1, 3, 2 and 1 chunks (the two raw buffers across pair ends), other items
  cross a change of B;
* sixteen launches back to back into a workspace filled with 0x7F bytes.

Every B image is a prefix of one pool of rows whose norms spread widely, so that the floors of
neighbouring groups of 32 sorted rows differ; the pool holds a run of 100 equal rows (equal norms are
neighbours in the sorted order: the run covers both lanes of a group and whole neighbouring groups,
whose floors are then equal).  The A images are copies of pool rows.  The test checks on the model's
own values that the planted cases are there: over all pairs the B row that decides a train row's R_w
sits at every one of the 16 x 16 x 4 places (lane n, block, lane group lg of the train row) of a wave;
the floors of neighbouring groups differ nearly everywhere; and there are train rows whose R_w is
reached by both lanes of a group, by two groups, and by groups of both reader halves."""
import numpy as np
import pytest

from test_sweep_raw_gpu import BIG, _model, _sorted

pytestmark = pytest.mark.gpu

S = 4
B_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049)
A_SIZES = (2, 384, 256, 127, 128, 129, 257)          # (the order of the pairs of a B image)
WAVE = 256


def _images():
    rng = np.random.default_rng(2121)
    n = max(B_SIZES)
    g = rng.gamma(0.6, 1.0, size=(n, 128))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    scale = rng.uniform(0.35, 1.0, size=(n, 1))          # norms spread widely
    pool = np.clip(np.rint(np.minimum(g, 0.2) * 640.0 * scale), 0, 255).astype(np.uint8)
    pool[20:120] = pool[7]                               # a run of equal rows in every B image of 255 rows and more
    bs = [pool[:k].copy() for k in B_SIZES]
    # A image i: copies of the pool's rows of sorted rank 5 a + 12 i, a = 0 .. k - 1 (sorted, its row a is that
    # copy): against the whole pool the place in the wave, rank mod 256, cycles over all 256 with a, and from
    # one image to the next the same place meets train row a + 156 (mod 256), another lane group
    order = _sorted(pool)[2]
    as_ = [pool[order[5 * np.arange(k) + 12 * i]].copy() for i, k in enumerate(A_SIZES)]
    return bs, as_


def _wave_values(xa, xb):
    """per wave of the B image: V [cap][16] = a sorted slot's minimum of E above its group's floor (slot s =
    rows q0 + 16 s .., group s >> 1, lane n = (s >> 1) | (s & 1) << 3), the slot's first deciding block
    [cap][16], and the floors of the wave's groups"""
    sa, n2a, _ = _sorted(xa)
    sb, n2b, _ = _sorted(xb)
    na, nb = len(xa), len(xb)
    cap = (na + 127) // 128 * 128
    E = np.full((cap, nb), BIG, np.int64)
    E[:na] = (n2a[:, None] - 2 * (sa @ sb.T) - (n2a & 1)[:, None]) // 2
    cq = n2b >> 1
    out = []
    for q0 in range(0, nb, WAVE):
        rows = np.minimum(q0 + np.arange(WAVE).reshape(16, 16), nb - 1)
        lo = cq[np.minimum(q0 + 32 * (np.arange(16) >> 1), nb - 1)]
        e = E[:, rows]                                    # [cap][slot][block]
        out.append((e.min(axis=2) + lo[None, :], e.argmin(axis=2), lo[::2], min(nb - q0, WAVE)))
    return out, na


def _planted(imgs, up):
    """the planted cases, counted on the model's own values"""
    places, tie_lanes, tie_groups, tie_halves, floors_differ, floors = set(), 0, 0, 0, 0, 0
    for bi, ai in up:
        waves, na = _wave_values(imgs[ai], imgs[bi])
        for V, blk, lo, nreal in waves:
            V, blk = V[:na], blk[:na]
            R = V.min(axis=1)
            hit = V == R[:, None]                         # [a][slot]
            s = hit.argmax(axis=1)
            a = np.arange(na)
            real = 16 * s + blk[a, s] < nreal             # (a row of the image, not a repeat of its last one)
            n = (s >> 1) | ((s & 1) << 3)
            places.update(zip(n[real], blk[a, s][real], ((a >> 2) & 3)[real]))
            grp = hit.reshape(na, 8, 2)
            tie_lanes += int(grp.all(axis=2).any(axis=1).sum())
            gh = grp.any(axis=2)                          # [a][group]
            tie_groups += int((gh.sum(axis=1) > 1).sum())
            tie_halves += int((gh[:, 0::2].any(axis=1) & gh[:, 1::2].any(axis=1)).sum())
            ng = (nreal + 31) // 32
            floors += ng - 1
            floors_differ += int((np.diff(lo[:ng]) != 0).sum())
    return places, tie_lanes, tie_groups, tie_halves, floors_differ, floors


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
    nb, chunks = counts[up[:, 0]], (counts[up[:, 1]] + 127) // 128
    assert any(nb[f] != nb[f + c - 1] for f, c, _ in items), 'no item crosses a change of B'
    assert any(c == 4 and nb[f] >= 1023 and tuple(chunks[f:f + 4]) == (1, 3, 2, 1) for f, c, _ in items), \
        'no item of pairs of 1, 3, 2 and 1 chunks'
    dev = torch.device('cuda')
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
    return dict(store=store, up=up, models=models, col_off=col_off, rowp_off=rowp_off, n_items=len(items),
                imgs=imgs, nbi=nbi,
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
    col_off, rowp_off, nbi = s['col_off'], s['rowp_off'], s['nbi']
    for u, ((bi, ai), (mcol, mmask, mrowp, _nwg, _cap)) in enumerate(zip(s['up'], s['models'])):
        nb = B_SIZES[bi]
        what = 'A %d rows, B %d rows' % (A_SIZES[ai - nbi], nb)
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


def test_the_planted_cases_are_in_the_model(setup):
    places, tie_lanes, tie_groups, tie_halves, floors_differ, floors = _planted(setup['imgs'], setup['up'])
    print('places', len(places), 'ties: lanes of a group', tie_lanes, 'groups', tie_groups, 'reader halves', tie_halves,
          'neighbouring floors that differ', floors_differ, 'of', floors)
    assert len(places) == 16 * 16 * 4, len(places)
    assert tie_lanes and tie_groups and tie_halves, (tie_lanes, tie_groups, tie_halves)
    # (all but the floors inside the run of equal rows: at most three a wave that holds it)
    assert floors_differ >= floors - 3 * len(setup['up']), (floors_differ, floors)


def test_rowred_outputs_equal_numpy(setup, first):
    _assert_model(setup, first, 0xEE)


def test_rowred_outputs_equal_the_32x32x32_item_kernel(setup, first):
    ref = _launch(setup, _workspace(setup, 0xEE), entry='iamx_knn2sym_sweep_items')
    for name, a, b in zip(('col', 'rowp', 'colmask'), ref, first):
        np.testing.assert_array_equal(b, a, err_msg=name)


def test_rowred_sixteen_launches_into_a_workspace_of_0x7f(setup):
    _assert_model(setup, _launch(setup, _workspace(setup, 0x7F), times=16), 0x7F)
