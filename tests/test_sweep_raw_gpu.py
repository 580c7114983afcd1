"""GPU: the symmetric sweep's raw outputs, bit for bit, against numpy -- the column results `col`
(v1, v2) and `colmask`, the row partials `rowp` (L, packed U1 / U2) -- for all three workgroup
shapes, at ragged sizes: streamed (A) images of 1, 127, 128, 129, 4096 and 5000 rows (one chunk, a
partial last chunk, the chunk edge, many chunks), register-resident (B) images of 1, 1000, 1024
and 4100 rows (waves and workgroups past the end of the image).

The model starts from the exact integer squared distances d2[a][b] of the rows in the store's
sorted order (rows of an image sorted by n2 = |x - 128|^2, stable) and follows the definitions in
csrc/match_knn2sym.hip:
  E[a][b]  = (d2 - n2_b - (n2_a & 1)) / 2 = (n2_a >> 1) - <a, b>   (the accumulator; BIG for the
             padding rows of A up to the next 128)
  column:  eight group minima per B row, group (k, g) = A rows with (a >> 5) & 3 == k and
           (a >> 2) & 1 == g; v1, v2 = the two smallest of the eight; colmask bit k + 4 g = group
           minimum <= v2
  row:     per A row and 1024 / 512 / 256-row workgroup of B, per wave w (QW * 32 B rows, lane c
           holds QW consecutive rows of its row quadruple, rows past the end repeat the last):
           R_w = min over lanes of (min over the lane's rows of E + lo(lane)), lo = Cq = n2 >> 1 of
           the lowest row of the lane's group of four lanes, S_w = the wave's largest spread of Cq
           over such a group; L = min R_w, U1 <= U2 the two smallest R_w + S_w (all at most BIG),
           stored as (L, min(U1 - L, 0xFFFF) | min(U2 - L, 0xFFFF) << 16)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 0x3F000000
NW = 4
QW = {0: 2, 1: 4, 2: 8}
A_SIZES = (1, 127, 128, 129, 4096, 5000)
B_SIZES = (1, 1000, 1024, 4100)


def _rows(rng, n):
    g = rng.gamma(0.6, 1.0, size=(n, 128))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    x = np.clip(np.rint(np.minimum(g, 0.2) * 640.0), 0, 255).astype(np.uint8)
    if n > 8:                                  # equal rows and equal norms: ties everywhere
        x[n // 2:n // 2 + 3] = x[1]
    return x


def _sorted(x):
    s = x.astype(np.int64) - 128
    n2 = (s * s).sum(1)
    p = np.argsort(n2, kind='stable')
    return s[p], n2[p], p


def _model(xa, xb, form):
    sa, n2a, _ = _sorted(xa)
    sb, n2b, _ = _sorted(xb)
    na, nb = len(xa), len(xb)
    d2 = n2a[:, None] + n2b[None, :] - 2 * np.rint(sa.astype(np.float64) @ sb.T.astype(np.float64)).astype(np.int64)
    num = d2 - n2b[None, :] - (n2a & 1)[:, None]
    assert not (num & 1).any()
    cap = (na + 127) // 128 * 128
    E = np.full((cap, nb), BIG, np.int64)
    E[:na] = num // 2

    # column direction
    gm = E.reshape(cap // 128, 4, 4, 2, 4, nb).min(axis=(0, 2, 4))          # [k][g][b]
    srt = np.sort(gm.reshape(8, nb), axis=0)
    v1, v2 = srt[0], srt[1]
    mask = np.zeros(nb, np.int64)
    for k in range(4):
        for g in range(2):
            mask |= (gm[k, g] <= v2).astype(np.int64) << (k + 4 * g)
    col = np.stack([v1, v2], 1)

    # row direction
    qw = QW[form]
    wg_rows = NW * qw * 32
    nwg = (nb + wg_rows - 1) // wg_rows
    cq = n2b >> 1
    c = np.arange(32)
    rc = (c & 16) | ((c & 3) << 2) | ((c >> 2) & 3)
    rowp = np.zeros((nwg * cap, 2), np.int64)
    for wgi in range(nwg):
        R = np.full((NW, cap), BIG, np.int64)
        S = np.zeros(NW, np.int64)
        for w in range(NW):
            q0 = wgi * wg_rows + w * qw * 32
            if q0 >= nb:
                continue
            rows = np.minimum(q0 + qw * rc[:, None] + np.arange(qw)[None, :], nb - 1)       # [c][qb]
            lo = cq[np.minimum(q0 + qw * (rc & ~3), nb - 1)]
            hi = cq[np.minimum(q0 + qw * (rc | 3) + qw - 1, nb - 1)]
            R[w] = (E[:, rows].min(axis=2) + lo[None, :]).min(axis=1)
            S[w] = (hi - lo).max()
        u = np.sort(R + S[:, None], axis=0)
        L = np.minimum(R.min(axis=0), BIG)
        U1, U2 = np.minimum(u[0], BIG), np.minimum(u[1], BIG)
        packed = np.minimum(U1 - L, 0xFFFF) | (np.minimum(U2 - L, 0xFFFF) << 16)
        rowp[wgi * cap:(wgi + 1) * cap, 0] = L
        rowp[wgi * cap:(wgi + 1) * cap, 1] = packed.astype(np.uint32).view(np.int32)
    return col, mask, rowp, nwg, cap


@pytest.mark.parametrize('form', [0, 1, 2])
def test_sweep_raw_outputs_equal_numpy(form):
    import torch
    from imageanalysis_amd import kernels
    from imageanalysis_amd._lib import check, lib, stream_ptr
    assert int(lib().iamx_knn2sym_rows_per_wg(form)) == NW * QW[form] * 32
    rng = np.random.default_rng(40 + form)
    imgs = [_rows(rng, n) for n in B_SIZES + A_SIZES]
    store = kernels.DescriptorStore.from_arrays(imgs)
    nbi = len(B_SIZES)
    # the store's row order is the model's
    perm = store.sperm.cpu().numpy()
    offs = store.img_off3.cpu().numpy()
    for i, x in enumerate(imgs):
        assert (perm[offs[i]:offs[i] + len(x)] == _sorted(x)[2]).all()

    up, col_off, rowp_off, wg, models = [], [0], [0], [0], []
    for bi in range(nbi):
        for ai in range(len(A_SIZES)):
            m = _model(imgs[nbi + ai], imgs[bi], form)
            models.append(m)
            up.append((bi, nbi + ai))
            col_off.append(col_off[-1] + int(store.caps3[bi]))
            rowp_off.append(rowp_off[-1] + m[3] * m[4])
            wg.append(wg[-1] + m[3])
    dev = torch.device('cuda')
    d_up = torch.tensor(up, dtype=torch.int32, device=dev)
    d_wg = torch.tensor(wg, dtype=torch.int32, device=dev)
    d_col_off = torch.tensor(col_off[:-1], dtype=torch.int64, device=dev)
    d_rowp_off = torch.tensor(rowp_off[:-1], dtype=torch.int64, device=dev)
    col = torch.full((col_off[-1], 2), -7, dtype=torch.int32, device=dev)
    rowp = torch.full((rowp_off[-1], 2), -7, dtype=torch.int32, device=dev)
    colmask = torch.full((col_off[-1],), 0xEE, dtype=torch.uint8, device=dev)
    p = kernels._ptr
    check(lib().iamx_knn2sym_sweep(p(store.desc3), p(store.sn2), p(store.sct), p(store.img_off3), p(store.img_n),
                                   p(d_up), p(d_wg), p(d_col_off), p(d_rowp_off), len(up), wg[-1], form,
                                   p(col), p(rowp), p(colmask), stream_ptr()), 'iamx_knn2sym_sweep')
    torch.cuda.synchronize()
    col, rowp, colmask = col.cpu().numpy(), rowp.cpu().numpy(), colmask.cpu().numpy()
    for u, ((bi, ai), (mcol, mmask, mrowp, _nwg, _cap)) in enumerate(zip(up, models)):
        nb = B_SIZES[bi]
        what = 'form %d: A %d rows, B %d rows' % (form, A_SIZES[ai - nbi], nb)
        np.testing.assert_array_equal(col[col_off[u]:col_off[u] + nb], mcol, err_msg='col ' + what)
        np.testing.assert_array_equal(colmask[col_off[u]:col_off[u] + nb], mmask, err_msg='colmask ' + what)
        np.testing.assert_array_equal(rowp[rowp_off[u]:rowp_off[u + 1]], mrowp, err_msg='rowp ' + what)
