"""GPU: a batch matched through the item sweep on v_mfma_i32_16x16x64_i8 (what PairBatch launches)
leaves the survivors, train rows and metrics that the 32x32x32 item kernel (iamx_knn2sym_sweep_items,
the same batch sent through the old entry) leaves, and for four ordered pairs those of the oracle
(oracle.cpu_ref.knn2_l2_u8 with the metric rule of bench.verify_sample).  Six images of 4096-4100
rows; image j copies 30 % of image j-1's rows with integer noise U[-6, 6], as bench.synth_descriptors
does, so that neighbours have survivors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THRESH = 270.0 * 0.75
SIZES = (4096, 4097, 4100, 4098, 4096, 4099)


def _images():
    rng = np.random.default_rng(17)
    out, prev = [], None
    for n in SIZES:
        g = rng.gamma(0.6, 1.0, size=(n, 128))
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        g = np.minimum(g, 0.2)
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        base = np.clip(np.rint(g * 512.0), 0, 255)
        cur = base.copy()
        if prev is not None:
            k = int(0.3 * min(n, len(prev)))
            src, dst = rng.permutation(len(prev))[:k], rng.permutation(n)[:k]
            cur[dst] = np.clip(prev[src] + rng.integers(-6, 7, size=(k, 128)), 0, 255)
        prev = base
        out.append(cur.astype(np.uint8))
    return out


def _survivors(pb, entry):
    import torch
    from imageanalysis_amd import kernels
    pb.sym_items_entry = entry
    ws = kernels.PairWorkspace(pb.rows, pb.n_pairs)
    pb.run(ws, THRESH)
    torch.cuda.synchronize()
    return ws.survivors(pb.n_pairs)


def test_batch_through_the_16x16x64_sweep_equals_the_old_kernel_and_the_oracle():
    from imageanalysis_amd import kernels
    from oracle import cpu_ref
    imgs = _images()
    store = kernels.DescriptorStore.from_arrays(imgs)
    ii, jj = np.triu_indices(len(imgs), k=1)
    und = np.stack([ii, jj], 1).astype(np.int32)
    ordered = np.concatenate([und, und[:, ::-1]])
    pb = kernels.PairBatch(store, ordered, sym=True)
    assert pb.sym_form == 2 and pb.sym_items_s > 1
    assert pb.sym_items_entry == 'iamx_knn2sym_sweep_items16'           # what a batch launches
    new = _survivors(pb, 'iamx_knn2sym_sweep_items16')
    old = _survivors(pb, 'iamx_knn2sym_sweep_items')
    for name, a, b in zip(('first', 'count', 'query rows', 'train rows', 'metrics'), new, old):
        np.testing.assert_array_equal(a, b, err_msg=name)
    f, c, sq, st, sm = new
    assert c.sum() > 0
    checked = 0
    for p, (a, b) in enumerate(ordered):
        if (a, b) not in ((0, 1), (1, 0), (2, 3), (5, 2)):
            continue
        ridx, rd2 = cpu_ref.knn2_l2_u8(imgs[a], imgs[b])
        d = np.sqrt(rd2.astype(np.float32)).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            metric = d[:, 0] * (d[:, 0] / d[:, 1])
        keep = np.nonzero(metric < THRESH)[0]
        lo, hi = f[p], f[p] + c[p]
        np.testing.assert_array_equal(sq[lo:hi], keep, err_msg='query rows of pair (%d, %d)' % (a, b))
        np.testing.assert_array_equal(st[lo:hi], ridx[keep, 0], err_msg='train rows of pair (%d, %d)' % (a, b))
        np.testing.assert_array_equal(sm[lo:hi], metric[keep], err_msg='metrics of pair (%d, %d)' % (a, b))
        checked += 1
    assert checked == 4
