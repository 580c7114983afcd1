#!/usr/bin/env python3
"""What the form-2 symmetric sweep pays per workgroup outside its chunk loop, measured from outside:
the same MFMA work and B loads per workgroup, in four times as many shorter workgroups or in fewer
longer ones.

  (a) 1024 B images x 4 A images, all 4096 rows, sorted by A: 4096 pairs, 16 384 workgroups
  (b) the same 1024 B images x ONE A image of 16 384 rows: 1024 pairs, 4096 workgroups
  (c) (a)'s pairs through the item kernel (iamx_knn2sym_sweep_items), the B image shared by
      consecutive pairs (sorted by B), S pairs per item (--items S, repeatable)

(b) streams as many A rows per workgroup as four (a) workgroups together, so (a - b) / a is about
the most that walking S = 4 pairs per workgroup can save.  The cases alternate in one process on
one device, each for --seconds of back-to-back launches per round, timed with events in batches of
10 launches.  Prints ms per launch (median, min, max over the batches of all rounds)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from imageanalysis_amd import kernels  # noqa: E402
from imageanalysis_amd._lib import check, lib, stream_ptr  # noqa: E402

N_B, ROWS, N_A4, ROWS_B_CASE = 1024, 4096, 4, 16384
DISTINCT = 16                      # distinct row contents (every image still has its own rows in HBM)


def sift_like(rng, n):
    g = rng.gamma(0.6, 1.0, size=(n, 128))
    g = np.minimum(g / np.linalg.norm(g, axis=1, keepdims=True), 0.2)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return np.clip(np.rint(g * 512.0), 0, 255).astype(np.uint8)


def sweep_tables(store, up):
    """iamx_knn2sym_sweep's tables for unordered pairs up[:, (B, A)], form 2"""
    counts = np.asarray(store.counts, np.int64)
    caps3 = np.asarray(store.caps3, np.int64)
    nwg = (counts[up[:, 0]] + 1023) // 1024
    wg = np.zeros(len(up) + 1, np.int64)
    np.cumsum(nwg, out=wg[1:])
    col_off = np.zeros(len(up) + 1, np.int64)
    np.cumsum(caps3[up[:, 0]], out=col_off[1:])
    rowp_off = np.zeros(len(up) + 1, np.int64)
    np.cumsum(nwg * caps3[up[:, 1]], out=rowp_off[1:])
    return wg, col_off, rowp_off


class Case(object):
    def __init__(self, name, store, up, items=0):
        dev = torch.device('cuda')
        self.name, self.store, self.items = name, store, items
        wg, col_off, rowp_off = sweep_tables(store, up)
        self.n_u, self.total_wg = len(up), int(wg[-1])
        t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)  # noqa: E731
        self.d_up, self.d_wg = t(up, torch.int32), t(wg, torch.int32)
        self.d_col_off, self.d_rowp_off = t(col_off[:-1], torch.int64), t(rowp_off[:-1], torch.int64)
        self.col = torch.zeros((int(col_off[-1]), 2), dtype=torch.int32, device=dev)
        self.rowp = torch.zeros((int(rowp_off[-1]), 2), dtype=torch.int32, device=dev)
        self.colmask = torch.zeros((int(col_off[-1]),), dtype=torch.uint8, device=dev)
        if items:
            it = kernels.sym_items(up, store.counts, items)
            self.d_items, self.n_items = t(it, torch.int32), len(it)
        self.desc = '%d pairs, %d workgroups' % (self.n_u, self.total_wg) + \
            (', %d items of S = %d' % (self.n_items, items) if items else '')

    def launch(self):
        st, p = self.store, kernels._ptr
        if self.items:
            check(lib().iamx_knn2sym_sweep_items(
                p(st.desc3), p(st.sn2), p(st.sct), p(st.img_off3), p(st.img_n), p(self.d_up),
                p(self.d_items), p(self.d_col_off), p(self.d_rowp_off), self.n_u, self.n_items,
                p(self.col), p(self.rowp), p(self.colmask), stream_ptr()), 'iamx_knn2sym_sweep_items')
        else:
            check(lib().iamx_knn2sym_sweep(
                p(st.desc3), p(st.sn2), p(st.sct), p(st.img_off3), p(st.img_n), p(self.d_up),
                p(self.d_wg), p(self.d_col_off), p(self.d_rowp_off), self.n_u, self.total_wg, 2,
                p(self.col), p(self.rowp), p(self.colmask), stream_ptr()), 'iamx_knn2sym_sweep')

    def timed(self, seconds, batch=10):
        out = []
        t_end = time.time() + seconds
        while time.time() < t_end:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                self.launch()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / batch)
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--seconds', type=float, default=2.0, help='back-to-back launches per case and round')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--items', type=int, action='append', default=[],
                    help='(c): S pairs per item of the item kernel (repeatable; none: (a) and (b) only)')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(8)
    pool = [sift_like(rng, ROWS) for _ in range(DISTINCT)]
    arrays = [pool[i % DISTINCT] for i in range(N_B)]                      # B images 0 .. 1023
    arrays += [pool[(i + 3) % DISTINCT] for i in range(N_A4)]              # A images of (a)
    arrays.append(np.concatenate(pool[:ROWS_B_CASE // ROWS]))              # A image of (b)
    store = kernels.DescriptorStore.from_arrays(arrays)
    a_imgs = N_B + np.arange(N_A4)
    b_imgs = np.arange(N_B)
    up_a = np.stack([np.tile(b_imgs, N_A4), np.repeat(a_imgs, N_B)], 1).astype(np.int32)   # sorted by A
    up_b = np.stack([b_imgs, np.full(N_B, N_B + N_A4)], 1).astype(np.int32)
    cases = [Case('(a) 4096-row A', store, up_a), Case('(b) 16384-row A', store, up_b)]
    for s in args.items:                    # (c): the same pairs, sorted by B (shared by an item)
        up_c = up_a[np.lexsort((up_a[:, 1], up_a[:, 0]))]
        cases.append(Case('(c) items S=%d' % s, store, up_c, items=s))
    for c in cases:                          # warm-up, and the first results
        for _ in range(3):
            c.launch()
    torch.cuda.synchronize()
    res = {c.name: [] for c in cases}
    for _ in range(args.rounds):
        for c in cases:
            res[c.name] += c.timed(args.seconds)
    print('device %s; %d rounds x %.1f s per case, alternating; ms per launch over batches of 10'
          % (torch.cuda.get_device_name(0), args.rounds, args.seconds))
    med = {}
    for c in cases:
        v = np.array(res[c.name])
        med[c.name] = float(np.median(v))
        print('%-18s %-44s median %.4f  min %.4f  max %.4f  (%d batches, spread %.2f %%)'
              % (c.name, c.desc, med[c.name], v.min(), v.max(), len(v), 100.0 * (v.max() - v.min()) / med[c.name]))
    a, b = med[cases[0].name], med[cases[1].name]
    print('(a - b) / a = %.2f %%' % (100.0 * (a - b) / a))
    for c in cases[2:]:
        print('%s: (a - c) / a = %.2f %%' % (c.name, 100.0 * (a - med[c.name]) / a))


if __name__ == '__main__':
    main()
