#!/usr/bin/env python3
"""Where a chunk of the form-2 symmetric sweep spends its cycles: the diagnostic builds of
csrc/match_knn2sym.hip (-DIAMX_T_STAMPS=<segment>, one segment a build, s_memtime differences added
into a scalar sum inside the chunk loop) run on the sweep alone (the kernel each store's launch uses), in steady state, on two stores:

  dense     tools/sweep_time.py's store (12 x 16384 rows, 66 pairs): 24 MB, stays in cache
  4096-row  tools/sweep_startup.py's store (1024 B images x 4 A images of 4096 rows, items of S = 4)

Segments: 1..16 the steps of a chunk (step 12 = the barrier step, steps 12..16 carry the stage pieces,
steps 4, 8, 12, 16 the last level of the row butterfly), 17 the barrier step's s_waitcnt (its vmcnt
part: the stamp in front of it drains lgkmcnt itself), 18 the s_barrier behind it, 19 two stamps back to
back (the stamp's own cost, subtracted from every other segment).  Every build also stamps the whole loop
with s_memtime and s_memrealtime: the in-kernel clock.  The 16x16x64 item kernel (--loops) stamps its whole
loop and its PAIR TAIL: the cycles from the end of a pair's chunk loop to the start of the item's next
pair's (the last merge, the column epilogue, the barrier, the first two stages, the first operand reads).
The tail's median is over every wave that ran chunks, waves past the end of the B image included (their tail
has no column epilogue); the 4096-row store has none.  It also stamps its ITEM START: the cycles from the
kernel's entry to the start of the first pair's chunk loop (a library from before that stamp leaves it at 0).

Prints the median over waves of cycles per chunk and the share of the loop's cycles per chunk IN THE
SAME BUILD.  Read the shares: a stamped build's fences forbid overlaps the shipped loop has, so its run
time says nothing.  The variants are small libraries of their own (the sweep's source and common.hip)
built into --dir; the package, smoke() and bench.py never load them."""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
import torch  # noqa: E402

from imageanalysis_amd import kernels  # noqa: E402
from imageanalysis_amd._lib import stream_ptr  # noqa: E402

CSRC = os.path.join(REPO, 'imageanalysis_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
NAMES = dict([(s + 1, 'step %d' % (s + 1)) for s in range(16)] +
             [(17, 'barrier step: s_waitcnt (vmcnt part)'), (18, 'barrier step: s_barrier'), (19, 'two stamps back to back')])
NW = 4


BUILD_JOBS = 8          # compilers at a time


def build_command(dirname, seg, prebuilt=False):
    """(command or None where the library is there and current, its path)"""
    out = os.path.join(dirname, 'libiamx_stamps_%d.so' % seg)
    src = [os.path.join(CSRC, 'match_knn2sym.hip'), os.path.join(CSRC, 'common.hip')]
    if os.path.exists(out) and (prebuilt or all(os.path.getmtime(out) >= os.path.getmtime(f) for f in src)):
        return None, out
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-Wno-unused-function',
           '-mllvm', '-amdgpu-mfma-vgpr-form', '-DIAMX_T_STAMPS=%d' % seg, '-I' + os.path.join(REPO, 'include'),
           '-I' + CSRC] + src + ['-o', out, '-lz', '-lpthread']
    return cmd, out


def build_all(jobs):
    """runs the commands BUILD_JOBS at a time; a failed build ends the tool with the compiler's own messages"""
    todo = [(cmd, out) for cmd, out in jobs if cmd is not None]
    for i in range(0, len(todo), BUILD_JOBS):
        procs = [(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out)
                 for cmd, out in todo[i:i + BUILD_JOBS]]
        for proc, out in procs:
            log = proc.communicate()[0]
            if proc.returncode != 0:
                raise SystemExit('build failed: %s\n%s' % (out, log))


def load(path):
    L = ctypes.CDLL(path)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.iamx_knn2sym_sweep_items.restype = ci
    L.iamx_knn2sym_sweep_items.argtypes = [vp] * 9 + [ci, ci] + [vp] * 4
    L.iamx_knn2sym_sweep_items16.restype = ci
    L.iamx_knn2sym_sweep_items16.argtypes = [vp] * 9 + [ci, ci] + [vp] * 4
    L.iamx_knn2sym_sweep.restype = ci
    L.iamx_knn2sym_sweep.argtypes = [vp] * 9 + [ci, ci, ci] + [vp] * 4
    L.iamx_knn2sym_set_stamps.restype = ci
    L.iamx_knn2sym_set_stamps.argtypes = [vp]
    return L


def dense_store():
    """tools/sweep_time.py's store and batch: the kernel its launch runs (the one-pair kernel where the batch
    forms no items), the launch's arguments and its workgroup count"""
    n_img, rows = 12, 16384
    rng = np.random.default_rng(5)
    g = rng.gamma(0.6, 1.0, size=(n_img, rows, 128))
    g /= np.linalg.norm(g, axis=2, keepdims=True)
    des = [np.clip(np.rint(np.minimum(x, 0.2) / np.linalg.norm(np.minimum(x, 0.2), axis=1, keepdims=True) * 512.0),
                   0, 255).astype(np.uint8) for x in g]
    store = kernels.DescriptorStore.from_arrays(des)
    und = [(a, b) for a in range(n_img) for b in range(a + 1, n_img)]
    pb = kernels.PairBatch(store, np.array(und + [(b, a) for a, b in und], np.int32), sym=True)
    ws = kernels.PairWorkspace(pb.rows, pb.n_pairs)
    ws.ensure_sym(pb.sym_col_rows, pb.sym_rowp_rows)
    p = kernels._ptr
    head = (p(store.desc3), p(store.sn2), p(store.sct), p(store.img_off3), p(store.img_n), p(pb.d_upairs))
    tail = (p(ws.col), p(ws.rowp), p(ws.colmask))
    if pb.sym_items_s > 1:
        return ('items', head + (p(pb.d_sym_items), p(pb.d_col_off), p(pb.d_rowp_off), pb.n_u, pb.n_sym_items) + tail,
                pb.n_sym_items, (store, pb, ws))
    assert pb.sym_form == 2, 'the dense batch runs form 2'
    return ('one pair', head + (p(pb.d_sym_wg), p(pb.d_col_off), p(pb.d_rowp_off), pb.n_u, pb.sym_total_wg, 2) + tail,
            pb.sym_total_wg, (store, pb, ws))


def startup_store():
    """tools/sweep_startup.py's case (c): 4096 pairs of 4096-row images, sorted by B, items of S = 4"""
    import sweep_startup as ss
    rng = np.random.default_rng(8)
    pool = [ss.sift_like(rng, ss.ROWS) for _ in range(ss.DISTINCT)]
    arrays = [pool[i % ss.DISTINCT] for i in range(ss.N_B)] + [pool[(i + 3) % ss.DISTINCT] for i in range(ss.N_A4)]
    store = kernels.DescriptorStore.from_arrays(arrays)
    up = np.stack([np.tile(np.arange(ss.N_B), ss.N_A4), np.repeat(ss.N_B + np.arange(ss.N_A4), ss.N_B)], 1).astype(np.int32)
    c = ss.Case('(c) items S=4', store, up[np.lexsort((up[:, 1], up[:, 0]))], items=4)
    p = kernels._ptr
    args = (p(store.desc3), p(store.sn2), p(store.sct), p(store.img_off3), p(store.img_n), p(c.d_up), p(c.d_items),
            p(c.d_col_off), p(c.d_rowp_off), c.n_u, c.n_items, p(c.col), p(c.rowp), p(c.colmask))
    return 'items', args, c.n_items, (store, c)


def measure(L, kernel, args, n_wg, seconds, pair_chunks=0):
    launch = {'items': L.iamx_knn2sym_sweep_items, 'items16': L.iamx_knn2sym_sweep_items16}.get(kernel, L.iamx_knn2sym_sweep)
    # [workgroups][waves][4], and behind it the 16x16x64 kernel's [workgroups][waves] item starts
    buf = torch.zeros(n_wg * NW * 5, dtype=torch.int64, device='cuda')
    L.iamx_knn2sym_set_stamps(buf.data_ptr())
    t_end = time.time() + seconds
    while time.time() < t_end:
        for _ in range(10):
            rc = launch(*args, stream_ptr())
            assert rc == 0, rc
        torch.cuda.synchronize()
    raw = buf.cpu().numpy().astype(np.float64)
    L.iamx_knn2sym_set_stamps(None)
    v, start = raw[:n_wg * NW * 4].reshape(-1, 4), raw[n_wg * NW * 4:]
    start = float(np.median(start[v[:, 1] > 0]))
    v = v[v[:, 1] > 0]
    seg = float(np.median(v[:, 0] / v[:, 1]))
    loop = float(np.median(v[:, 2] / v[:, 1]))
    ghz = float(np.median(v[:, 2] / v[:, 3])) * 0.1             # s_memrealtime ticks at 100 MHz
    if pair_chunks:
        # the 16x16x64 kernel's segment sum is its pair tails: the pairs of a wave's item but the last have one
        tails = v[:, 1] / pair_chunks - 1
        seg = float(np.median(v[tails > 0, 0] / tails[tails > 0]))
        return seg, loop, ghz, start
    return seg, loop, ghz


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--dir', default='/tmp/iamx_stamps', help='where the variant libraries are built (and found)')
    ap.add_argument('--segments', default='1-19')
    ap.add_argument('--seconds', type=float, default=1.0, help='back-to-back launches per variant and store')
    ap.add_argument('--loops', action='store_true',
                    help='the 4096-row store only, whole chunk loop only: the 32x32x32 item kernel and the 16x16x64 one '
                         '(which stamps nothing else), alternating, from the first library of --segments')
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--prebuilt', action='store_true', help='take the libraries found in --dir as they are')
    args = ap.parse_args()
    lo, _, hi = args.segments.partition('-')
    segs = list(range(int(lo), int(hi or lo) + 1))
    os.makedirs(args.dir, exist_ok=True)
    jobs = [build_command(args.dir, s, args.prebuilt) for s in segs]
    build_all(jobs)
    if args.build_only:
        return
    torch.cuda.set_device(0)
    if args.loops:
        import sweep_startup as ss
        L = load(jobs[0][1])
        _kernel, a, n_wg, _keep = startup_store()
        print('device %s; 4096-row store, %d workgroups, %.1f s of back-to-back launches each; median over waves'
              % (torch.cuda.get_device_name(0), n_wg, args.seconds))
        for rep in range(3):
            for kernel in ('items', 'items16'):
                pair_chunks = ss.ROWS // 128 if kernel == 'items16' else 0
                tail, loop, ghz, *start = measure(L, kernel, a, n_wg, args.seconds, pair_chunks)
                print('  %-8s chunk loop %7.0f cycles a chunk, in-kernel clock %.3f GHz, %.3f us a chunk'
                      % (kernel, loop, ghz, loop / ghz * 1e-3) +
                      (', pair tail %.0f cycles (%.2f %% of a pair of %d chunks), item start %.0f cycles'
                       % (tail, 100.0 * tail / (tail + loop * pair_chunks), pair_chunks, start[0]) if pair_chunks else ''))
        return
    stores = [('dense', ) + dense_store(), ('4096-row', ) + startup_store()]
    res = {}
    for s, (_, path) in zip(segs, jobs):
        L = load(path)
        for name, kernel, a, n_wg, _keep in stores:
            res[s, name] = measure(L, kernel, a, n_wg, args.seconds)
    print('device %s; the form-2 sweep alone, %.1f s of back-to-back launches per build and store; median over waves'
          % (torch.cuda.get_device_name(0), args.seconds))
    for name, kernel, _a, n_wg, _keep in stores:
        own = res[19, name][0] if (19, name) in res else 0.0
        loops = [res[s, name][1] for s in segs]
        print('%s store (%s kernel, %d workgroups): stamp cost %.0f cycles (subtracted below); in-kernel clock %.3f GHz '
              '(min %.3f, max %.3f over the builds)'
              % (name, kernel, n_wg, own, np.median([res[s, name][2] for s in segs]), min(res[s, name][2] for s in segs),
                 max(res[s, name][2] for s in segs)))
        print('  (loop cycles per chunk in the stamped builds: %.0f .. %.0f -- not the shipped loop\'s)' % (min(loops), max(loops)))
        for s in segs:
            if s == 19:
                continue
            seg, loop, _ = res[s, name]
            print('  %-40s %7.0f cycles a chunk  %5.1f %% of its build\'s chunk' % (NAMES[s], seg - own, 100.0 * (seg - own) / loop))
        steps = [res[s, name][0] - own for s in segs if s <= 16]
        if len(steps) == 16:
            print('  steps 1..16 together %.0f cycles; 16 x 8 MFMAs of 32 cycles = 4096' % sum(steps))


if __name__ == '__main__':
    main()
