"""GPU: iamx_match_postfilter, iamx_match_pack_results and iamx_exclusive_scan_i32 through the C
ABI at their structural edges, against the plain reference of postfilter_reference.py (which
test_postfilter.py holds against the host path and the golden pairs).  Every output starts poison
filled with guard elements behind it; everything compared is integer lists and counts, exact."""
import numpy as np
import pytest
import torch

import postfilter_reference as pr

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = {torch.int32: -0x5A5A5A5B, torch.int64: -0x5A5A5A5A5A5A5A5B, torch.float64: pr.PACK_FILL_F64}
CASES = pr.cases()
BY_NAME = dict((c['name'], c) for c in CASES)


class Guarded(object):
    """a poison-filled output buffer with GUARD poison elements behind it (device memory, or
    page-locked host memory that the device writes directly)"""

    def __init__(self, shape, dtype, poison=None, pinned=False):
        self.n = int(np.prod(shape))
        self.poison = POISON[dtype] if poison is None else poison
        if pinned:
            self.buf = torch.empty(self.n + GUARD, dtype=dtype, pin_memory=True)
            self.buf.fill_(self.poison)
        else:
            self.buf = torch.full((self.n + GUARD,), self.poison, dtype=dtype, device='cuda')
        self.shape = tuple(shape)

    def ptr(self):
        from imageanalysis_amd.kernels import _ptr
        return _ptr(self.buf)

    def get(self):
        host = self.buf.cpu().numpy()
        assert (host[self.n:] == self.poison).all(), "a guard element was written"
        return host[:self.n].reshape(self.shape).copy()


def _dev(a, dtype):
    """device copy with one spare element behind it (an empty array still has an address)"""
    a = np.ascontiguousarray(a).reshape(-1)
    t = torch.zeros(len(a) + 1, dtype=dtype, device='cuda')
    if len(a):
        t[:len(a)] = torch.from_numpy(a).to(device='cuda', dtype=dtype)
    return t


def launch(cases, min_pairs, thr_factor, surv_cnt=None):
    """one iamx_match_postfilter launch over `cases`; `surv_cnt` {ordered pair: count} replaces
    survivor counts after the arrays are laid out.  Returns per pair (list, stat, status), the
    untouched part of the pair's out_pairs slot still poison."""
    from imageanalysis_amd import kernels, matcher
    from imageanalysis_amd.kernels import _ptr
    L = kernels.lib()
    clip = int(L.iamx_match_postfilter_clip())
    assert clip == pr.CLIP
    n = len(cases)
    xy = np.concatenate([c[k] for c in cases for k in ('xy1', 'xy2')]).astype(np.float32)
    kp_off = np.concatenate([[0], np.cumsum([len(c[k]) for c in cases for k in ('xy1', 'xy2')])])[:-1]
    ordered = [c['fwd'] for c in cases] + [c['rev'] for c in cases]
    cnt = np.array([len(s[0]) for s in ordered], np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)])
    if surv_cnt:
        for k, v in surv_cnt.items():
            cnt[k] = v
    slots = np.array([[2 * k, 2 * k + 1] for k in range(n)] + [[2 * k + 1, 2 * k] for k in range(n)])
    d = dict(off=_dev(off, torch.int64), cnt=_dev(cnt, torch.int32),
             q=_dev(np.concatenate([s[0] for s in ordered]), torch.int32),
             t=_dev(np.concatenate([s[1] for s in ordered]), torch.int32),
             m=_dev(np.concatenate([s[2] for s in ordered]), torch.float64),
             pairs=_dev(slots, torch.int32), kp_off=_dev(kp_off, torch.int64),
             xy=_dev(xy, torch.float32), key2=_dev(matcher.kp_key2(xy), torch.int32))
    out_cnt, out_pairs = Guarded((n,), torch.int32), Guarded((n, clip, 2), torch.int32)
    scratch, stat = Guarded((n, 2, clip, 2), torch.int32), Guarded((n, 4), torch.int32)
    status = Guarded((n,), torch.int32)
    kernels.check(L.iamx_match_postfilter(_ptr(d['off']), _ptr(d['cnt']), _ptr(d['q']), _ptr(d['t']),
                                          _ptr(d['m']), _ptr(d['pairs']), _ptr(d['kp_off']),
                                          _ptr(d['xy']), _ptr(d['key2']), n, float(pr.SIZE[0]),
                                          float(pr.SIZE[1]), float(min_pairs), float(thr_factor),
                                          out_cnt.ptr(), out_pairs.ptr(), scratch.ptr(), stat.ptr(),
                                          status.ptr(), kernels.stream_ptr()),
                  'iamx_match_postfilter')
    torch.cuda.synchronize()
    scratch.get()
    c, p, s, st = out_cnt.get(), out_pairs.get(), stat.get(), status.get()
    out = []
    for k in range(n):
        assert 0 <= c[k] <= clip
        assert (p[k, c[k]:] == POISON[torch.int32]).all(), "rows behind the count were written"
        out.append((p[k, :c[k]].astype(np.int64), s[k].tolist(), int(st[k])))
    return out


def assert_case(got, case):
    want, stat = pr.expected(case)
    lst, got_stat, status = got
    assert status == 0, case['name']
    assert got_stat == stat, case['name']
    assert len(lst) == len(want) and np.array_equal(lst, want), case['name']


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_single_pair_equals_reference(case):
    """sort / clip at the borders of its two paths, the radix select on every byte, GMS at its
    threshold, on argmax ties, in the last row / column / half cell and under rotation, the
    de-duplication's replay, the min_pairs gates and the -1 of out_stat"""
    got, = launch([case], case['min_pairs'], case['thr_factor'])
    assert_case(got, case)


def _groups(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c['min_pairs'], c['thr_factor']), []).append(c)
    return groups


def test_batch_equals_single_pair_launches():
    """the small cases in one launch per (min_pairs, factor): every pair's result is the one of its
    own launch -- and the reference's"""
    small = [c for c in CASES if c['small']]
    assert len(small) >= 12
    for (min_pairs, thr_factor), group in _groups(small).items():
        together = launch(group, min_pairs, thr_factor)
        for case, got in zip(group, together):
            alone, = launch([case], min_pairs, thr_factor)
            assert got[1:] == alone[1:] and np.array_equal(got[0], alone[0]), case['name']
            assert_case(got, case)


def test_oversize_directions_are_refused_and_their_neighbours_are_not():
    """more than 2^24 survivors in a direction: status 1, count 0, nothing read or written for
    that pair (the kernel returns before it looks at a survivor, so the count alone is large),
    and the pair beside them in the launch is what it is alone"""
    big = (1 << 24) + 1
    cases = [BY_NAME['gate_fwd40_rev25'], BY_NAME['dedupe_chain'], BY_NAME['sort_n25']]
    assert len(set((c['min_pairs'], c['thr_factor']) for c in cases)) == 1
    got = launch(cases, 25, 5.0, surv_cnt={0: big, 3 + 1: big})      # pair 0 forward, pair 1 reverse
    for k in (0, 1):
        lst, stat, status = got[k]
        assert status == 1 and len(lst) == 0 and stat == [-1, -1, -1, -1]
    assert_case(got[2], cases[2])
    alone, = launch([cases[2]], 25, 5.0)
    assert got[2][1:] == alone[1:] and np.array_equal(got[2][0], alone[0])
    # (the same two pairs with their true counts pass: it is the count that refuses them)
    for got_k, case in zip(launch(cases, 25, 5.0), cases):
        assert_case(got_k, case)


# ---- packing ----------------------------------------------------------------------------------
def run_pack(n, with_z, cap, pinned=False):
    from imageanalysis_amd import kernels
    from imageanalysis_amd.kernels import _ptr
    cnt, status, lists, z = pr.pack_inputs(n)
    off = Guarded((n + 1,), torch.int64, pinned=pinned)
    out = Guarded((cap, 2), torch.int32, poison=pr.PACK_FILL_I32, pinned=pinned)
    out_z = Guarded((cap,), torch.float64, pinned=pinned)
    d_z = _dev(z, torch.float64) if with_z else None
    keep = (_dev(cnt, torch.int32), _dev(status, torch.int32), _dev(lists, torch.int32))
    kernels.check(kernels.lib().iamx_match_pack_results(_ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
                                                        _ptr(d_z), n, pr.PACK_CLIP, cap, off.ptr(), out.ptr(),
                                                        out_z.ptr() if with_z else _ptr(None),
                                                        kernels.stream_ptr()),
                  'iamx_match_pack_results')
    torch.cuda.synchronize()
    want_off, want, want_z = pr.pack(cnt, status, lists, pr.PACK_CLIP, cap, z if with_z else None)
    assert np.array_equal(off.get(), want_off)
    assert np.array_equal(out.get(), want)                         # unwritten rows still poison
    assert np.array_equal(out_z.get(), want_z)
    return cnt, status, want_off


@pytest.mark.parametrize('with_z', [False, True], ids=['pairs', 'pairs_z'])
@pytest.mark.parametrize('n', pr.PACK_SIZES)
def test_pack_results_device_targets(n, with_z):
    """the scan's carry across its 1024-pair chunks, refused pairs that have a count, no pairs"""
    cnt, status, _lists, _z = pr.pack_inputs(n)
    total = int(cnt[status == 0].sum())
    _cnt, _status, off = run_pack(n, with_z, total + 5)
    assert off[-1] == total
    if n >= 4:
        assert (status != 0).any() and cnt[status != 0].max() > 0


@pytest.mark.parametrize('with_z', [False, True], ids=['pairs', 'pairs_z'])
def test_pack_results_page_locked_host_targets(with_z):
    cnt, status, _lists, _z = pr.pack_inputs(1025)
    run_pack(1025, with_z, int(cnt[status == 0].sum()) + 5, pinned=True)


@pytest.mark.parametrize('n', [1025, 3000])
def test_pack_results_cap_below_the_total(n):
    """pairs that do not fit are skipped, the others written, off[] complete, nothing at or
    behind cap"""
    cnt, status, _lists, _z = pr.pack_inputs(n)
    total = int(cnt[status == 0].sum())
    full = np.concatenate([[0], np.cumsum(np.where(status == 0, cnt, 0))])
    j = min(k for k in range(n // 2, n) if status[k] == 0 and cnt[k] >= 2)
    cap = int(full[j]) + 1                                        # pair j starts below cap and ends behind it
    _c, _s, off = run_pack(n, True, cap)
    assert off[-1] == total > cap
    fits = (status == 0) & (cnt > 0) & (off[:-1] + cnt <= cap)
    assert fits.any() and ((status == 0) & (cnt > 0) & ~fits).any()
    # a pair that straddles cap exists, so "skipped" is not just "behind the end"
    assert ((off[:-1] < cap) & (off[:-1] + cnt > cap) & (status == 0)).any()


# ---- scan -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', pr.SCAN_LENGTHS)
def test_exclusive_scan(n):
    from imageanalysis_amd import kernels
    from imageanalysis_amd.kernels import _ptr
    v = pr.scan_input(n)
    d_in = _dev(v, torch.int32)
    out = Guarded((n + 1,), torch.int64)
    kernels.check(kernels.lib().iamx_exclusive_scan_i32(_ptr(d_in), n, out.ptr(), kernels.stream_ptr()),
                  'iamx_exclusive_scan_i32')
    torch.cuda.synchronize()
    want = np.concatenate([[0], np.cumsum(v.astype(np.int64))])
    assert np.array_equal(out.get(), want)
    if n >= 63:
        assert want[-1] > (1 << 32) and (v == (1 << 31) - 1).any()
