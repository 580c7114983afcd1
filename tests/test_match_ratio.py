"""CPU: the 'bestratio' strategy's restatement (tests/ratio_reference.py) against the goldens of the
reference's own ratio_pair_matches (tools/gen_ratio_golden.py), the argument checks of the new
entries, and the strategies find_matches still refuses."""
import numpy as np
import pytest

import ratio_reference as rr


@pytest.mark.parametrize('name', rr.CASES)
def test_restatement_equals_golden(name):
    gold = rr.load_golden(name)
    inp = rr.case(name)
    assert gold['min_pairs'] == inp['min_pairs'] and gold['tol'] == rr.TOL == 33
    assert gold['cutoffs'] == rr.CUTOFFS and (gold['hypotheses'], gold['seed']) == (rr.HYPOTHESES, rr.SEED)
    for a, b in zip(gold['pairs'], inp['pairs']):            # the golden's inputs are the generator's
        for k in ('des1', 'xy1', 'des2', 'xy2'):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, k)
    got = rr.restate(gold, rr.host_ransac(gold['hypotheses'], gold['seed']))
    assert len(got) == len(gold['results'])
    for g, want in zip(got, gold['results']):
        assert np.array_equal(g['fwd'], want['fwd']) and np.array_equal(g['rev'], want['rev'])
        assert np.array_equal(g['rev'], want['fwd'][:, ::-1])
        assert np.array_equal(g['stats'], want['stats']) and g['chosen'] == want['chosen']
        assert want['margin'] > 1e-9


def test_goldens_show_what_their_names_say():
    res = {name: rr.load_golden(name)['results'] for name in rr.CASES}
    st = lambda name: res[name][0]['stats']
    assert res['clean'][0]['chosen'] == 7 and len(res['clean'][0]['fwd']) == 300
    assert st('clean')[-1].tolist() == [360, 300, 300]
    # higher bins add fitted entries but no unique ones: the strict `>` keeps the first bin
    assert res['early'][0]['chosen'] == 0 and (np.diff(st('early')[:, 1]) >= 0).all()
    assert st('early')[-1, 1] > st('early')[0, 1] and (st('early')[:, 2] == st('early')[0, 2]).all()
    assert st('below20')[:, 2].max() == 20 and res['below20'][0]['chosen'] == -1 and not len(res['below20'][0]['fwd'])
    assert st('twentyone')[:, 2].max() == 21 and len(res['twentyone'][0]['fwd']) == 21
    g = rr.load_golden('gates')
    assert st('gates')[:3, 0].tolist() == [g['min_pairs'] - 1, g['min_pairs'], g['min_pairs'] + 1]
    assert st('gates')[0, 1] == -1 and st('gates')[1, 1] >= 0
    assert st('gates')[:, 1].max() >= g['min_pairs'] > st('gates')[:, 2].max() > rr.MIN_UNIQUE
    assert res['gates'][0]['chosen'] >= 0 and not len(res['gates'][0]['fwd'])
    assert (st('dups')[:, 2] < st('dups')[:, 1]).all() and len(res['dups'][0]['fwd']) == st('dups')[-1, 2]
    assert st('exact')[:, 0].tolist() == [30, 40, 40, 40, 40, 50, 50, 50]
    assert [len(p['des1']) for p in rr.load_golden('guards')['pairs']] == [0, 47, 1, 47, 2, 2]
    assert all(r['chosen'] == -1 and not len(r['fwd']) for r in res['guards'])


def test_constants_agree():
    from imageanalysis_amd import kernels, matcher
    assert list(matcher.RATIO_CUTOFFS) == list(kernels.RATIO_CUTOFFS) == rr.CUTOFFS
    assert matcher.RATIO_MIN_UNIQUE == kernels.RATIO_MIN_UNIQUE == rr.MIN_UNIQUE == 20
    assert matcher.RATIO_HYPOTHESES == matcher.VERIFY_HYPOTHESES['homography'] == 2048


def test_new_entries_check_their_arguments_without_a_gpu():
    import ctypes
    from imageanalysis_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 64)(*([0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85] + [0.0] * 56))
    p = ctypes.cast(buf, ctypes.c_void_p)                  # (an address that is never read)
    bins = lambda **kw: L.iamx_ratio_bins(*[kw.get(k, d) for k, d in (
        ('idx', p), ('d2', p), ('row_off', p), ('pairs', p), ('kp_off', p), ('xy', p), ('n_pairs', 1),
        ('n_bins', 8), ('cutoffs', p), ('min_pairs', 25.0), ('cap', 8), ('bin_cnt', p), ('seg_cnt', p),
        ('seg_off', p), ('pts', p), ('rows', p), ('flag', p), ('stream', None))])
    select = lambda **kw: L.iamx_ratio_select(*[kw.get(k, d) for k, d in (
        ('pairs', p), ('kp_off', p), ('key2', p), ('n_pairs', 1), ('n_bins', 8), ('min_pairs', 25.0),
        ('min_unique', 20), ('bin_cnt', p), ('seg_cnt', p), ('seg_off', p), ('rows', p), ('mask', p),
        ('vstatus', p), ('cap', 8), ('stride', 1), ('tab_size', 64), ('work', p), ('out_slots', p),
        ('out_cnt', p), ('out_off', p), ('out_rows', p), ('out_cap', 1), ('chosen', p), ('stats', p),
        ('flag', p), ('stream', None))])
    for name in ('idx', 'd2', 'row_off', 'pairs', 'kp_off', 'xy', 'cutoffs', 'bin_cnt', 'seg_cnt',
                 'seg_off', 'pts', 'rows', 'flag'):
        assert bins(**{name: None}) == -1 and b'null pointer' in L.iamx_last_error(), name
    for name in ('pairs', 'kp_off', 'key2', 'bin_cnt', 'seg_cnt', 'seg_off', 'rows', 'mask', 'vstatus',
                 'work', 'out_slots', 'out_cnt', 'out_off', 'out_rows', 'chosen', 'stats', 'flag'):
        assert select(**{name: None}) == -1 and b'null pointer' in L.iamx_last_error(), name
    for fn in (bins, select):
        assert fn(n_pairs=-1) == -1
        assert fn(cap=-1) == -1
        for nb in (0, 9, -1):
            assert fn(n_bins=nb) == -1 and b'n_bins' in L.iamx_last_error()
    assert select(stride=0) == -1 and select(tab_size=48) == -1 and select(stride=64, tab_size=64) == -1
    assert select(out_cap=-1) == -1
    down = (ctypes.c_double * 8)(0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.85, 0.8)
    assert bins(cutoffs=ctypes.cast(down, ctypes.c_void_p)) == -1 and b'ascend' in L.iamx_last_error()


@pytest.mark.parametrize('strategy', ['smart', 'bruteforce'])
def test_find_matches_still_refuses_the_other_strategies(strategy):
    from imageanalysis_amd import matcher
    said = []

    class Log(object):
        def log(self, *a):
            said.append(' '.join(str(x) for x in a))
        qlog = log
    from imageanalysis_amd import _deps
    old = _deps.logger
    _deps.logger = lambda: Log()
    try:
        with pytest.raises(SystemExit):
            matcher.find_matches(None, None, strategy=strategy)
    finally:
        _deps.logger = old
    assert "'traditional'" in said[-1] and "'bestratio'" in said[-1]


def test_device_matcher_is_still_a_k2_search():
    from imageanalysis_amd import matcher
    with pytest.raises(ValueError):
        matcher.DeviceMatcher().knnMatch(np.zeros((4, 128), np.uint8), np.zeros((4, 128), np.uint8), k=3)
