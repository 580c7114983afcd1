"""CPU: the cheap reject in front of the symmetric filter's candidate rule never rejects a row the
rule keeps.  csrc/sym_cand_rule.h (the text the kernel calls) is compiled into a small host program
that walks (Lb, Ub) along the curve Lb^2 = K Ub, where the two tests could disagree:

  Ub = 1 .. 200 000, a stride through 2^24, a stride up to 2^33 and the values the packed partials'
  "no bound" (2 * 0x7F000000 + 1, + 2) gives;  for each, Lb = floor(sqrt(K Ub)) - 3 .. + 3 and Lb = 0;
  Ub = 0 with Lb = 0;  thresholds that are not finite, not positive, or whose square leaves the
  range of a double (K must be +inf: nothing is rejected early).

A mutant with K = thresh^2 (no margin) must be caught: the margin is what pays for the float32
roundings of the rule."""
import atexit
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'imageanalysis_amd', 'csrc')

PROGRAM = r'''
#include "sym_cand_rule.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static long long bad, undecided, rejected, total;

static void one(long long Lb, long long Ub, double K, double thresh)
{
    if (Lb < 0) return;
    const bool rej = sym_cand_reject(Lb, Ub, K), keep = sym_cand_keep(Lb, Ub, thresh);
    ++total;
    if (rej) ++rejected;
    if (rej && keep) {
        if (bad < 5) printf("# rejected but kept: Lb %lld Ub %lld\n", Lb, Ub);
        ++bad;
    }
    if (!rej && !keep) ++undecided;
}

static void column(long long Ub, double K, double thresh)
{
    one(0, Ub, K, thresh);
    const double kk = K < 1e300 ? K : thresh * thresh;       // (K = +inf: walk the rule's own curve)
    const double c = sqrt(kk * (double)Ub);
    if (!(c < 9e18)) return;
    const long long mid = (long long)c;
    for (long long Lb = mid - 3; Lb <= mid + 3; ++Lb) one(Lb, Ub, K, thresh);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const double thresh = strtod(argv[1], NULL);
    const bool mutant = !strcmp(argv[2], "mutant");
    const double K = mutant ? thresh * thresh : sym_cand_K(thresh);
    one(0, 0, K, thresh);
    for (long long Ub = 1; Ub <= 200000; ++Ub) column(Ub, K, thresh);
    for (long long Ub = 200001; Ub <= (1ll << 24); Ub += 97) column(Ub, K, thresh);
    for (long long Ub = (1ll << 24); Ub <= (1ll << 33); Ub += 2039) column(Ub, K, thresh);
    for (long long d = -4096; d <= 4096; ++d) column(2ll * 0x7F000000 + 1 + d, K, thresh);
    for (long long d = -64; d <= 0; ++d) column((1ll << 33) + d, K, thresh);
    printf("K %.17g bad %lld undecided %lld rejected %lld total %lld\n", K, bad, undecided, rejected, total);
    return 0;
}
'''

_driver = {}


def _program():
    if 'path' not in _driver:
        cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
        assert cxx, 'no host C++ compiler'
        d = tempfile.mkdtemp(prefix='iamx_scr_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = os.path.join(d, 'sym_cand_rule_walk.cpp')
        with open(src, 'w') as f:
            f.write(PROGRAM)
        out = os.path.join(d, 'sym_cand_rule_walk')
        # (-ffp-contract=off: the products of the two rules rounded one by one, as written)
        r = subprocess.run([cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-I', CSRC, src, '-o', out, '-lm'],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _driver['path'] = out
    return _driver['path']


def _walk(thresh, mode='rule'):
    r = subprocess.run([_program(), repr(float(thresh)), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1].split()
    res = dict(zip(last[0::2], last[1::2]))
    print(r.stdout[-600:])
    return {k: (float(v) if k == 'K' else int(v)) for k, v in res.items()}


@pytest.mark.parametrize('thresh', [202.5, 1.0, 270.0, 1e-3])
def test_reject_never_drops_a_row_the_rule_keeps(thresh):
    res = _walk(thresh)
    assert res['K'] == thresh * thresh * (1.0 + 2.0 ** -20)
    assert res['total'] > 30_000_000
    assert res['rejected'] > res['total'] // 4           # (the walk does reach both sides of the curve)
    # the rows that pass the reject and then fail the rule (printed, not bounded)
    print('thresh %r: %.4f %% of the walked rows pass the reject and fail the rule'
          % (thresh, 100.0 * res['undecided'] / res['total']))
    assert res['bad'] == 0


@pytest.mark.parametrize('thresh', [float('inf'), float('nan'), -1.0, 0.0, -float('inf'), 1e-200, 1e200])
def test_thresholds_without_a_usable_K_reject_nothing(thresh):
    res = _walk(thresh)
    assert res['K'] == float('inf')
    assert res['rejected'] == 0 and res['bad'] == 0


def test_mutant_without_margin_is_caught():
    """K = thresh^2 exactly: somewhere along the curve the rule's float32 roots keep a row that
    Lb^2 >= thresh^2 Ub rejects"""
    assert sum(_walk(t, 'mutant')['bad'] for t in (202.5, 1.0, 270.0, 1e-3)) > 0
