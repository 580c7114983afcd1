"""CPU: the item start of the item sweep on v_mfma_i32_16x16x64_i8 (knn2sym16_kernel) on the ISA the
installed hipcc emits for csrc/match_knn2sym.hip under build.sh's flags (cross-compiled to gfx950
assembly, no GPU needed; helpers from test_sweep_gaps.py and test_sweep16_rowred_isa.py).

A pair's first two stages are issued in front of the B slice's loads, and where B changes the squared
norms and all 32 loads of the slice are in flight together (one round trip, not one a load):

* the two chunk loops are what they were: 644 / 633 vector instructions beside 256 MFMAs, 5 / 0
  global_load_lds;
* in front of the first MFMA the kernel holds the ten global_load_lds of the two stages, behind them
  the 32 global_load_dwordx4 of the slice with no s_waitcnt between the first and the last of them, and
  the six global_load_dword of the norms in front of the slice's first wait.

(The hand-off of the next pair's first chunks behind the chunk loops, which this file was to pin, was
measured and taken out again -- DESIGN.md section 4, K2, round 32 -- so the kernel holds the 15
global_load_lds it held before: ten here, five in the staging loop.)"""
import pytest

from test_sweep16_rowred_isa import NAME, _count, _mfma_loops, _vector_beside
from test_sweep_gaps import _kernel, _mnemonic


@pytest.fixture(scope='module')
def kernel():
    from isa_common import device_assembly
    return _kernel(open(device_assembly('match_knn2sym.hip')).read().split('\n'), NAME)


def test_the_chunk_loops_are_unchanged(kernel):
    loops = _mfma_loops(kernel)
    assert len(loops) == 2, len(loops)
    staging, last = loops
    for body in loops:
        assert _count(body, 'v_mfma_i32_16x16x64_i8') == 256 and _count(body, 'v_mfma') == 256
    assert (_vector_beside(staging), _vector_beside(last)) == (644, 633)
    assert (_count(staging, 'global_load_lds'), _count(last, 'global_load_lds')) == (5, 0)
    every = [m for m in (_mnemonic(l) for l in kernel) if m]
    assert _count(every, 'global_load_lds') == 15


def test_the_stage_and_the_whole_b_slice_are_in_flight_together(kernel):
    mn = [m for m in (_mnemonic(l) for l in kernel) if m]
    head = mn[:next(i for i, m in enumerate(mn) if m.startswith('v_mfma'))]
    dma = [i for i, m in enumerate(head) if m.startswith('global_load_lds')]
    wide = [i for i, m in enumerate(head) if m == 'global_load_dwordx4']
    assert len(dma) == 10 and len(wide) == 32, (len(dma), len(wide))
    assert dma[-1] < wide[0], 'the stage is issued in front of the slice'
    assert 's_waitcnt' not in head[wide[0]:wide[-1] + 1], 'a wait between the loads of the slice'
    first_wait = wide[-1] + head[wide[-1]:].index('s_waitcnt')
    norms = [i for i, m in enumerate(head) if m == 'global_load_dword' and dma[-1] < i < first_wait]
    assert len(norms) == 6, norms
