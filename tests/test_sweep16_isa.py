"""CPU: the item sweep on v_mfma_i32_16x16x64_i8 (knn2sym16_kernel) on the ISA the installed hipcc
emits for csrc/match_knn2sym.hip under build.sh's flags (cross-compiled to gfx950 assembly, no GPU
needed):

* its chunk loop holds 256 v_mfma_i32_16x16x64_i8 (two chained per 16 x 16 tile, 128 rows of A
  against the wave's 256 rows of B) and no other MFMA;
* no accumulator copy and no exchange across DPP rows: no v_accvgpr_*, no v_permlane16_swap;
* no scratch, at most 512 registers (one wave per SIMD: 256 VGPRs + 256 AGPRs);
* the loop has fewer vector instructions beside its MFMAs (VALU, LDS, global, buffer) than the
  32x32x32 item kernel's loop in the same assembly."""
import re

import pytest

from test_sweep_gaps import KERNELS, _chunk_loop, _kernel, _vector

NAME = '_ZN12_GLOBAL__N_116knn2sym16_kernelILi2EEEvNS_7SymArgsE'


@pytest.fixture(scope='module')
def kernels():
    from isa_common import device_assembly
    lines = open(device_assembly('match_knn2sym.hip')).read().split('\n')
    return _kernel(lines, NAME), _kernel(lines, KERNELS['items'])


def _directive(lines, key):
    vals = [int(m.group(1)) for m in (re.match(r'\s*\.amdhsa_%s\s+(\d+)' % key, l) for l in lines) if m]
    assert len(vals) == 1, (key, vals)
    return vals[0]


def test_chunk_loop_is_256_mfmas_of_the_16x16x64_shape(kernels):
    body = _chunk_loop(kernels[0])
    mfma = [mn for mn in body if mn.startswith('v_mfma')]
    assert len(mfma) == 256 and set(mfma) == {'v_mfma_i32_16x16x64_i8'}, (len(mfma), set(mfma))
    assert not [mn for mn in body if mn.startswith(('v_accvgpr', 'v_permlane16_swap'))]


def test_no_scratch_and_at_most_512_registers(kernels):
    new = kernels[0]
    assert _directive(new, 'private_segment_fixed_size') == 0
    assert not [l for l in new if re.match(r'\s*scratch_', l)]
    # (next_free_vgpr counts the unified file: the VGPR half and the AGPR half behind accum_offset)
    assert _directive(new, 'next_free_vgpr') <= 512
    assert _directive(new, 'accum_offset') <= 256


def test_fewer_vector_instructions_beside_the_mfmas_than_the_32x32x32_loop(kernels):
    new, old = (_chunk_loop(k) for k in kernels)
    n_new = sum(_vector(mn) and not mn.startswith('v_mfma') for mn in new)
    n_old = sum(_vector(mn) and not mn.startswith('v_mfma') for mn in old)
    print('vector instructions beside the MFMAs, a chunk: 16x16x64', n_new, '32x32x32', n_old)
    assert sum(mn.startswith('v_mfma') for mn in old) == 128
    assert n_new < n_old, (n_new, n_old)
