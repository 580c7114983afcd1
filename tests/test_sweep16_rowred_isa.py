"""CPU: the row direction through LDS and the chunk loop without spare stages of the item sweep on
v_mfma_i32_16x16x64_i8 (knn2sym16_kernel), on the ISA the installed hipcc emits for
csrc/match_knn2sym.hip under build.sh's flags (cross-compiled to gfx950 assembly, no GPU needed;
helpers from test_sweep_gaps.py).

The kernel holds two chunk loops of 256 MFMAs: the one test_sweep16_gaps.py and test_sweep16_isa.py
read (the first, `_chunk_loop`'s), which stages chunk + 2, and the one the last two chunks of a pair
run, which stages nothing.

* neither loop holds a v_mov_b32_dpp (the row butterfly's masked levels cost two each), a
  v_permlane* or a ds_bpermute_b32; the four DPP instructions left are the reader's quad_perm minima
  with the neighbouring lane;
* each holds 32 ds_read_b128 -- 3 a tile of operands and Ct, 8 of the reader -- and 9 ds_write_b128
  -- a tile's raw row minima 8 times, the reader's four rows of R_w once -- and no ds_write_b32;
* the staging loop holds the 5 global_load_lds of a stage, the other loop none;
* the staging loop has 644 vector instructions beside its 256 MFMAs (709 with the butterfly), the
  other one the stage's 5 LDS-DMAs and their 6 held or address instructions fewer.  The counts are
  what the cross-compiler gives for the shipped source: a change of either is a change of the loop."""
import re

import pytest

from test_sweep_gaps import _gaps, _kernel, _mnemonic, _vector

NAME = '_ZN12_GLOBAL__N_116knn2sym16_kernelILi2EEEvNS_7SymArgsE'


def _mfma_loops(lines):
    """the mnemonics of every innermost loop that holds MFMAs, in the order of the assembly"""
    found = []
    for i, line in enumerate(lines):
        m = re.match(r'^(\.LBB\w+):', line)
        d = re.search(r'Loop Header: Depth=(\d+)', line + ' ' + (lines[i + 1] if i + 1 < len(lines) else ''))
        if not m or not d:
            continue
        header, depth = m.group(1), int(d.group(1))
        member = [header] + [l.split(':')[0] for l in lines if 'Header=' + header[2:] in l]
        ends = [j for j, l in enumerate(lines)
                if re.search(r's_(cbranch_\w+|branch)\s+(%s)\b' % '|'.join(map(re.escape, member)), l)]
        if not ends:
            continue
        body = [mn for mn in (_mnemonic(l) for l in lines[i:max(ends) + 1]) if mn]
        if sum(mn.startswith('v_mfma') for mn in body) >= 64:
            found.append((depth, body))
    deepest = max(d for d, _ in found)
    return [body for d, body in found if d == deepest]


@pytest.fixture(scope='module')
def loops():
    from isa_common import device_assembly
    kernel = _kernel(open(device_assembly('match_knn2sym.hip')).read().split('\n'), NAME)
    found = _mfma_loops(kernel)
    assert len(found) == 2, len(found)
    return found


def _count(body, prefix):
    return sum(mn.startswith(prefix) for mn in body)


def _vector_beside(body):
    return sum(_vector(mn) for g in _gaps(body) for mn in g)


def test_both_loops_are_256_mfmas_and_the_first_one_stages(loops):
    staging, last = loops
    for body in loops:
        assert _count(body, 'v_mfma_i32_16x16x64_i8') == 256 and _count(body, 'v_mfma') == 256
    assert _count(staging, 'global_load_lds') == 5
    assert _count(last, 'global_load_lds') == 0
    assert not [mn for mn in last if mn.startswith(('global_load', 'buffer_load'))]


@pytest.mark.parametrize('which', [0, 1])
def test_no_butterfly_in_the_loop(loops, which):
    body = loops[which]
    assert _count(body, 'v_mov_b32_dpp') == 0
    assert _count(body, 'v_permlane') == 0 and _count(body, 'ds_bpermute') == 0
    dpp = [mn for mn in body if 'dpp' in mn]
    assert len(dpp) == 4 and all(mn.startswith('v_min_i32_dpp') for mn in dpp), dpp


@pytest.mark.parametrize('which', [0, 1])
def test_lds_instructions_of_the_row_direction(loops, which):
    body = loops[which]
    print('ds_read_b128', _count(body, 'ds_read_b128'), 'ds_write_b128', _count(body, 'ds_write_b128'))
    assert _count(body, 'ds_read_b128') == 32
    assert _count(body, 'ds_write_b128') == 9
    assert _count(body, 'ds_write_b32') == 0


def test_vector_instructions_beside_the_mfmas(loops):
    staging, last = (_vector_beside(body) for body in loops)
    print('vector instructions beside the MFMAs, a chunk: staging loop', staging, 'last two chunks', last)
    assert staging == 644
    assert last == 633
    assert staging < 709
