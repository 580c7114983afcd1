"""CPU: the shipped sweep (form 2) keeps its MFMA pipe fed across tile and chunk edges.  Pinned on
the ISA the installed hipcc emits for csrc/match_knn2sym.hip under build.sh's flags (cross-compiled
to gfx950 assembly, no GPU needed):

* the chunk loop holds the 128 MFMAs of a chunk, and fewer than 40 vector instructions (VALU, LDS,
  global) of a chunk issue outside an MFMA gap -- in front of the loop body's first MFMA or behind
  its last one (111 VALU + 9 LDS when the chunk head and tail were not pipelined);
* no gap between two MFMAs carries more than 16 vector instructions except two, which stay within
  32: the one that holds the chunk's barrier, the stage of the chunk after next and the merge of
  the previous chunk, and the one with that stage's address arithmetic (the row butterfly's levels
  were one 29 + 18 instruction gap per tile).  The target of at most 6 per gap is NOT met: the
  butterfly pieces are asm blocks of 8 DPP instructions (gaps of 13) and the barrier step holds
  about 30;
* VGPRs + AGPRs stay within the 512 of one wave per SIMD, with no scratch."""
import re

import pytest

from isa_common import device_assembly

FORM2 = '_ZN12_GLOBAL__N_114knn2sym_kernelILi8ELi4ELi0ELi5ELi2ELi0ELb1ELi128ELi1EEEvNS_7SymArgsE'


@pytest.fixture(scope='module')
def form2():
    out = device_assembly('match_knn2sym.hip')
    lines, cur = [], False
    for line in open(out):
        if line.startswith(FORM2 + ':'):
            cur = True
        elif cur and line.startswith('\t.end_amdhsa_kernel'):
            lines.append(line.rstrip())
            break
        if cur:
            lines.append(line.rstrip())
    assert lines, 'form-2 sweep not found'
    return lines


def _kind(line):
    s = line.split(';')[0].strip()
    if not s or s.startswith('.') or s.endswith(':'):
        return None
    mn = s.split()[0]
    if mn.startswith('v_mfma'):
        return 'M'
    if mn.startswith(('ds_', 'global_', 'buffer_')) or mn.startswith('v_'):
        return 'V'
    return 'S'


def _chunk_loop(lines):
    """instruction kinds of the loop that holds the MFMAs: its header label to the last branch back"""
    for i, line in enumerate(lines):
        m = re.match(r'^(\.LBB\w+):.*Loop Header', line)
        if not m:
            continue
        header = m.group(1)
        member = [header] + [l.split(':')[0] for l in lines if 'Header=' + header[2:] in l]    # (.LBB -> BB)
        ends = [j for j, l in enumerate(lines)
                if re.search(r's_(cbranch_\w+|branch)\s+(%s)\b' % '|'.join(map(re.escape, member)), l)]
        if not ends:
            continue
        body = [k for k in (_kind(l) for l in lines[i:max(ends) + 1]) if k]
        if body.count('M') >= 64:
            return body
    raise AssertionError('no MFMA loop found')


def test_chunk_loop_issues_its_vector_work_beside_mfmas(form2):
    body = _chunk_loop(form2)
    assert body.count('M') == 128
    parts = ''.join(body).split('M')
    outside = parts[0].count('V') + parts[-1].count('V')
    assert outside < 40, outside
    gaps = sorted(p.count('V') for p in parts[1:-1])
    # (two gaps larger: the chunk's barrier with the stage of the chunk after next and the merge,
    #  and the address arithmetic of that stage)
    assert gaps[-3] <= 16 and gaps[-1] <= 32, gaps[-8:]


def test_one_wave_fits_its_registers(form2):
    text = '\n'.join(form2)
    vgpr = int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', text).group(1))
    scratch = int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', text).group(1))
    assert vgpr <= 512 and scratch == 0, (vgpr, scratch)
