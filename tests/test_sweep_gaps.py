"""CPU: the form-2 sweep spreads the vector work of a chunk evenly over its 128 MFMA gaps, for the
one-pair kernel and for the item kernel, on the ISA the installed hipcc emits for
csrc/match_knn2sym.hip under build.sh's flags (cross-compiled to gfx950 assembly, no GPU needed).

One wave per SIMD issues in order: an MFMA holds the vector issue port for 8 of its 32 cycles, a
vector instruction (VALU, LDS, global, buffer) or an s_nop takes 4, a v_permlane16_swap about 8; a
gap lasts max(32, sum), and a light gap cannot pay back a heavy one.  So what counts is the modelled
overflow  sum over gaps of max(0, 8 + 4 (vector + s_nop) + 4 per v_permlane16_swap - 32):

* the chunk loop holds 128 MFMAs;
* the overflow is at most 350 cycles a chunk (692 before the gaps were written out one by one, when
  the row butterfly rode in asm blocks of 8 DPP instructions and the barrier step held 30 and 31
  instructions; a perfectly even placement of those instructions would give 170 - 240);
* no gap holds more than 12 vector instructions;
* no global_load_lds shares a gap with another one.

The loop is a cycle: the gap behind its last MFMA continues in front of its first one."""
import re

import pytest

from isa_common import device_assembly

KERNELS = {
    'one_pair': '_ZN12_GLOBAL__N_114knn2sym_kernelILi8ELi4ELi0ELi5ELi2ELi0ELb1ELi128ELi1EEEvNS_7SymArgsE',
    'items': '_ZN12_GLOBAL__N_114knn2sym_kernelILi8ELi4ELi1ELi5ELi2ELi0ELb1ELi128ELi1EEEvNS_7SymArgsE',
}


@pytest.fixture(scope='module')
def assembly():
    return open(device_assembly('match_knn2sym.hip')).read().split('\n')


def _kernel(lines, name):
    out, cur = [], False
    for line in lines:
        if line.startswith(name + ':'):
            cur = True
        elif cur and line.startswith('\t.end_amdhsa_kernel'):
            break
        if cur:
            out.append(line.rstrip())
    assert out, name
    return out


def _mnemonic(line):
    s = line.split(';')[0].strip()
    if not s or s.startswith('.') or s.endswith(':'):
        return None
    return s.split()[0]


def _chunk_loop(lines):
    """mnemonics of the innermost loop that holds MFMAs: its header label to the last branch back"""
    best = None
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
        if sum(mn.startswith('v_mfma') for mn in body) >= 64 and (best is None or depth > best[0]):
            best = (depth, body)
    assert best is not None, 'no MFMA loop found'
    return best[1]


def _gaps(body):
    """the instructions between consecutive MFMAs of the loop, the last gap closed around the back edge"""
    parts, cur = [], []
    for mn in body:
        if mn.startswith('v_mfma'):
            parts.append(cur)
            cur = []
        else:
            cur.append(mn)
    return parts[1:] + [cur + parts[0]]


def _vector(mn):
    return mn.startswith(('v_', 'ds_', 'global_', 'buffer_'))


@pytest.mark.parametrize('which', sorted(KERNELS))
def test_chunk_loop_gaps(assembly, which):
    gaps = _gaps(_chunk_loop(_kernel(assembly, KERNELS[which])))
    assert len(gaps) == 128
    vector = [sum(_vector(mn) for mn in g) for g in gaps]
    cost = [8 + 4 * (v + sum(mn == 's_nop' for mn in g)) + 4 * sum(mn.startswith('v_permlane16_swap') for mn in g)
            for v, g in zip(vector, gaps)]
    overflow = sum(max(0, c - 32) for c in cost)
    print(which, 'vector instructions per gap', vector, 'overflow', overflow)
    assert overflow <= 350, (overflow, vector)
    assert max(vector) <= 12, vector
    dma = [sum(mn.startswith('global_load_lds') for mn in g) for g in gaps]
    assert sum(dma) == 5 and max(dma) == 1, dma
