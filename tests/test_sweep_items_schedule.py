"""CPU: the form-2 sweep that walks items (knn2sym_kernel VARIANT 1, the kernel the product launches
for form 2) keeps the chunk loop of the one-pair kernel, on the ISA the installed hipcc emits for
csrc/match_knn2sym.hip under build.sh's flags (cross-compiled to gfx950 assembly, no GPU needed),
with the limits tests/test_sweep_schedule.py sets for the one-pair kernel:

* the innermost MFMA loop (the chunk loop, inside the loop over the item's pairs) holds the 128
  MFMAs of a chunk, and fewer than 40 vector instructions of a chunk issue outside an MFMA gap;
* no gap carries more than 16 vector instructions except two, which stay within 32;
* the chunk loop has no waterfall loop (a buffer resource or address in vector registers: its
  s_and_saveexec / exec loop would cut the barrier step's gap in two);
* VGPRs + AGPRs stay within the 512 of one wave per SIMD, with no scratch."""
import re

import pytest

from isa_common import device_assembly

ITEMS2 = '_ZN12_GLOBAL__N_114knn2sym_kernelILi8ELi4ELi1ELi5ELi2ELi0ELb1ELi128ELi1EEEvNS_7SymArgsE'


@pytest.fixture(scope='module')
def items2():
    out = device_assembly('match_knn2sym.hip')
    lines, cur = [], False
    for line in open(out):
        if line.startswith(ITEMS2 + ':'):
            cur = True
        elif cur and line.startswith('\t.end_amdhsa_kernel'):
            lines.append(line.rstrip())
            break
        if cur:
            lines.append(line.rstrip())
    assert lines, 'item sweep not found'
    return lines


def _mnemonic(line):
    s = line.split(';')[0].strip()
    if not s or s.startswith('.') or s.endswith(':'):
        return None
    return s.split()[0]


def _kind(mn):
    if mn.startswith('v_mfma'):
        return 'M'
    if mn.startswith(('ds_', 'global_', 'buffer_')) or mn.startswith('v_'):
        return 'V'
    return 'S'


def _chunk_loop(lines):
    """mnemonics of the innermost loop that holds MFMAs: its header label to the last branch back"""
    best = None
    for i, line in enumerate(lines):
        # (the header note sits on the label's line, or on the next one for an inner loop)
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
        if sum(_kind(mn) == 'M' for mn in body) >= 64 and (best is None or depth > best[0]):
            best = (depth, body)
    assert best is not None, 'no MFMA loop found'
    assert best[0] >= 2, 'the chunk loop should sit inside the loop over the pairs'
    return best[1]


def test_item_chunk_loop_issues_its_vector_work_beside_mfmas(items2):
    body = _chunk_loop(items2)
    kinds = ''.join(_kind(mn) for mn in body)
    assert kinds.count('M') == 128
    parts = kinds.split('M')
    outside = parts[0].count('V') + parts[-1].count('V')
    assert outside < 40, outside
    gaps = sorted(p.count('V') for p in parts[1:-1])
    assert gaps[-3] <= 16 and gaps[-1] <= 32, gaps[-8:]


def test_item_chunk_loop_has_no_waterfall(items2):
    body = _chunk_loop(items2)
    assert not [mn for mn in body if mn.startswith(('s_and_saveexec', 's_or_saveexec'))]


def test_item_sweep_fits_one_wave_per_simd(items2):
    text = '\n'.join(items2)
    vgpr = int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', text).group(1))
    scratch = int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', text).group(1))
    assert vgpr <= 512 and scratch == 0, (vgpr, scratch)
