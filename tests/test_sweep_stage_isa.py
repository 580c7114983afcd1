"""CPU: where the form-2 sweep's chunk loop issues its stage (the five LDS-DMA pieces of chunk + 2) and how
its steps open, for the one-pair kernel and for the item kernel, on the ISA the installed hipcc emits for
csrc/match_knn2sym.hip under build.sh's flags (cross-compiled to gfx950 assembly, no GPU needed):

* every global_load_lds of the loop sits inside an inline-asm block that writes M0 in front of it and puts
  M0 back behind it (M0 is the compiler's: nothing outside the block may rely on what the block left);
* no gap between two MFMAs holds both a global_load_lds and a ds_read (the pieces are held in gaps that
  carry valu instructions only; beside the operand reads an LDS-DMA instruction costs several slots);
* the pieces follow the loop's s_barrier, which follows its explicit s_waitcnt vmcnt(0) -- the wait the
  compiler does not know these loads need;
* no step opens with an s_nop: the first valu instructions behind a step's first MFMA read acc0, which
  was written two MFMAs earlier (row minima there read acc1 and drew 4 or 5 wait states a step);
* no clock read (s_memtime, s_memrealtime) anywhere in the shipped kernels: the stamps of
  -DIAMX_T_STAMPS exist in the diagnostic build only."""
import re

import pytest

from test_sweep_gaps import KERNELS, _kernel, assembly  # noqa: F401  (the fixture compiles the source once)


def _loop_lines(lines):
    """the raw lines of the innermost loop that holds MFMAs, comments and asm markers kept"""
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
        body = lines[i:max(ends) + 1]
        if sum('\tv_mfma' in l for l in body) >= 64 and (best is None or depth > best[0]):
            best = (depth, body)
    assert best is not None, 'no MFMA loop found'
    return best[1]


def _instructions(body):
    """(mnemonic, operands, inside an inline-asm block) of every instruction of the loop"""
    out, in_asm = [], False
    for line in body:
        if '#ASMSTART' in line:
            in_asm = True
        elif '#ASMEND' in line:
            in_asm = False
        s = line.split(';')[0].strip()
        if not s or s.startswith('.') or s.endswith(':'):
            continue
        parts = s.split(None, 1)
        out.append((parts[0], parts[1] if len(parts) > 1 else '', in_asm))
    return out


@pytest.mark.parametrize('which', sorted(KERNELS))
def test_stage_pieces_and_step_heads(assembly, which):  # noqa: F811
    kernel = _kernel(assembly, KERNELS[which])
    assert not any(re.search(r'\bs_mem(real)?time\b', l.split(';')[0]) for l in kernel), 'a clock read in a shipped kernel'
    ins = _instructions(_loop_lines(kernel))
    mfma = [i for i, (mn, _, _) in enumerate(ins) if mn.startswith('v_mfma')]
    assert len(mfma) == 128
    dma = [i for i, (mn, _, _) in enumerate(ins) if mn.startswith('global_load_lds')]
    assert len(dma) == 5
    for i in dma:
        assert ins[i][2], 'a stage piece outside an asm block'
        # its block: back to the first instruction inside the same block, on to the last
        a = i
        while a > 0 and ins[a - 1][2]:
            a -= 1
        b = i
        while b + 1 < len(ins) and ins[b + 1][2]:
            b += 1
        before = [mn + ' ' + op for mn, op, _ in ins[a:i]]
        after = [mn + ' ' + op for mn, op, _ in ins[i + 1:b + 1]]
        assert any(re.match(r's_mov_b32 m0,', x) for x in before), before
        assert any(re.match(r's_mov_b32 s\d+, m0', x) for x in before), before
        assert any(re.match(r's_mov_b32 m0, s\d+', x) for x in after), after
    # gaps: between consecutive MFMAs (the loop's last gap closes around the back edge)
    gaps = [ins[a + 1:b] for a, b in zip(mfma, mfma[1:])] + [ins[mfma[-1] + 1:] + ins[:mfma[0]]]
    for g, gap in enumerate(gaps):
        names = [mn for mn, _, _ in gap]
        assert not (any(n.startswith('global_load_lds') for n in names) and any(n.startswith('ds_read') for n in names)), \
            'gap %d holds a stage piece and an LDS read: %s' % (g, names)
    # the wait, the barrier, then the pieces
    wait = [i for i, (mn, op, _) in enumerate(ins) if mn == 's_waitcnt' and 'vmcnt(0)' in op]
    bar = [i for i, (mn, _, _) in enumerate(ins) if mn == 's_barrier']
    assert len(wait) == 1 and len(bar) == 1 and wait[0] < bar[0] < dma[0], (wait, bar, dma)
    # step heads: the gap behind the first MFMA of each of the 16 steps opens with a valu instruction
    for st in range(16):
        first = gaps[8 * st][0][0]
        assert first.startswith('v_'), 'step %d opens with %s' % (st, first)
        assert 's_nop' not in [mn for mn, _, _ in gaps[8 * st][:6]], 'step %d: s_nop at its head' % st
