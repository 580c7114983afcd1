"""Shared by the tests that read device assembly (test_sweep_gaps.py, test_sweep_schedule.py,
test_sweep_items_schedule.py, test_sweep_stage_isa.py, test_isa_hazards.py): one csrc source compiled to
gfx950 assembly with the flags csrc/build.sh compiles it with, so that what they pin is what ships."""
import functools
import os
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'imageanalysis_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@functools.lru_cache(maxsize=None)
def device_assembly(src):
    """path of the gfx950 assembly of csrc/<src> (cross-compiled, no GPU needed; once per process)"""
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    flags = subprocess.check_output(['bash', os.path.join(CSRC, 'build.sh'), '--flags', src], text=True).split()
    out = os.path.join(tempfile.mkdtemp(prefix='iamx_isa_'), src[:-len('.hip')] + '.s')
    subprocess.check_call([HIPCC] + flags + ['-S', '--cuda-device-only', '-I' + os.path.join(REPO, 'include'),
                                             '-I' + CSRC, os.path.join(CSRC, src), '-o', out],
                          stderr=subprocess.DEVNULL)
    return out
