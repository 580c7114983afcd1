"""CPU: csrc/build.sh compiles what is stale, with the flags each source is meant to get, at most 16 at a
time, and a source that does not compile fails the build instead of linking an older object.

Every case runs a COPY of build.sh in a temporary tree that mirrors imageanalysis_amd/csrc/ and include/
(empty files under the real names), with HIPCC pointing at a stub that logs its command line and its start
and end time, creates its -o file and fails for the source $STUB_FAIL names.  Nothing is compiled and the
real obj/ and libiamx.so are never touched."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, 'imageanalysis_amd', 'csrc')
SOURCES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, '*.hip')))
COMMON = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function']
PER_FILE = dict({name + '.hip': ['-ffp-contract=off'] for name in (
    'trf_vec', 'ba_robust', 'image_area', 'image_colour', 'surface_grid', 'image_prep', 'chain_geom',
    'ortho_raster', 'match_verify', 'terrain', 'match_ratio')},
    **{'match_knn2sym.hip': ['-mllvm', '-amdgpu-mfma-vgpr-form']})

STUB = r'''#!/bin/bash
start=$(date +%s.%N)
prev="" out="" src=""
for a in "$@"; do
    [ "$prev" = "-o" ] && out="$a"
    case "$a" in *.hip) src="$(basename "$a")" ;; esac
    prev="$a"
done
sleep 0.03
: > "$out"                     # (a compiler may leave a partial object behind when it fails)
rc=0
[ -n "$STUB_FAIL" ] && [ "$src" = "$STUB_FAIL" ] && rc=1
echo "$start $(date +%s.%N) $rc $*" >> "$STUB_LOG"
exit $rc
'''


class Tree:
    def __init__(self, root):
        self.root = str(root)
        self.csrc = os.path.join(self.root, 'imageanalysis_amd', 'csrc')
        self.lib = os.path.join(self.root, 'imageanalysis_amd', 'libiamx.so')
        self.log = os.path.join(self.root, 'hipcc.log')
        self.hipcc = os.path.join(self.root, 'hipcc')
        os.makedirs(self.csrc)
        os.makedirs(os.path.join(self.root, 'include'))
        shutil.copy(os.path.join(CSRC, 'build.sh'), self.csrc)
        for p in glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')):
            open(os.path.join(self.csrc, os.path.basename(p)), 'w').close()
        open(os.path.join(self.root, 'include', 'iamx.h'), 'w').close()
        with open(self.hipcc, 'w') as f:
            f.write(STUB)
        os.chmod(self.hipcc, 0o755)

    def obj(self, src):
        return os.path.join(self.csrc, 'obj', src[:-len('.hip')] + '.o')

    def run(self, *args, **env):
        """-> (exit status, output, [(start, end, argv)] of the compiles, the same of the links) of one run"""
        open(self.log, 'w').close()
        keep = {k: v for k, v in os.environ.items()
                if k not in ('IAMX_REBUILD', 'IAMX_EXTRA_FLAGS', 'MAX_JOBS', 'STUB_FAIL')}
        r = subprocess.run(['bash', os.path.join(self.csrc, 'build.sh')] + list(args), text=True,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           env=dict(keep, HIPCC=self.hipcc, STUB_LOG=self.log, **env))
        calls = [(float(w[0]), float(w[1]), w[3:]) for w in (l.split() for l in open(self.log))]
        return (r.returncode, r.stdout, [c for c in calls if '-c' in c[2]], [c for c in calls if '-shared' in c[2]])

    def age(self):
        """every file 100 s older, their order kept: what is touched next is newer than every object"""
        for d, _dirs, files in os.walk(self.root):
            for f in files:
                st = os.stat(os.path.join(d, f))
                os.utime(os.path.join(d, f), ns=(st.st_atime_ns, st.st_mtime_ns - 100 * 10 ** 9))

    def touch(self, *rel):
        p = os.path.join(self.root, *rel)
        open(p, 'a').close()
        os.utime(p)


def _compiled(compiles):
    return sorted(os.path.basename(a) for _s, _e, argv in compiles for a in argv if a.endswith('.hip'))


def _most_at_once(compiles):
    edges = sorted([(s, 1) for s, _e, _a in compiles] + [(e, -1) for _s, e, _a in compiles])
    most = now = 0
    for _t, step in edges:          # (an end sorts in front of a start at the same instant)
        now += step
        most = max(most, now)
    return most


@pytest.fixture
def tree(tmp_path):
    return Tree(tmp_path)


def test_the_tree_under_test_has_the_sources_the_flag_table_names():
    assert set(PER_FILE) <= set(SOURCES) and len(SOURCES) >= 26


@pytest.mark.parametrize('rebuild', [False, True])
def test_a_source_that_does_not_compile_fails_the_build(tree, rebuild):
    assert tree.run()[0] == 0 and os.path.exists(tree.lib) and os.path.exists(tree.obj('jpeg.hip'))
    tree.age()
    env = {'IAMX_REBUILD': '1'} if rebuild else {}
    if not rebuild:
        tree.touch('imageanalysis_amd', 'csrc', 'jpeg.hip')       # its object in obj/ is the stale one
    rc, out, compiles, links = tree.run(STUB_FAIL='jpeg.hip', **env)
    assert rc != 0
    assert 'jpeg.hip' in out and 'sift.hip' not in out
    assert _compiled(compiles) == (SOURCES if rebuild else ['jpeg.hip'])
    assert not links
    assert not os.path.exists(tree.lib)
    assert not os.path.exists(tree.obj('jpeg.hip'))
    assert not glob.glob(os.path.join(tree.root, 'imageanalysis_amd', '*.so'))


def test_a_clean_run_compiles_every_source_once_and_links_them_all(tree):
    rc, out, compiles, links = tree.run()
    assert rc == 0, out
    assert _compiled(compiles) == SOURCES
    assert len(links) == 1
    assert sorted(a for a in links[0][2] if a.endswith('.o')) == sorted(tree.obj(s) for s in SOURCES)
    assert os.path.exists(tree.lib)
    assert glob.glob(os.path.join(tree.root, 'imageanalysis_amd', '*.so')) == [tree.lib]    # no temporary left


def test_a_touched_source_is_the_only_one_compiled(tree):
    assert tree.run()[0] == 0
    tree.age()
    rc, _out, compiles, links = tree.run()
    assert rc == 0 and _compiled(compiles) == [] and len(links) == 1                # nothing touched: only the link
    tree.age()
    tree.touch('imageanalysis_amd', 'csrc', 'terrain.hip')
    rc, _out, compiles, links = tree.run()
    assert rc == 0 and _compiled(compiles) == ['terrain.hip'] and len(links) == 1
    tree.age()
    rc, _out, compiles, links = tree.run()
    assert rc == 0 and _compiled(compiles) == [] and len(links) == 1


HEADERS = ['include/iamx.h'] + ['imageanalysis_amd/csrc/' + os.path.basename(p)
                                for p in sorted(glob.glob(os.path.join(CSRC, '*.h')))]


@pytest.mark.parametrize('header', HEADERS + ['imageanalysis_amd/csrc/a_new_header.h'])   # the last: added, then touched
def test_a_touched_header_recompiles_every_source(tree, header):
    assert len(HEADERS) >= 6
    assert tree.run()[0] == 0
    tree.age()
    tree.touch(*header.split('/'))
    rc, _out, compiles, links = tree.run()
    assert rc == 0 and _compiled(compiles) == SOURCES and len(links) == 1
    tree.age()
    rc, _out, compiles, links = tree.run()
    assert rc == 0 and _compiled(compiles) == [] and len(links) == 1


@pytest.mark.parametrize('max_jobs, cap', [(None, 16), ('3', 3), ('64', 16)])
def test_job_cap(tree, max_jobs, cap):
    rc, _out, compiles, _links = tree.run(**({} if max_jobs is None else {'MAX_JOBS': max_jobs}))
    assert rc == 0 and len(compiles) == len(SOURCES)
    assert 2 <= _most_at_once(compiles) <= cap


def test_the_two_long_compiles_start_first(tree):
    rc, _out, compiles, _links = tree.run(MAX_JOBS='2')       # (two at a time: the third starts when one has ended)
    assert rc == 0 and _most_at_once(compiles) <= 2
    order = [os.path.basename(argv[-3]) for _s, _e, argv in sorted(compiles)]
    assert set(order[:2]) == {'match_knn2sym.hip', 'sift.hip'}


def test_flags_mode_prints_the_flags_and_compiles_nothing(tree):
    for src in SOURCES:
        rc, out, compiles, links = tree.run('--flags', src)
        assert rc == 0 and out.split() == COMMON + PER_FILE.get(src, []), src
        assert not compiles and not links
    rc, out, compiles, links = tree.run('--flags', 'terrain.hip', IAMX_EXTRA_FLAGS='-DIAMX_T_NOPACK -g')
    assert out.split() == COMMON + ['-ffp-contract=off', '-DIAMX_T_NOPACK', '-g']
    rc, out, compiles, links = tree.run('--flags', 'common.hip', IAMX_EXTRA_FLAGS='-DIAMX_T_NOPACK')
    assert out.split() == COMMON + ['-DIAMX_T_NOPACK']
    assert not os.path.exists(os.path.join(tree.csrc, 'obj')) and not os.path.exists(tree.lib)
    # and a compile gets exactly what --flags prints, then -c <source> -o <object>
    rc, _out, compiles, _links = tree.run(IAMX_EXTRA_FLAGS='-DIAMX_T_NOPACK')
    assert rc == 0
    for _s, _e, argv in compiles:
        src = os.path.basename(argv[-3])
        assert argv == COMMON + PER_FILE.get(src, []) + ['-DIAMX_T_NOPACK', '-c', os.path.join(tree.csrc, src),
                                                         '-o', tree.obj(src)]
