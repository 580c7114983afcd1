"""The host half of the cull step (imageanalysis_amd.match_culling) against the reference's own
scripts/4b-mre-by-image.py runs recorded by tools/gen_mre_golden.py: marking and deletion on the
plain lists and on the array-backed match_cleanup.Chains, byte for byte after pickle, and the
observation -> (match, last member from that image) mapping."""
import contextlib
import glob
import gzip
import io
import os
import pickle

import pytest

from imageanalysis_amd import match_culling as cull
from imageanalysis_amd.match_cleanup import Chains

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(glob.glob(os.path.join(GOLD, 'mre_*.pkl.gz')))


def _load(path):
    with gzip.open(path, 'rb') as f:
        return pickle.load(f)


def _section(stdout, first, last):
    """the lines of stdout from the first one containing `first` (cut there: the input() prompt
    before it has no newline) to the first after it starting with `last`"""
    lines = stdout.splitlines()
    a = next(i for i, l in enumerate(lines) if first in l)
    b = next(i for i, l in enumerate(lines) if l.startswith(last) and i >= a)
    return [lines[a][lines[a].index(first):]] + lines[a + 1:b + 1]


def test_goldens_present():
    assert len(CASES) == 8
    for path in CASES:
        g = _load(path)
        assert g['margin'] > 1e-9, path          # no decision sits on a rounding edge


@pytest.mark.parametrize('path', CASES, ids=os.path.basename)
@pytest.mark.parametrize('form', ['list', 'chains'])
def test_delete_marked_features_matches_reference(path, form):
    g = _load(path)
    matches = pickle.loads(g['matches_in'])
    if form == 'chains':
        matches = Chains.from_lists(matches)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        for mi, fi in g['marked']:
            cull.mark_feature(matches, mi, fi, '-')
        if g['marked']:
            cull.delete_marked_features(matches, 3, strong='--strong' in g['argv'])
    if form == 'chains':
        assert matches.untouched()                       # the vectorised path, not the rows
        matches = matches.rows()
    assert pickle.dumps(matches) == g['matches_out']
    if g['marked']:
        want = _section(g['stdout'], ' deleting marked items', 'final matches size')
        assert out.getvalue().splitlines()[-len(want):] == want


def test_delete_semantics_small():
    """strong / non-strong, chains falling below min_chain_len, short chains without marks"""
    def rows():
        return [[[1.0, 2.0, 3.0], 0, [0, [1.0, 1.0]], [1, [2.0, 2.0]], [2, [3.0, 3.0]], [3, [4.0, 4.0]]],
                [None, 0, [0, [5.0, 5.0]], [1, [6.0, 6.0]]],                      # short, unmarked
                [[4.0, 5.0, 6.0], 0, [1, [7.0, 7.0]], [2, [8.0, 8.0]], [3, [9.0, 9.0]]],
                [[7.0, 8.0, 9.0], 1, [0, [1.5, 1.5]], [2, [2.5, 2.5]], [4, [3.5, 3.5]], [5, [4.5, 4.5]]]]
    marks = [(0, 1), (2, 0), (3, 0), (3, 3)]
    # chain 0 keeps 3 members, 2 and 3 fall to 2 (< 3) and go, 1 is short but has no mark
    want = {False: [rows()[0], rows()[1]], True: [rows()[1]]}
    del want[False][0][3]
    for strong in (False, True):
        for form in ('list', 'chains'):
            m = rows() if form == 'list' else Chains.from_lists(rows())
            with contextlib.redirect_stdout(io.StringIO()):
                for mi, fi in marks:
                    cull.mark_feature(m, mi, fi, 0.0)
                cull.delete_marked_features(m, 3, strong=strong)
            got = m if form == 'list' else m.rows()
            assert pickle.dumps(got) == pickle.dumps(want[strong]), (strong, form)


def test_observation_to_last_member():
    rows = [[None, 0, [3, [0.0, 0.0]], [5, [1.0, 1.0]], [3, [2.0, 2.0]], [7, [3.0, 3.0]]],
            [None, 0, [1, [0.0, 0.0]], [2, [1.0, 1.0]]]]
    match_index = [0, 0, 0, 1, 1, 0]
    image_index = [3, 5, 7, 2, 1, 9]
    want = [2, 1, 3, 1, 0, 0]       # image 3 twice -> its last member; no member -> 0
    for m in (rows, Chains.from_lists(rows)):
        assert cull.observation_features(m, match_index, image_index).tolist() == want


@pytest.mark.parametrize('path', [p for p in CASES if 'mid_default' in p or 'dist_sd2max8' in p],
                         ids=os.path.basename)
def test_marked_members_are_last_of_their_image(path):
    """every recorded mark names the last member of its chain from that member's image; the chain
    with two observations from one image is in the projects"""
    g = _load(path)
    matches = pickle.loads(g['matches_in'])
    for mi, fi in g['marked']:
        img = matches[mi][fi + 2][0]
        assert [p[0] for p in matches[mi][2:]][fi + 1:].count(img) == 0
    dup = matches[g['dup_chain']]
    imgs = [p[0] for p in dup[2:]]
    assert len(imgs) != len(set(imgs))


def test_interactive_needs_cv2_message(monkeypatch):
    monkeypatch.setitem(__import__('sys').modules, 'cv2', None)      # import cv2 -> ImportError
    with pytest.raises(RuntimeError, match='OpenCV'):
        cull.show_outliers([[1.0, 0, 0]], [], [])
