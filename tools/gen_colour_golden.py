#!/usr/bin/env python3
"""Golden of the explorer's colour tables from the reference's OWN scripts/lib/histogram.py.

Needs a checkout of the reference project, given by the IAMX_REFERENCE environment variable (the
directory that holds its scripts/).  The reference's file is executed as it is, with stand-ins for
what is absent here:

  cv2.split / cv2.merge   numpy (channel views / np.dstack)
  cv2.resize              oracle.image_oracle.resize_linear_u8 (the bilinear restatement the
                          package's own resize kernel is tested against)
  lib.logger              a log() that prints

on a seeded scene of eleven cameras with 120 x 80 frames.  The poses pin every branch of
make_templates:

  c0 - c1   exactly 1.0 m apart                         (dist_m <= 1: weight 1)
  c0 - c2   offsets (24, 32, 0): exactly 40.0 m         (dist_m > dist_cutoff is False: kept)
  c0        first neighbour in list order within 1 m, the later ones not (a float32 sum that takes
            float64 terms in place)
  c3        beyond 40 m of everything                   (float32 NaN templates: 0/0)
  c4, c5    the same position                           (dist_m = 0)
  c9, c10   0.3 m apart, far from the rest              (float32 templates: no float64 weight)

tests/golden/colour_scene.pkl.gz: the names, the poses, the frames, the reference's histograms and
templates, and its match_neighbors outputs for c0 and c9.  No reference source goes into it.

    IAMX_REFERENCE=<reference checkout> python tools/gen_colour_golden.py
"""
import contextlib
import gzip
import importlib.util
import io
import os
import pickle
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(REPO, 'tests', 'golden')
sys.path.insert(0, REPO)

H, W = 80, 120
NED = [(0.0, 0.0, -100.0), (1.0, 0.0, -100.0), (24.0, 32.0, -100.0), (1000.0, 1000.0, -100.0),
       (10.0, 5.0, -100.0), (10.0, 5.0, -100.0), (10.5, 5.0, -100.0), (30.0, 30.0, -100.0),
       (-20.0, 12.0, -103.0), (2000.0, 0.0, -100.0), (2000.3, 0.0, -100.0)]
MATCHED = ('c0', 'c9')
MAX_BYTES = 500 * 1000


class Frame(object):
    def __init__(self, name, ned, pixels):
        self.name, self.ned, self.pixels = name, ned, pixels

    def load_rgb(self):
        return self.pixels

    def get_camera_pose(self):
        return list(self.ned), [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]


def frames():
    rng = np.random.default_rng(20261017)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for k, ned in enumerate(NED):
        gain, lift = 0.55 + 0.08 * (k % 6), 8.0 * (k % 4)
        base = 70 + 60 * np.sin(x / 11.0 + k) * np.cos(y / 7.0 - k) + 0.4 * x
        img = base[:, :, None] * gain * np.array([1.0, 0.9, 1.1]) + lift + rng.normal(0, 12, (H, W, 3))
        out.append(Frame('c%d' % k, ned, np.clip(np.rint(img), 0, 255).astype(np.uint8)))
    return out


def reference_histogram():
    """the reference's lib/histogram.py, executed with the stand-ins"""
    from oracle.image_oracle import resize_linear_u8
    ref = os.environ.get('IAMX_REFERENCE')
    if not ref:
        sys.exit("IAMX_REFERENCE must name a checkout of the reference project")

    def resize(img, dsize, fx=None, fy=None):
        assert tuple(dsize) == (0, 0) and fx == fy
        return resize_linear_u8(img, fx)
    cv2 = types.ModuleType('cv2')
    cv2.resize = resize
    cv2.split = lambda img: tuple(np.ascontiguousarray(img[:, :, k]) for k in range(img.shape[2]))
    cv2.merge = lambda chans: np.dstack(chans)
    lib = types.ModuleType('lib')
    lib.__path__ = []
    logger = types.ModuleType('lib.logger')
    logger.log = lambda *a: print(*a)
    sys.modules.update({'cv2': cv2, 'lib': lib, 'lib.logger': logger})
    spec = importlib.util.spec_from_file_location('lib.histogram',
                                                  os.path.join(ref, 'scripts', 'lib', 'histogram.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    hist = reference_histogram()
    scene = frames()
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)       # (c3: 0/0)
        hist.make_histograms(scene)
        hist.make_templates(scene)
        matched = {name: hist.match_neighbors(scene[int(name[1:])].pixels, name) for name in MATCHED}
    gold = {'names': [f.name for f in scene], 'ned': [list(f.ned) for f in scene],
            'frames': {f.name: f.pixels for f in scene},
            'histograms': {k: tuple(np.array(a) for a in v) for k, v in hist.histograms.items()},
            'templates': {k: tuple(np.array(a) for a in v) for k, v in hist.templates.items()},
            'matched': matched, 'dist_cutoff': 40, 'self_weight': 0.1, 'numpy': np.__version__}
    path = os.path.join(GOLD, 'colour_scene.pkl.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        pickle.dump(gold, f, protocol=4)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    for name in gold['names']:
        t = gold['templates'][name]
        print(name, t[0].dtype, 'NaN' if np.isnan(t[0]).any() else '')
    print(path, size, 'bytes')


if __name__ == '__main__':
    main()
