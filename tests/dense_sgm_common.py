"""The inputs of the semi-global quality tests: dense_common's slope and roof as they are, and a harder
pair made from the same views -- seeded Gaussian noise on the neighbours' grey planes, and a band of the
ground's texture (|north - BAND_NORTH| < BAND_HALF metres, the same ground in every view) flattened to
a low contrast that still passes the texture gate.  The score stacks (reference view 0 against views
1 .. 3, 13 planes, r = 3) are computed once and shared."""
import functools

import numpy as np

import dense_common as dc
import dense_restatement as dr
import dense_sgm_restatement as ds
from imageanalysis_amd import dense

NOISE_SIGMA = 30.0                      # grey levels, on the neighbours only
BAND_NORTH, BAND_HALF = -12.0, 9.0      # metres
BAND_CONTRAST = 0.2                     # of the texture's contrast about the band's mean grey
RADIUS = 3


def _north(view, t):
    """the NED north of the surface point every pixel of the view sees (t: its true depth)"""
    h, w = t.shape
    dirs = np.concatenate([view.rays, np.ones((h, w, 1))], 2).dot(view.R)
    return view.C[0] + dirs[:, :, 0] * t


@functools.lru_cache(maxsize=None)
def hard_scene(surface):
    """-> (views, true depths): dense_common.scene(surface) made hard (the cached scene is not touched)"""
    made = [dc.make_view(surface, k) for k in range(len(dc.CENTRES))]
    band = [np.abs(_north(v, t) - BAND_NORTH) < BAND_HALF for v, t in made]
    grey = np.concatenate([np.asarray(v.G, np.float64)[b] for (v, _t), b in zip(made, band)]).mean()
    views = []
    for k, ((v, _t), b) in enumerate(zip(made, band)):
        G = np.asarray(v.G, np.float64)
        G = np.where(b, grey + BAND_CONTRAST * (G - grey), G)
        if k > 0:
            G = G + np.random.default_rng(500 + k).normal(0.0, NOISE_SIGMA, G.shape)
        views.append(dense.View(np.clip(np.rint(G), 0, 255).astype(np.float32), v.K, v.dist, v.R, v.C, rays=v.rays,
                                name='hard-%s%d' % (surface, k)))
    return views, [t for _v, t in made]


INPUTS = ('slope', 'roof', 'hard-slope', 'hard-roof')


@functools.lru_cache(maxsize=None)
def scores(name):
    """-> (score stack float32 [H, W, 13] of view 0 against views 1 .. 3, view 0's true depth)"""
    views, truth = hard_scene(name[5:]) if name.startswith('hard-') else dc.scene(name)
    S = ds.score_stack(views[0], views[1:], dc.W_FAR, dc.W_NEAR, dc.PLANES, RADIUS)
    S.setflags(write=False)
    return S, truth[0]


def quality(depth, truth):
    """-> (the share of the kept pixels within one plane step of the true inverse depth, kept pixels)"""
    step = dr.plane_step(dc.W_FAR, dc.W_NEAR, dc.PLANES)
    kept = ~np.isnan(depth)
    err = np.abs(1.0 / depth[kept].astype(np.float64) - 1.0 / truth[kept])
    return float((err <= step).mean()), int(kept.sum())


# ---- the reference's lib package as the command-line test needs it: the four cameras over the slope ----
LIB_STANDIN = {
    '__init__.py': '',
    'project.py': '''\
import os
import dense_common as dc
class ProjectMgr(object):
    """stand-in: the four cameras over the slope, frames under <project>/images"""
    def __init__(self, project_dir):
        self.project_dir = project_dir
        self.analysis_dir = os.path.join(project_dir, 'ImageAnalysis')
    def load_images_info(self):
        proj = dc.standin_project(self.analysis_dir, os.path.join(self.project_dir, 'images'))
        self.image_list = proj.image_list
''',
    'groups.py': '''\
import dense_common as dc
def load(analysis_dir):
    return [list(dc.NAMES)]
''',
}
