"""The vignette correction of the reference's scripts/99-vignette.py on the device: the mean of
every frame of the survey (models/vignette-avg.jpg), a fit of a r^4 + b r^2 + c per channel about
the principal point, and the mask the explorer adds to every texture (models/vignette-mask.jpg,
explorer.py:233-237,286-288,517-519).

  1. sum_u32 += frame for every frame (csrc/image_colour.hip, 8 frames per launch), then
     avg = uint8(trunc(float32(sum) / float32(count))): the reference's (sum / count).astype('uint8')
     on its float32 sum, which is exact -- and so independent of its random.shuffle -- while
     255 * count < 2^24.  A survey of more than 65 793 frames is refused.
  2. models/vignette-avg.jpg through panda3d.encode_jpeg; skipped when the file exists.
  3. the file is decoded again: the reference fits the JPEG, not the mean.
  4. the radial moments on the device, three 3 x 3 systems on the host (solve_moments), or nothing
     with nofit.
  5. the fitted mask at the camera's configured size, dithered with a counter-based hash
     (DITHER_SEED); with nofit the decoded average.
  6. per channel m = 255 - v, m -= min(m); models/vignette-mask.jpg.

With histograms=True the same pass over the frames fills histogram.histograms as well (one decode
feeds both) and <analysis_dir>/histogram is written.
"""
import io
import os

import numpy as np

from . import histogram

MAX_FRAMES = 65793             # 255 * count < 2^24
DITHER_SEED = 0


def _frame_size(path):
    from PIL import Image as PILImage
    with PILImage.open(path) as im:                        # (reads the header only)
        return im.size


def check_survey(image_list):
    """the refusals, before any frame is decoded: too many frames for an exact float32 sum, and a
    frame whose size differs from the first one's (the reference dies there in `sum += rgb`)"""
    n = len(image_list)
    if n > MAX_FRAMES:
        raise ValueError("%d frames: the reference's float32 sum is exact only while 255 * count < 2^24, "
                         "that is for at most %d frames" % (n, MAX_FRAMES))
    first = None
    for im in image_list:
        size = _frame_size(im.image_file)
        if first is None:
            first = size
        elif size != first:
            raise ValueError("%s is %d x %d, the first frame (%s) is %d x %d: the average needs frames "
                             "of one size" % (im.image_file, size[0], size[1], image_list[0].image_file,
                                              first[0], first[1]))
    return first


def average(image_list, histograms=False):
    """the mean frame of the survey, device uint8 [h,w,3]; histograms=True: histogram.histograms is
    filled from the same decoded frames"""
    import torch
    from . import kernels
    from ._lib import require_gpu
    if not image_list:
        raise ValueError("no images")
    w, h = check_survey(image_list)
    dev = require_gpu()
    total = torch.zeros((h, w, 3), dtype=torch.int32, device=dev)
    histogram.frame_pass(image_list, want_hist=histograms,
                         on_frames=lambda frames: kernels.colour_accumulate(total, frames))
    return kernels.colour_mean(total, len(image_list))


def solve_moments(moments, R):
    """moments [3][8] = per channel sum s^8, s^6, s^4, s^2, n, s^4 v, s^2 v, v with s = r / R ->
    [3][3] = per channel (a, b, c) of a r^4 + b r^2 + c: the least-squares fit curve_fit makes, from
    the scaled normal equations (condition number ~ 7e2; unscaled they span 28 decades)"""
    m = np.asarray(moments, np.float64).reshape(3, 8)
    R = float(R)
    out = np.zeros((3, 3))
    for c in range(3):
        s8, s6, s4, s2, n, s4v, s2v, v = m[c]
        A = np.array([[s8, s6, s4], [s6, s4, s2], [s4, s2, n]])
        x = np.linalg.solve(A, np.array([s4v, s2v, v]))
        out[c] = (x[0] / R ** 4, x[1] / R ** 2, x[2])
    return out


def fit(frame, cu, cv):
    """frame uint8 [h,w,3] (numpy or device) -> the coefficients [3][3]"""
    from . import kernels
    m, R = kernels.colour_moments(frame, cu, cv)
    return solve_moments(m.cpu().numpy(), R)


def _decode(data):
    from . import kernels
    with kernels.polite_waits():
        return histogram._decode_frame(data)


def make_vignette(analysis_dir, image_list, cu, cv, width, height, nofit=False, histograms=False,
                  dist_cutoff=40, self_weight=0.1, seed=None):
    """99-vignette.py from its image loop to its last line.  Returns the coefficients [3][3] (None
    with nofit)."""
    from . import kernels, panda3d
    models = os.path.join(analysis_dir, 'models')
    os.makedirs(models, exist_ok=True)
    avg_file = os.path.join(models, 'vignette-avg.jpg')
    mask_file = os.path.join(models, 'vignette-mask.jpg')
    if not os.path.exists(avg_file):
        avg = average(image_list, histograms=histograms)
        panda3d._write_atomic(avg_file, panda3d.encode_jpeg(avg.cpu().numpy()))
    elif histograms:
        histogram.frame_pass(image_list, want_hist=True)
    if histograms:
        histogram.make_templates(image_list, dist_cutoff=dist_cutoff, self_weight=self_weight)
        histogram.save(analysis_dir)
    with open(avg_file, 'rb') as fp:
        vmask = _decode(fp.read())
    h, w = int(vmask.shape[0]), int(vmask.shape[1])
    print("shape:", h, w)
    coef = None
    if not nofit:
        coef = fit(vmask, cu, cv)
        for name, c in zip(('blue', 'green', 'red'), coef):
            print("%s fit coefficients:" % name, c)
        print("original shape:", height, width)
        vmask = kernels.colour_fit_mask(height, width, cu, cv, coef, DITHER_SEED if seed is None else seed)
    mask = kernels.colour_mask_finish(vmask)
    panda3d._write_atomic(mask_file, panda3d.encode_jpeg(mask.cpu().numpy()))
    return coef
