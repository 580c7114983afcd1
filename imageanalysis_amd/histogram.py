"""MI355X-native stand-in for the reference's scripts/lib/histogram.py (neighbour histogram
matching, what explorer.py:79,284,515 loads and applies before it shows a texture):

    get_histogram_rgb(image, scale=0.25)                histogram.py:18-30
    make_histograms(image_list)                         histogram.py:32-35
    make_templates(image_list, dist_cutoff, self_weight)   histogram.py:39-96
    match_neighbors(rgb, image_name)                    histogram.py:98-119
    load(analysis_dir) / save(analysis_dir)             histogram.py:121-135

with the same module-level `histograms` / `templates` dicts and the same file: a pickle of
(histograms, templates) at <analysis_dir>/histogram that the reference's own load() reads.

A histogram is made from the file's bytes on the device: the split JPEG decoder
(kernels.jpeg_decode), the quarter-size bilinear image (kernels.equalize_resize(equalize=False);
its parity with cv2.resize is unpinned, see README) and csrc/image_colour.hip's histogram kernel;
768 counts come back.  make_histograms runs on the worker scheme of
panda3d.make_textures_opencv.  The look-up tables of match_neighbors are built with the
reference's expressions and applied by the look-up kernel.

make_templates stays on the host (768 numbers per neighbour) and gives the reference's result bit
for bit, dtype included: its scalar expressions per candidate, its order of accumulation, and the
dtypes numpy's promotion gives it written out (below).  Only the candidate search differs: a
cKDTree with a padded radius instead of the loop over all pairs.

One departure: for an image whose template is NaN (no neighbour within the cutoff: 0/0) the
reference casts NaN to uint8, which is undefined; match_neighbors here logs the name and returns
the image unchanged.

Use `install(lib.histogram)` to give the reference's module these functions (drop-in).
"""
import io
import os
import pickle
import threading

import numpy as np

from . import _deps

histograms = {}
templates = {}

# worker threads of one pass over the frames (each holds one decoded frame, 60 MB at 20 MP, on the
# device); never beyond 16
HISTOGRAM_WORKERS = 16
SCALE = 0.25
_F32, _F64 = np.float32, np.float64


def _log(*a):
    _deps.logger().log(*a)


# ---------------------------------------------------------------------------------------------
# one pass over the survey's frames: histograms, and / or the frames themselves for the sum
# ---------------------------------------------------------------------------------------------
def _decode_frame(data):
    """file bytes -> BGR uint8 [h,w,3] on the device (the host decoder for what the split one refuses)"""
    from . import image as _image, kernels
    frame = kernels.jpeg_decode(data)
    if frame is None:
        frame = kernels._dev(_image._decode_bgr(io.BytesIO(data), writable=False), kernels.U8)
        kernels.wait_stream()                              # (the upload's staging copy has been read)
    return frame


def _histogram_of(frame, scale):
    """device frame -> three float32 [256] arrays, channel order 0, 1, 2"""
    from . import kernels, panda3d
    small = kernels.equalize_resize(frame, scale, equalize=False)
    hist = kernels.colour_histogram(small)
    pin = panda3d._pinned_take(hist.numel() * 4)
    try:
        pin.copy_(hist.view(kernels.U8).reshape(-1), non_blocking=True)
        kernels.wait_stream()
        counts = pin.numpy().view(np.uint32).reshape(3, 256).astype(_F32)
    finally:
        panda3d._pinned_give(pin)
    return counts[0].copy(), counts[1].copy(), counts[2].copy()


class _Job(object):
    __slots__ = ('image', 'device', 'scale', 'want_hist', 'keep_frame', 'stop')

    def __init__(self, image, device, scale, want_hist, keep_frame, stop):
        self.image, self.device, self.scale = image, device, scale
        self.want_hist, self.keep_frame, self.stop = want_hist, keep_frame, stop


def _frame_job(job):
    """worker: one file -> (histogram or None, device frame or None, event or None)"""
    import torch
    from . import image as _image, kernels
    if job.stop.is_set():
        return None
    with open(job.image.image_file, 'rb') as fp:
        data = fp.read()
    with torch.cuda.device(job.device), torch.cuda.stream(_image._worker_stream()), kernels.polite_waits():
        frame = _decode_frame(data)
        hist = _histogram_of(frame, job.scale) if job.want_hist else None
        if not job.keep_frame:
            return hist, None, None
        ev = torch.cuda.Event()
        ev.record()
        return hist, frame, ev


def frame_pass(image_list, want_hist=True, on_frames=None, scale=SCALE, batch=8):
    """Decode every image of image_list once on worker threads.  want_hist: histograms[name] is set
    for each.  on_frames(list of device frames): called on this thread's stream with up to `batch`
    decoded frames at a time, in list order (the vignette sum)."""
    import torch
    from . import cacheio, kernels
    from ._lib import require_gpu
    if not image_list:
        return
    device = require_gpu()
    stop = threading.Event()
    jobs = [_Job(im, device, scale, want_hist, on_frames is not None, stop) for im in image_list]
    pf = cacheio.Prefetch(_frame_job, jobs, max(1, min(HISTOGRAM_WORKERS, 16, len(jobs))))
    held = []

    def flush():
        if held:
            here = torch.cuda.current_stream()
            for frame, ev in held:
                here.wait_event(ev)
                frame.record_stream(here)                  # (allocated on a worker's stream)
            on_frames([f for f, _ in held])
            del held[:]
    try:
        for job in jobs:
            hist, frame, ev = pf.take(job)
            if want_hist:
                histograms[job.image.name] = hist
            if frame is not None:
                held.append((frame, ev))
                if len(held) >= batch:
                    flush()
        flush()
        if on_frames is not None:
            kernels.wait_stream()
    finally:
        stop.set()
        pf.close()
        pf.workers.shutdown(wait=True)


def get_histogram_rgb(image, scale=0.25):
    """the three float32 histograms of the image's file shrunk by `scale` (the reference names them
    g, b, r; they are channels 0, 1, 2 of the decoded frame)"""
    from . import kernels
    from ._lib import require_gpu
    print(image.name)
    require_gpu()
    with open(image.image_file, 'rb') as fp:
        data = fp.read()
    with kernels.polite_waits():
        return _histogram_of(_decode_frame(data), scale)


def make_histograms(image_list):
    print("Generating individual histograms...")
    frame_pass(image_list, want_hist=True)


# ---------------------------------------------------------------------------------------------
# templates (host)
# ---------------------------------------------------------------------------------------------
def _neighbour_candidates(ned, dist_cutoff):
    """per image the ascending indices of every image that CAN lie within dist_cutoff (a superset:
    the radius is padded far beyond the rounding of the distance; the reference's own test decides)"""
    from scipy.spatial import cKDTree
    pts = np.asarray(ned, _F64).reshape(-1, 3)
    if len(pts) == 0:
        return []
    finite = np.isfinite(pts).all(axis=1)
    if not finite.all() or not np.isfinite(dist_cutoff):
        return [list(range(len(pts)))] * len(pts)          # (nothing to prune with)
    pad = float(dist_cutoff) * (1.0 + 1e-9) + 1e-9 * (1.0 + float(np.abs(pts).max()))
    tree = cKDTree(pts)
    return [sorted(c) for c in tree.query_ball_point(pts, max(pad, 0.0))]


def make_templates(image_list, dist_cutoff=40, self_weight=0.1):
    """the reference's templates, bit for bit.  What numpy 2 makes of histogram.py:62-96, written out:
      weight          the int 1 within 1 m, else the float64 1 / dist_m
      hist * 1        float32;   hist * float64 -> float64
      src += rhs      keeps src's dtype: a float32 src (first neighbour within 1 m) takes a float64
                      rhs as float32(float64(src) + rhs)
      src_weights     a Python float until a float64 weight is added, then float64
      self weight     self_weight * src_weights: a Python float multiplies the float32 histogram as
                      a float32; a float64 makes a float64 product
      src / weights   float32 / Python float: float32 (0/0 = NaN for an image without neighbour);
                      anything / float64: float64
      cumsum, /=      in the dtype that arrives"""
    print("Computing histogram templates:")
    poses = [im.get_camera_pose()[0] for im in image_list]
    cand = _neighbour_candidates(poses, dist_cutoff)
    for i, i1 in enumerate(image_list):
        print(i1.name)
        src = None
        src_weights = 0.0
        wide = False                                       # src_weights has become a float64
        ned1 = poses[i]
        for j in cand[i]:
            if i == j:
                continue
            i2 = image_list[j]
            diff = np.array(poses[j]) - np.array(ned1)
            dist_m = np.linalg.norm(diff)
            if dist_m > dist_cutoff:
                continue
            h = histograms[i2.name]
            if dist_m <= 1:
                weight = 1
                if src is None:
                    src = [np.array(h[k], dtype=_F32) for k in range(3)]
                else:
                    for k in range(3):                     # float32 += float32, or float64 += float32
                        src[k] += np.asarray(h[k], _F32)
            else:
                weight = 1 / dist_m
                wide = True
                rhs = [np.asarray(h[k], _F32).astype(_F64) * _F64(weight) for k in range(3)]
                if src is None:
                    src = rhs
                else:
                    for k in range(3):
                        if src[k].dtype == _F64:
                            src[k] += rhs[k]
                        else:
                            src[k] = (src[k].astype(_F64) + rhs[k]).astype(_F32)
            src_weights += weight
        # include ourselves at some relative weight to the surrounding pairs
        weight = self_weight * src_weights
        h = histograms[i1.name]
        if wide:
            rhs = [np.asarray(h[k], _F32).astype(_F64) * _F64(weight) for k in range(3)]
        else:
            rhs = [np.asarray(h[k], _F32) * _F32(weight) for k in range(3)]
        if src is None:
            src = rhs
        else:
            for k in range(3):
                if src[k].dtype == rhs[k].dtype or src[k].dtype == _F64:
                    src[k] += rhs[k]
                else:
                    src[k] = (src[k].astype(_F64) + rhs[k]).astype(_F32)
        src_weights += weight
        out = []
        with np.errstate(invalid='ignore', divide='ignore'):
            for k in range(3):
                # normalize
                if wide:
                    s = src[k].astype(_F64) / _F64(src_weights)
                else:
                    s = src[k] / _F32(src_weights)
                # cumulative sums (normalized)
                q = np.cumsum(s)
                q /= q[-1]
                out.append(q)
        templates[i1.name] = tuple(out)


# ---------------------------------------------------------------------------------------------
# matching
# ---------------------------------------------------------------------------------------------
def lookup_tables(image_name):
    """uint8 [3, 256]: the reference's interp_*_values truncated to uint8, or None when the image's
    template is NaN"""
    lut = np.zeros((3, 256), np.uint8)
    for k in range(3):
        t = templates[image_name][k]
        if np.isnan(t).any():
            return None
        q = np.cumsum(histograms[image_name][k])
        q /= q[-1]
        lut[k] = np.interp(q, t, np.arange(256)).astype('uint8')
    return lut


def match_neighbors(rgb, image_name):
    """the image with each channel's quantiles moved onto the template's.  rgb: uint8 [h,w,3], numpy
    (a numpy array comes back) or a device tensor (a device tensor comes back)."""
    from . import kernels
    lut = lookup_tables(image_name)
    if lut is None:
        _log("histogram: no neighbour template for", image_name, "(image left as it is)")
        return rgb
    return kernels.colour_lut(rgb, lut)


def load(analysis_dir):
    global histograms
    global templates
    hist_file = os.path.join(analysis_dir, "histogram")
    if os.path.isfile(hist_file):
        _log("Loading histogram templates:", hist_file)
        with open(hist_file, "rb") as fp:
            (histograms, templates) = pickle.load(fp)
        return True
    else:
        _log("no histogram templates found...")
        return False


def save(analysis_dir):
    hist_file = os.path.join(analysis_dir, "histogram")
    with open(hist_file, "wb") as fp:
        pickle.dump((histograms, templates), fp)


def install(ref_histogram_module):
    """Give the reference's lib.histogram the device functions (drop-in).  The two dicts stay this
    module's: the reference's load() rebinds its own globals, so load / save are replaced too and
    the explorer's calls (histogram.load, histogram.match_neighbors) all land here."""
    for name in ('get_histogram_rgb', 'make_histograms', 'make_templates', 'match_neighbors', 'load', 'save'):
        setattr(ref_histogram_module, name, globals()[name])
