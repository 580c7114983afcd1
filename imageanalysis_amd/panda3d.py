"""MI355X-native stand-in for the reference's scripts/lib/panda3d.py:

    make_textures_opencv(src_dir, analysis_dir, image_list, resolution=512)     panda3d.py:24-74
    generate_from_grid(proj, group, ref_image, src_dir, analysis_dir, resolution)  panda3d.py:77-144

make_textures_opencv is the first and heaviest thing Step 5 ("Create the map") does: every
full-resolution JPEG of the project is decoded, shrunk to resolution x resolution with
cv2.resize(INTER_AREA) and written as <analysis_dir>/models/<image.name>.JPG, plus a 64 x 64
models/dummy.jpg from the first image.  generate_from_grid calls it and then writes
models/<root>.egg for every image of the group from image.grid_list / image.distorted_uv (the ray /
surface grids of render_panda3d.build_map), byte for byte the reference's files.

Here the decode is the split JPEG decoder (bit-identical to libjpeg-turbo, kernels.jpeg_decode),
the downscale is csrc/image_area.hip (kernels.resize_area) and only the 0.8 MB texture comes back
to the host, where Pillow encodes it.  Worker threads (the pattern of image.prefetch: one stream
per worker, polite waits, the caller's device) each take a file from its bytes to its texture.
Files the split decoder does not handle (progressive, CMYK, ...) are decoded on the host and go
through the same kernel; a greyscale file stays one channel and becomes a grey JPEG, as
cv2.imread(IMREAD_ANYCOLOR) + cv2.imwrite make it.

The encoder: Pillow, quality 95, 4:2:0, standard tables -- cv2.imwrite's defaults as far as they
can be stated.  The file BYTES against OpenCV's are unpinned (cv2 is not available to compare
with), like the resize itself (tests/area_restatement.py lists the convention and the departures).

Use `install(lib.panda3d)` to give the reference's module this function (drop-in).
"""
import io
import os
import threading
import time
from math import sqrt

import numpy as np

from . import _deps, cacheio, image as _image

# where the JPEG Huffman decode of a texture's source runs: 'device' (kernels.jpeg_device_decode,
# the host half for the files it refuses) or 'host'.  'host' until an A/B with repeats says otherwise:
# profiles/r10_texture_rate.txt holds one 24-frame run only (no spread), and 'host' has the mileage.
TEXTURE_ENTROPY = 'host'
# worker threads of one make_textures_opencv call (each holds one decoded frame, 60 MB at 20 MP,
# on the device); sized like image.PREFETCH_DEPTH, never beyond 16
TEXTURE_WORKERS = min(16, _image.PREFETCH_DEPTH)
DUMMY_RESOLUTION = 64
JPEG_QUALITY = 95
JPEG_SUBSAMPLING = '4:2:0'
TIME_STAGES = False            # True: wait for the resize kernel on its own (tools/texture_rate.py's split)

# files written / found in place / decoded at all / decoded the host way (no split decoder), the
# frames per second of the last call that made a file, and worker seconds per stage
texture_stats = {'made': 0, 'skipped': 0, 'decoded': 0, 'host_decoded': 0, 'frames_per_s': 0.0,
                 'stage_s': {'read': 0.0, 'decode': 0.0, 'resize': 0.0, 'download': 0.0,
                             'encode': 0.0, 'write': 0.0}}
_stats_lock = threading.Lock()


def _log(*a):
    _deps.logger().log(*a)


def _qlog(*a):
    _deps.logger().qlog(*a)


def _count(**kw):
    with _stats_lock:
        for k, v in kw.items():
            texture_stats[k] += v


def _decode_host(data):
    """the host way, from the file's bytes: [h,w] for a greyscale file (IMREAD_ANYCOLOR keeps one
    channel), else image._decode_bgr's BGR [h,w,3]"""
    from PIL import Image as PILImage
    with PILImage.open(io.BytesIO(data)) as im:
        if im.mode == 'L':
            im.load()
            w, h = im.size
            return np.frombuffer(im.tobytes(), np.uint8).reshape(h, w)
    return _image._decode_bgr(io.BytesIO(data), writable=False)


def _is_grey(data):
    from PIL import Image as PILImage
    try:
        with PILImage.open(io.BytesIO(data)) as im:       # (reads the header only)
            return im.mode == 'L'
    except Exception:                                     # noqa: BLE001  (the decoder reports it)
        return False


def encode_jpeg(pixels):
    """uint8 BGR [h,w,3] or grey [h,w] -> the bytes of the texture file"""
    from PIL import Image as PILImage
    if pixels.ndim == 2:
        im = PILImage.fromarray(np.ascontiguousarray(pixels), 'L')
    else:
        im = PILImage.fromarray(np.ascontiguousarray(pixels[:, :, ::-1]), 'RGB')
    buf = io.BytesIO()
    im.save(buf, format='JPEG', quality=JPEG_QUALITY, subsampling=JPEG_SUBSAMPLING)
    return buf.getvalue()


def _write_atomic(dst, data):
    """a killed run must not leave a half file that the exists-check then skips for good"""
    tmp = '%s.%d.%d.tmp' % (dst, os.getpid(), threading.get_ident())
    try:
        with open(tmp, 'wb') as fp:
            fp.write(data)
        os.replace(tmp, dst)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


_pinned_free = {}               # nbytes -> free page-locked download buffers, kept for the process


def _pinned_take(nbytes):
    """a page-locked download buffer (page-locking costs about a millisecond: the worker threads
    are new in every call, the buffers are not)"""
    import torch
    with _stats_lock:
        free = _pinned_free.get(nbytes)
        if free:
            return free.pop()
    return torch.empty(nbytes, dtype=torch.uint8).pin_memory()


def _pinned_give(buf):
    with _stats_lock:
        free = _pinned_free.setdefault(buf.numel(), [])
        if len(free) < 16:
            free.append(buf)


class _Job(object):
    __slots__ = ('src', 'outputs', 'device', 'entropy', 'stop')

    def __init__(self, src, outputs, device, entropy, stop):
        self.src, self.outputs, self.device = src, outputs, device
        self.entropy, self.stop = entropy, stop


def _texture_job(job):
    """worker: one source file -> its textures, job.outputs = [(dst, resolution), ...]"""
    import torch
    from . import kernels
    if job.stop.is_set():
        return False
    clock = time.perf_counter
    stage = dict.fromkeys(texture_stats['stage_s'], 0.0)
    t = clock()
    with open(job.src, 'rb') as fp:
        data = fp.read()
    stage['read'] = clock() - t
    host_way = False
    with torch.cuda.device(job.device), torch.cuda.stream(_image._worker_stream()), kernels.polite_waits():
        t = clock()
        frame = None if _is_grey(data) else kernels.jpeg_decode(data, entropy=job.entropy)
        if frame is None:
            host_way = True
            frame = _decode_host(data)
        h, w = int(frame.shape[0]), int(frame.shape[1])
        stage['decode'] = clock() - t
        for dst, res in job.outputs:
            if h < res or w < res:
                raise ValueError("%s: %d x %d is smaller than the %d x %d texture asked for"
                                 % (job.src, w, h, res, res))
        for dst, res in job.outputs:
            t = clock()
            # the reference's call: fx = resolution / float(width), fy = resolution / float(height)
            small = kernels.resize_area(frame, res / float(w), res / float(h))
            if TIME_STAGES:
                kernels.wait_stream()
            stage['resize'] += clock() - t
            t = clock()
            pin = _pinned_take(small.numel())
            try:
                pin.copy_(small.reshape(-1), non_blocking=True)
                kernels.wait_stream()
                pixels = pin.numpy().reshape(tuple(small.shape)).copy()
            finally:
                _pinned_give(pin)
            stage['download'] += clock() - t
            t = clock()
            blob = encode_jpeg(pixels)
            stage['encode'] += clock() - t
            t = clock()
            _write_atomic(dst, blob)
            stage['write'] += clock() - t
    with _stats_lock:
        texture_stats['decoded'] += 1
        texture_stats['host_decoded'] += 1 if host_way else 0
        for k, v in stage.items():
            texture_stats['stage_s'][k] += v
    return True


def make_textures_opencv(src_dir, analysis_dir, image_list, resolution=512):
    """the reference's signature and result: models/<image.name>.JPG (resolution x resolution) for
    every image that has none yet, and models/dummy.jpg (64 x 64) from the first image's file"""
    if TEXTURE_ENTROPY not in ('host', 'device'):
        raise ValueError("TEXTURE_ENTROPY must be 'host' or 'device'")
    dst_dir = os.path.join(analysis_dir, 'models')
    if not os.path.exists(dst_dir):
        _log("Notice: creating texture directory =", dst_dir)
        os.makedirs(dst_dir, exist_ok=True)
    resolution = int(resolution)
    dummy = os.path.join(dst_dir, "dummy.jpg")
    want_dummy = len(image_list) > 0 and not os.path.exists(dummy)
    from ._lib import require_gpu
    stop = threading.Event()
    jobs, plan, device, planned = [], [], None, set()
    for k, im in enumerate(image_list):
        dst = os.path.join(dst_dir, im.name + '.JPG')
        # (a name listed twice: the reference's loop finds the first one's file and skips)
        outputs = [] if dst in planned or os.path.exists(dst) else [(dst, resolution)]
        planned.add(dst)
        made = len(outputs)
        if k == 0 and want_dummy:
            outputs.append((dummy, DUMMY_RESOLUTION))     # from the frame decoded for the texture
        job = None
        if outputs:
            if device is None:
                device = require_gpu()                    # the workers run on the caller's device
            job = _Job(im.image_file, outputs, device, TEXTURE_ENTROPY, stop)
            jobs.append(job)
        plan.append((im, dst, job, made))
    t0 = time.perf_counter()
    pf = cacheio.Prefetch(_texture_job, jobs, max(1, min(TEXTURE_WORKERS, 16, len(jobs))))
    n_made = 0
    try:
        for im, dst, job, made in plan:
            _log(im.image_file, '->', dst)
            if job is not None:
                pf.take(job)
            if made:
                n_made += 1
                _count(made=1)
                _qlog("Texture %dx%d %s" % (resolution, resolution, dst))
            else:
                _count(skipped=1)
        if image_list:
            _log("Dummy:", image_list[0].image_file, dummy)
            if want_dummy:
                _qlog("Texture %dx%d %s" % (DUMMY_RESOLUTION, DUMMY_RESOLUTION, dummy))
    finally:
        stop.set()                                        # (after an error: queued files are not started)
        pf.close()
        pf.workers.shutdown(wait=True)                    # ... and the running ones finish or clean up
    if n_made:
        dt = time.perf_counter() - t0
        with _stats_lock:
            texture_stats['frames_per_s'] = n_made / dt if dt > 0 else 0.0


_EGG_HEAD = "<CoordinateSystem> { Z-Up }\n\n<Texture> tex { \"dummy.jpg\" }\n\n<VertexPool> surface {\n"


def _uv_lines(distorted_uv, width, height):
    return ["    <UV> { %.5f %.5f }\n  }\n" % (uv[0]/float(width), 1.0-uv[1]/float(height))
            for uv in distorted_uv]


def egg_text(grid_list, uv_lines):
    """the text of one .egg file (panda3d.py:92-137) and its polygon count; uv_lines = _uv_lines()"""
    steps = int(sqrt(len(grid_list))) - 1
    side = steps + 1
    out = [_EGG_HEAD]
    nan = set()
    for n in range(1, side * side + 1):
        v = grid_list[n-1]
        if v[0] != v[0] or v[1] != v[1] or v[2] != v[2]:
            v = [0.0, 0.0, 0.0]
            nan.add(n)
        out.append("  <Vertex> %d {\n    %.2f %.2f %.2f\n" % (n, v[0], v[1], v[2]))
        out.append(uv_lines[n-1])
    out.append("}\n\n<Group> surface {\n")
    count = 0
    for j in range(steps):
        for i in range(steps):
            c = (j * side) + i + 1
            d = ((j+1) * side) + i + 1
            if nan and (c in nan or d in nan or (c+1) in nan or (d+1) in nan):
                continue
            out.append("  <Polygon> {\n   <TRef> { tex }\n   <Normal> { 0 0 1 }\n"
                       "   <VertexRef> { %d %d %d %d <Ref> { surface } }\n  }\n" % (d, d+1, c+1, c))
            count += 1
    out.append("}\n")
    return "".join(out), count


def generate_from_grid(proj, group, ref_image=False, src_dir=".", analysis_dir=".", resolution=512):
    """The reference's generate_from_grid: the textures (if needed), then models/<root>.egg per image
    of the group -- "dummy.jpg" as the texture name, %.2f / %.5f numbers, NaN vertices written as
    zeros and the polygons that touch one left out, a file without a polygon removed (with the
    reference's warning), an image with an empty grid_list skipped.  Each file's text is built in
    memory and written once (the reference: ~500 f.write calls per file); one host thread writes
    1 000 files in 0.07 s (profiles/r11_step5_grid_rate.txt: 10 000 files in under a second), so
    there are no worker threads."""
    make_textures_opencv(src_dir, analysis_dir, proj.image_list, resolution)
    camera = _deps.camera()
    uv_cache = {}                                         # build_map gives a group ONE distorted_uv list
    for name in group:
        image = proj.findImageByName(name)
        if len(image.grid_list) == 0:
            continue
        root, ext = os.path.splitext(image.name)
        name = os.path.join(analysis_dir, "models", root + ".egg")
        _log("EGG file name:", name)
        width, height = camera.get_image_params()
        key = (id(image.distorted_uv), width, height)
        if key not in uv_cache:
            uv_cache[key] = (image.distorted_uv, _uv_lines(image.distorted_uv, width, height))
        text, count = egg_text(image.grid_list, uv_cache[key][1])
        if count == 0:
            # no polygon fully on the surface: the reference writes the file, warns and deletes it
            _log("Warning: no polygons fully on surface, removing:", name)
            if os.path.exists(name):
                os.remove(name)
            continue
        with open(name, "w") as f:
            f.write(text)


def install(ref_panda3d_module):
    """Give the reference's lib.panda3d the device texture maker (drop-in)."""
    ref_panda3d_module.make_textures_opencv = make_textures_opencv
