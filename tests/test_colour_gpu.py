"""GPU: csrc/image_colour.hip against numpy restatements (histogram, frame sum and mean, radial
moments, fitted and finished mask, look-up), imageanalysis_amd.histogram against the reference's
own results (tests/golden/colour_scene.pkl.gz) and scripts/99-vignette.py end to end."""
import json
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import REPO
import test_colour_host as host

pytestmark = pytest.mark.gpu


def _bincount3(img):
    return np.stack([np.bincount(img[:, :, c].ravel(), minlength=256) for c in range(3)]).astype(np.int64)


def _counts(hist):
    return hist.cpu().numpy().view(np.uint32).astype(np.int64)


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(1, 1), (3, 5), (228, 342), (457, 683)])
def test_histogram_equals_bincount(h, w):
    import torch
    from imageanalysis_amd import kernels
    img = _noise(h, w, seed=h)
    img[: h // 2, :, 1] = 200                                 # long runs of one value in one channel
    assert np.array_equal(_counts(kernels.colour_histogram(img)), _bincount3(img))
    # a device tensor one byte into its allocation: the byte-wise loop
    flat = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), img.reshape(-1)])).cuda()
    assert np.array_equal(_counts(kernels.colour_histogram(flat[1:].view(h, w, 3))), _bincount3(img))


def test_histogram_of_flat_images_and_two_calls_add():
    import torch
    from imageanalysis_amd import kernels
    flat = np.empty((228, 342, 3), np.uint8)
    flat[:] = (7, 7, 250)
    hist = kernels.colour_histogram(flat)
    assert np.array_equal(_counts(hist), _bincount3(flat))
    other = _noise(61, 77, seed=2)
    assert kernels.colour_histogram(other, hist) is hist
    assert np.array_equal(_counts(hist), _bincount3(flat) + _bincount3(other))
    # one flat survey frame: a float counter would stop at 2^24
    frame = torch.full((3648, 5472, 3), 131, dtype=torch.uint8, device='cuda')
    got = _counts(kernels.colour_histogram(frame))
    assert got[:, 131].tolist() == [19961856] * 3 and got.sum() == 3 * 19961856


def _jpeg(path, pixels_rgb, **opt):
    from PIL import Image
    Image.fromarray(pixels_rgb, 'RGB').save(path, 'JPEG', quality=90, **opt)


def _chain_histogram(path):
    """the reference's chain on the host: decode, quarter-size bilinear image, bincount"""
    from imageanalysis_amd import image
    from oracle.image_oracle import resize_linear_u8
    small = resize_linear_u8(image._decode_bgr(path), 0.25)
    return _bincount3(small).astype(np.float32)


class _Img(object):
    def __init__(self, path, ned=(0.0, 0.0, 0.0)):
        self.image_file = path
        self.name = os.path.splitext(os.path.basename(path))[0]
        self.ned = ned

    def get_camera_pose(self):
        return list(self.ned), [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]


def test_get_histogram_rgb_on_a_jpeg_file(tmp_path):
    from imageanalysis_amd import histogram
    path = str(tmp_path / 'one.JPG')
    _jpeg(path, host.vignetted(456, 684, 340.0, 230.0, seed=1))
    got = histogram.get_histogram_rgb(_Img(path))
    assert len(got) == 3 and all(a.dtype == np.float32 and a.shape == (256,) for a in got)
    assert np.array_equal(np.stack(got), _chain_histogram(path))


@pytest.fixture(scope='module')
def gold():
    import gzip
    with gzip.open(host.GOLD, 'rb') as f:
        return pickle.load(f)


def test_histograms_of_the_golden_frames_equal_the_reference(gold):
    import torch
    from imageanalysis_amd import histogram
    for name in gold['names']:
        got = histogram._histogram_of(torch.from_numpy(gold['frames'][name]).cuda(), 0.25)
        for k in range(3):
            assert got[k].dtype == np.float32
            assert np.array_equal(got[k], gold['histograms'][name][k]), (name, k)


# ---------------------------------------------------------------------------------------------
# sum and mean
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 7, 9])
def test_accumulate_and_mean(n):
    import torch
    from imageanalysis_amd import _lib, kernels
    rng = np.random.default_rng(n)
    frames = [rng.integers(0, 256, (37, 53, 3), dtype=np.uint8) for _ in range(n)]
    frames[0][0, 0] = 255
    total = torch.zeros((37, 53, 3), dtype=torch.int32, device='cuda')
    assert kernels.colour_accumulate(total, [torch.from_numpy(f).cuda() for f in frames]) is total
    want = np.zeros((37, 53, 3), np.uint32)
    for f in frames:
        want += f
    assert np.array_equal(total.cpu().numpy().view(np.uint32), want)
    avg = kernels.colour_mean(total, n).cpu().numpy()
    assert np.array_equal(avg, (want.astype(np.float32) / np.float32(n)).astype(np.uint8))
    with pytest.raises(_lib.IamxError, match='65793'):
        kernels.colour_mean(total, 65794)


def test_accumulate_unaligned_frames_and_large_sums():
    import torch
    from imageanalysis_amd import kernels
    img = _noise(19, 23, seed=4)
    flat = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), img.reshape(-1)])).cuda()
    view = flat[3:].view(19, 23, 3)
    total = torch.full((19, 23, 3), 16777000, dtype=torch.int32, device='cuda')     # beyond a float's integers
    kernels.colour_accumulate(total, [view] * 10)
    assert np.array_equal(total.cpu().numpy().view(np.uint32), 16777000 + 10 * img.astype(np.uint32))


def test_one_pass_over_more_frames_than_two_launches_hold(tmp_path):
    """19 files on 16 workers: the sum is made in three launches, the histograms in the same pass"""
    from imageanalysis_amd import histogram, image, vignette
    frames = []
    for k in range(19):
        path = str(tmp_path / ('p%02d.JPG' % k))
        _jpeg(path, host.vignetted(64, 96, 40.0 + k, 30.0, seed=60 + k))
        frames.append(_Img(path))
    keep = histogram.histograms
    histogram.histograms = {}
    try:
        avg = vignette.average(frames, histograms=True).cpu().numpy()
        got = histogram.histograms
    finally:
        histogram.histograms = keep
    total = np.zeros((64, 96, 3), np.uint32)
    for f in frames:
        total += image._decode_bgr(f.image_file)
    assert np.array_equal(avg, (total.astype(np.float32) / np.float32(19)).astype(np.uint8))
    assert list(got) == [f.name for f in frames]
    for f in frames:
        assert np.array_equal(np.stack(got[f.name]), _chain_histogram(f.image_file)), f.name


# ---------------------------------------------------------------------------------------------
# radial moments and the fit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w,h', [(96, 64), (342, 228)])
def test_moments_and_fit(w, h):
    from imageanalysis_amd import kernels, vignette
    cu, cv = w / 2.0 - 3.3, h / 2.0 + 1.7
    img = host.vignetted(h, w, cu, cv, seed=w)
    m, R = kernels.colour_moments(img, cu, cv)
    m2, R2 = kernels.colour_moments(img, cu, cv)
    m, m2 = m.cpu().numpy(), m2.cpu().numpy()
    assert R == R2 and m.tobytes() == m2.tobytes()            # reproducible bit for bit
    want, Rw = host.numpy_moments(img, cu, cv)
    assert R == Rw
    rel = np.abs(m - want) / np.abs(want)
    print('moments: largest relative difference %.3g' % rel.max())
    assert rel.max() <= 1e-12
    coef = vignette.fit(img, cu, cv)
    d = host.curve_difference(coef, host.curve_fit_coefficients(img, cu, cv), h, w, cu, cv)
    print('%d x %d: the curves differ by at most %.3g grey levels' % (w, h, d))
    assert d <= host.FIT_BOUND


# ---------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------
def _finish(vmask):
    """99-vignette.py:142-149"""
    out = []
    for c in range(3):
        m = 255 - vmask[:, :, c]
        m -= np.amin(m)
        out.append(m)
    return np.dstack(out)


def test_nofit_mask_equals_the_restatement():
    import torch
    from imageanalysis_amd import kernels
    img = host.vignetted(229, 341, 170.0, 115.0, seed=8)
    img[5, 7] = (255, 3, 90)
    assert np.array_equal(kernels.colour_mask_finish(img).cpu().numpy(), _finish(img))
    assert np.array_equal(kernels.colour_mask_finish(torch.from_numpy(img).cuda()).cpu().numpy(), _finish(img))


COEF = np.array([[-2.1e-10, -1.9e-4, 201.3], [-4.4e-10, -1.1e-4, 179.6], [0.9e-10, -2.6e-4, 150.2]])


def test_fitted_mask_dither():
    from imageanalysis_amd import kernels
    h, w, cu, cv = 456, 684, 338.7, 229.7
    raw = kernels.colour_fit_mask(h, w, cu, cv, COEF, seed=11)
    fin = kernels.colour_mask_finish(raw).cpu().numpy()
    raw = raw.cpu().numpy()
    assert np.array_equal(fin, _finish(raw))
    v = raw.reshape(-1, 3).max(axis=0).astype(np.int64) - fin            # the finish undone
    assert np.array_equal(v, raw)
    y, x = np.mgrid[0:h, 0:w]
    dx, dy = x - cu, y - cv
    rad = np.sqrt(dx * dx + dy * dy)
    order = np.argsort(rad.ravel(), kind='stable')
    rings = np.array_split(order, 24)                                    # 12 996 pixels each
    assert min(len(r) for r in rings) >= 10000
    for c in range(3):
        a, b, c0 = COEF[c]
        xs = a*rad*rad*rad*rad + b*rad*rad + c0
        lo = np.floor(xs)
        fr = xs - lo
        up = v[:, :, c] - lo
        sure = (fr > 1e-3) & (fr < 1 - 1e-3)
        assert sure.mean() > 0.99
        assert np.isin(up[sure], (0, 1)).all()
        assert np.abs(up[~sure]).max(initial=0) <= 1
        for ring in rings:
            n, p = len(ring), fr.ravel()[ring].mean()
            share = up.ravel()[ring].mean()
            sd = np.sqrt(p * (1 - p) / n)
            assert abs(share - p) <= 4 * sd, (c, share, p, sd)
    again = kernels.colour_fit_mask(h, w, cu, cv, COEF, seed=11).cpu().numpy()
    assert np.array_equal(again, raw)
    other = kernels.colour_fit_mask(h, w, cu, cv, COEF, seed=12).cpu().numpy()
    assert (other != raw).mean() > 0.1


def test_a_polynomial_that_leaves_the_range_is_an_error():
    from imageanalysis_amd import kernels
    from imageanalysis_amd._lib import IamxError
    bad = COEF.copy()
    bad[1] = (0.0, 1e-3, 200.0)                              # 200 + 1e-3 r^2 passes 255 at r = 235
    with pytest.raises(IamxError, match='leaves'):
        kernels.colour_fit_mask(456, 684, 338.7, 229.7, bad)
    bad[1] = (2e-8, -4e-3, 180.0)                            # in range at the centre and the corner, -20 at r = 316
    with pytest.raises(IamxError, match='leaves'):
        kernels.colour_fit_mask(456, 684, 338.7, 229.7, bad)


# ---------------------------------------------------------------------------------------------
# look-up
# ---------------------------------------------------------------------------------------------
def _lut(seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8)


def _lut_want(img, lut, mask=None):
    out = np.dstack([lut[c][img[:, :, c]] for c in range(3)])
    if mask is not None:
        out = np.clip(out.astype(np.uint16) + mask, 0, 255).astype(np.uint8)
    return out


@pytest.mark.parametrize('h,w', [(1, 1), (5, 3), (229, 341), (457, 683)])
def test_lookup_numpy_and_device_inputs(h, w):
    import torch
    from imageanalysis_amd import kernels
    img, mask, lut = _noise(h, w, seed=w), _noise(h, w, seed=w + 1), _lut(h)
    got = kernels.colour_lut(img, lut)
    assert isinstance(got, np.ndarray) and np.array_equal(got, _lut_want(img, lut))
    assert np.array_equal(kernels.colour_lut(img, lut, mask), _lut_want(img, lut, mask))
    dev = kernels.colour_lut(torch.from_numpy(img).cuda(), lut, torch.from_numpy(mask).cuda())
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), _lut_want(img, lut, mask))
    flat = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), img.reshape(-1)])).cuda()
    dev = kernels.colour_lut(flat[1:].view(h, w, 3), torch.from_numpy(lut).cuda())
    assert np.array_equal(dev.cpu().numpy(), _lut_want(img, lut))


def test_lookup_on_a_survey_frame():
    import torch
    from imageanalysis_amd import kernels
    g = torch.Generator(device='cuda').manual_seed(3)
    img = torch.randint(0, 256, (3648, 5472, 3), dtype=torch.uint8, device='cuda', generator=g)
    mask = torch.randint(0, 64, (3648, 5472, 3), dtype=torch.uint8, device='cuda', generator=g)
    lut = _lut(20)
    got = kernels.colour_lut(img, lut, mask).cpu().numpy()
    assert np.array_equal(got, _lut_want(img.cpu().numpy(), lut, mask.cpu().numpy()))


@pytest.fixture
def hist(gold):
    from imageanalysis_amd import histogram
    keep = histogram.histograms, histogram.templates
    histogram.histograms = {k: tuple(a.copy() for a in v) for k, v in gold['histograms'].items()}
    histogram.templates = {k: tuple(a.copy() for a in v) for k, v in gold['templates'].items()}
    yield histogram
    histogram.histograms, histogram.templates = keep


def test_match_neighbors_equals_the_reference(gold, hist, capsys):
    import torch
    for name, want in gold['matched'].items():
        img = gold['frames'][name]
        got = hist.match_neighbors(img, name)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want), name
        dev = hist.match_neighbors(torch.from_numpy(img).cuda(), name)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    capsys.readouterr()
    img = gold['frames']['c3']                                # the NaN template: logged, unchanged
    assert hist.match_neighbors(img, 'c3') is img
    assert 'c3' in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
LIB_STANDIN = {
    '__init__.py': '',
    'camera.py': 'from imageanalysis_amd.hostlib.camera import *   # noqa: F401,F403\n',
    'project.py': textwrap.dedent('''\
        import json, os
        from imageanalysis_amd.hostlib import camera
        class Image(object):
            def __init__(self, rec):
                self.name, self.image_file, self.ned = rec['name'], rec['file'], rec['ned']
            def get_camera_pose(self):
                return list(self.ned), [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]
        class ProjectMgr(object):
            """stand-in: the frames, poses and camera of project.json"""
            def __init__(self, project_dir):
                self.analysis_dir = os.path.join(project_dir, 'ImageAnalysis')
                self._rec = json.load(open(os.path.join(project_dir, 'project.json')))
            def load_images_info(self):
                c = self._rec['camera']
                camera.set_K(c['fx'], c['fy'], c['cu'], c['cv'], optimized=True)
                camera.set_K(c['fx'], c['fy'], c['cu'], c['cv'])
                camera.set_image_params(c['width'], c['height'])
                self.image_list = [Image(r) for r in self._rec['images']]
        '''),
}


def test_script_end_to_end(tmp_path):
    from PIL import Image
    from imageanalysis_amd import image, panda3d
    lib = tmp_path / 'standin' / 'lib'
    lib.mkdir(parents=True)
    for name, text in LIB_STANDIN.items():
        (lib / name).write_text(text)
    proj = tmp_path / 'project'
    (proj / 'images').mkdir(parents=True)
    w, h, cu, cv = 342, 228, 169.4, 115.2
    ned = [(0, 0, -90), (0.5, 0, -90), (15, 8, -90), (30, 0, -90), (31, 0.2, -90), (300, 300, -90)]
    recs = []
    for k, p in enumerate(ned):
        path = str(proj / 'images' / ('f%d.JPG' % k))
        _jpeg(path, host.vignetted(h, w, cu, cv, seed=30 + k), subsampling='4:2:0' if k % 2 else '4:4:4')
        recs.append({'name': 'f%d' % k, 'file': path, 'ned': list(p)})
    (proj / 'project.json').write_text(json.dumps({
        'images': recs, 'camera': {'fx': 400.0, 'fy': 400.0, 'cu': cu, 'cv': cv, 'width': w, 'height': h}}))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / 'standin'), REPO]))
    script = os.path.join(REPO, 'imageanalysis_amd', 'scripts', '99-vignette.py')
    models = proj / 'ImageAnalysis' / 'models'
    avg_file, mask_file, hist_file = models / 'vignette-avg.jpg', models / 'vignette-mask.jpg', \
        proj / 'ImageAnalysis' / 'histogram'

    def run(*options):
        cmd = ['timeout', '-k', '10', '300', sys.executable, script, str(proj)] + list(options)
        p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stdout

    def check_histograms():
        with open(hist_file, 'rb') as f:
            histograms, templates = pickle.load(f)
        assert list(histograms) == [r['name'] for r in recs] == list(templates)
        for r in recs:
            assert np.array_equal(np.stack(histograms[r['name']]), _chain_histogram(r['file'])), r['name']
        assert np.isnan(templates['f5'][0]).all() and templates['f0'][0].dtype == np.float64
        assert templates['f0'][1][-1] == 1.0

    out = run('--histogram', '--scale', '0.5')
    assert 'Project cu = %.2f  cv = %.2f:' % (cu, cv) in out and 'blue fit coefficients:' in out
    assert avg_file.is_file() and mask_file.is_file() and hist_file.is_file()
    check_histograms()
    # the average: numpy's uint32 sum of the decoded frames, the reference's float32 division
    total = np.zeros((h, w, 3), np.uint32)
    for r in recs:
        total += image._decode_bgr(r['file'])
    avg = (total.astype(np.float32) / np.float32(len(recs))).astype(np.uint8)
    assert avg_file.read_bytes() == panda3d.encode_jpeg(avg)
    with Image.open(str(mask_file)) as im:
        assert im.size == (w, h) and im.mode == 'RGB'
    fitted = mask_file.read_bytes()
    stamp = avg_file.stat().st_mtime_ns
    os.remove(str(hist_file))
    # a second run, without the fit: the average stays, the mask is the decoded average's
    out = run('--histogram', '--nofit')
    assert 'fit coefficients' not in out
    assert avg_file.stat().st_mtime_ns == stamp and avg_file.read_bytes() == panda3d.encode_jpeg(avg)
    check_histograms()
    want = panda3d.encode_jpeg(_finish(image._decode_bgr(str(avg_file))))
    assert mask_file.read_bytes() == want and want != fitted
