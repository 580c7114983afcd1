"""GPU: kernels.resize_area against its numpy restatement bit for bit, and the texture maker
imageanalysis_amd.panda3d.make_textures_opencv end to end on small projects."""
import glob
import io
import os
import threading

import numpy as np
import pytest

import area_restatement as ar

pytestmark = pytest.mark.gpu


def _textured(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 96 + 80 * np.sin(x / 17.0 + seed) * np.cos(y / 23.0) + 40 * ((x // 5 + y // 7) % 2)
    img = base[:, :, None] + rng.normal(0, 35, (h, w, ch)) + rng.integers(-20, 20, ch)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img if ch == 3 else img[:, :, 0]


def _check(img, fx, fy, as_tensor=False):
    import torch
    from imageanalysis_amd import kernels
    src = torch.from_numpy(img).cuda() if as_tensor else img
    got = kernels.resize_area(src, fx, fy)
    assert got.is_cuda and got.dtype == torch.uint8
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = ar.resize_area(img, fx, fy)
    assert got.shape == want.shape
    bad = int((got != want).sum())
    print('%s fx=%.6f fy=%.6f -> %s: %d of %d values differ' % (img.shape, fx, fy, got.shape, bad, got.size))
    assert bad == 0
    return got


# (width, height, resolution, channels)
@pytest.mark.parametrize('w,h,r,ch', [(684, 456, 64, 3), (1000, 750, 64, 3), (342, 228, 32, 3),
                                      (684, 456, 64, 1), (512, 384, 64, 3)])
def test_kernel_equals_the_restatement(w, h, r, ch):
    _check(_textured(h, w, ch, seed=w + r), r / float(w), r / float(h))


@pytest.mark.parametrize('r', [512, 64])
def test_kernel_equals_the_restatement_on_a_survey_frame(r):
    rng = np.random.default_rng(r)
    img = _textured(3648, 5472, 3, seed=r)
    img[::2] ^= rng.integers(0, 64, (1824, 5472, 3), dtype=np.uint8)     # row-to-row contrast
    out = _check(img, r / float(5472), r / float(3648), as_tensor=True)
    assert out.shape == (r, r, 3)


def test_integer_ratio_branches():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (4096, 4096, 3), dtype=np.uint8)
    assert _check(img, 512 / float(4096), 512 / float(4096), as_tensor=True).shape == (512, 512, 3)
    small = rng.integers(0, 256, (300, 500, 3), dtype=np.uint8)
    _check(small, 0.5, 0.5)                                  # 2 x 2: (sum + 2) >> 2
    _check(small[:, :, 1].copy(), 0.5, 0.5)
    _check(rng.integers(0, 256, (301, 503, 3), dtype=np.uint8), 0.25, 0.25)   # blocks over the edge
    _check(rng.integers(0, 256, (303, 501, 1), dtype=np.uint8)[:, :, 0], 0.5, 0.5)
    # the largest block the entry point admits: 4096 x 4096 x 255 does not fit a signed 32-bit sum
    assert _check(np.full((4096, 4096), 255, np.uint8), 1 / 4096.0, 1 / 4096.0)[0, 0] == 255


def test_device_and_numpy_inputs_odd_shapes_and_alignment():
    import torch
    from imageanalysis_amd import kernels
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (457, 683, 3), dtype=np.uint8)            # rows not 16-byte multiples
    a = _check(img, 64 / 683.0, 64 / 457.0)
    b = _check(img, 64 / 683.0, 64 / 457.0, as_tensor=True)
    assert np.array_equal(a, b)
    _check(img, 1.0, 1.0)                                    # scale 1: a copy through the integer branch
    _check(img, 0.999, 0.7)                                  # scale just above 1
    _check(img, 1 / 170.5, 1 / 114.0)                        # long rows of taps, one an integer
    _check(rng.integers(0, 256, (97, 131), dtype=np.uint8), 0.3, 0.41)
    # a device tensor that starts one byte into its allocation
    flat = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), img.reshape(-1)])).cuda()
    view = flat[1:].view(457, 683, 3)
    got = kernels.resize_area(view, 0.31, 0.27).cpu().numpy()
    assert np.array_equal(got, ar.resize_area(img, 0.31, 0.27))
    with pytest.raises(Exception):
        kernels.resize_area(img, 1.5, 0.5)


# ---------------------------------------------------------------------------------------------
class _Img(object):
    def __init__(self, path):
        self.image_file = path
        self.name = os.path.splitext(os.path.basename(path))[0]


def _project(tmp_path, tag='p'):
    """4:2:0, 4:2:2, progressive and greyscale JPEGs of different sizes"""
    from PIL import Image
    src = tmp_path / (tag + '_images')
    src.mkdir()
    specs = [('a420', 1216, 800, dict(subsampling='4:2:0')),
             ('b422', 1000, 750, dict(subsampling='4:2:2')),
             ('cprog', 900, 700, dict(subsampling='4:2:0', progressive=True)),
             ('dgrey', 1024, 768, None),
             ('e444', 777, 601, dict(subsampling='4:4:4'))]
    images = []
    for k, (name, w, h, opt) in enumerate(specs):
        path = str(src / (name + '.JPG'))
        if opt is None:
            Image.fromarray(_textured(h, w, 1, seed=k), 'L').save(path, 'JPEG', quality=90)
        else:
            Image.fromarray(_textured(h, w, 3, seed=k), 'RGB').save(path, 'JPEG', quality=90, **opt)
        images.append(_Img(path))
    return str(src), images


def _expected_bytes(path, resolution):
    """Pillow's encoding (quality 95, 4:2:0, standard tables) of restatement(_decode_bgr(file));
    a greyscale file: of its one channel, as a grey JPEG"""
    from PIL import Image
    from imageanalysis_amd import image
    bgr = image._decode_bgr(path)
    h, w = bgr.shape[:2]
    with Image.open(path) as im:
        grey = im.mode == 'L'
    buf = io.BytesIO()
    if grey:
        small = ar.resize_area(np.ascontiguousarray(bgr[:, :, 0]), resolution / float(w), resolution / float(h))
        Image.fromarray(small, 'L').save(buf, format='JPEG', quality=95, subsampling='4:2:0')
    else:
        small = ar.resize_area(bgr, resolution / float(w), resolution / float(h))
        Image.fromarray(np.ascontiguousarray(small[:, :, ::-1]), 'RGB').save(
            buf, format='JPEG', quality=95, subsampling='4:2:0')
    return buf.getvalue()


def _check_models(an, images, resolution):
    from PIL import Image
    models = os.path.join(an, 'models')
    for im in images:
        dst = os.path.join(models, im.name + '.JPG')
        assert os.path.isfile(dst), dst
        with Image.open(dst) as t:
            assert t.size == (resolution, resolution)
            with Image.open(im.image_file) as s:
                assert t.mode == ('L' if s.mode == 'L' else 'RGB')
        assert open(dst, 'rb').read() == _expected_bytes(im.image_file, resolution), im.name
    dummy = os.path.join(models, 'dummy.jpg')
    with Image.open(dummy) as t:
        assert t.size == (64, 64)
    assert open(dummy, 'rb').read() == _expected_bytes(images[0].image_file, 64)
    assert not glob.glob(os.path.join(models, '*.tmp'))


@pytest.fixture
def entropy_switch():
    from imageanalysis_amd import panda3d
    keep = panda3d.TEXTURE_ENTROPY
    yield panda3d
    panda3d.TEXTURE_ENTROPY = keep


def test_end_to_end_project_both_decode_routes(tmp_path, entropy_switch):
    from imageanalysis_amd import kernels
    panda3d = entropy_switch
    src, images = _project(tmp_path)
    files = {}
    for route in ('host', 'device'):
        panda3d.TEXTURE_ENTROPY = route
        an = str(tmp_path / ('analysis_' + route))
        os.makedirs(an)
        before = dict(panda3d.texture_stats)
        on_device = kernels.jpeg_device_stats['device']
        panda3d.make_textures_opencv(src, an, images, resolution=256)
        _check_models(an, images, 256)
        after = panda3d.texture_stats
        # the three baseline colour files went through the device entropy decoder, or none did
        assert kernels.jpeg_device_stats['device'] - on_device == (3 if route == 'device' else 0)
        assert after['made'] - before['made'] == len(images)
        assert after['decoded'] - before['decoded'] == len(images)
        assert after['host_decoded'] - before['host_decoded'] == 2        # progressive and greyscale
        assert after['frames_per_s'] > 0
        files[route] = {f: open(os.path.join(an, 'models', f), 'rb').read()
                        for f in sorted(os.listdir(os.path.join(an, 'models')))}
    assert set(files['host']) == set(im.name + '.JPG' for im in images) | {'dummy.jpg'}
    assert files['host'] == files['device']


def test_second_call_decodes_nothing_and_foreign_files_stay(tmp_path):
    from imageanalysis_amd import panda3d
    src, images = _project(tmp_path)
    an = str(tmp_path / 'analysis')
    models = os.path.join(an, 'models')
    os.makedirs(models)
    foreign = os.path.join(models, images[1].name + '.JPG')
    with open(foreign, 'wb') as fp:
        fp.write(b'not ours')
    panda3d.make_textures_opencv(src, an, images, resolution=128)
    assert open(foreign, 'rb').read() == b'not ours'
    rest = [im for im in images if im is not images[1]]
    for im in rest:
        assert open(os.path.join(models, im.name + '.JPG'), 'rb').read() == _expected_bytes(im.image_file, 128)
    stamp = {f: os.stat(os.path.join(models, f)).st_mtime_ns for f in os.listdir(models)}
    before = dict(panda3d.texture_stats)
    panda3d.make_textures_opencv(src, an, images, resolution=128)
    after = panda3d.texture_stats
    assert after['decoded'] == before['decoded'] and after['made'] == before['made']
    assert after['host_decoded'] == before['host_decoded']
    assert after['skipped'] - before['skipped'] == len(images)
    assert stamp == {f: os.stat(os.path.join(models, f)).st_mtime_ns for f in os.listdir(models)}
    # a missing dummy alone is made again, from the first image's file
    os.remove(os.path.join(models, 'dummy.jpg'))
    panda3d.make_textures_opencv(src, an, images, resolution=128)
    assert open(os.path.join(models, 'dummy.jpg'), 'rb').read() == _expected_bytes(images[0].image_file, 64)
    assert panda3d.texture_stats['made'] == after['made']


def test_a_frame_smaller_than_the_resolution_is_an_error(tmp_path):
    from PIL import Image
    from imageanalysis_amd import panda3d
    src, images = _project(tmp_path)
    tiny = os.path.join(src, 'tiny.JPG')
    Image.fromarray(_textured(200, 300, 3, seed=1), 'RGB').save(tiny, 'JPEG', quality=90)
    images.insert(2, _Img(tiny))
    an = str(tmp_path / 'analysis')
    with pytest.raises(ValueError, match='tiny.JPG'):
        panda3d.make_textures_opencv(src, an, images, resolution=256)
    models = os.path.join(an, 'models')
    assert not glob.glob(os.path.join(models, '*.tmp'))
    assert not os.path.exists(os.path.join(models, 'tiny.JPG'))
    for f in os.listdir(models):                              # what was written is whole
        with Image.open(os.path.join(models, f)) as t:
            t.load()


def test_two_threads_two_directories(tmp_path):
    import torch
    from imageanalysis_amd import panda3d
    torch.cuda.synchronize()
    projects = [(_project(tmp_path, 'p%d' % k), str(tmp_path / ('analysis%d' % k))) for k in range(2)]
    errors = []

    def run(k):
        try:
            (src, images), an = projects[k]
            panda3d.make_textures_opencv(src, an, images, resolution=128 if k else 192)
        except Exception as e:                                # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, ((src, images), an) in enumerate(projects):
        _check_models(an, images, 128 if k else 192)


def test_reference_log_lines(tmp_path, capsys):
    from imageanalysis_amd import panda3d
    src, images = _project(tmp_path)
    an = str(tmp_path / 'analysis')
    panda3d.make_textures_opencv(src, an, images[:2], resolution=128)
    out = capsys.readouterr().out
    models = os.path.join(an, 'models')
    assert 'Notice: creating texture directory = ' + models in out
    assert '%s -> %s' % (images[0].image_file, os.path.join(models, images[0].name + '.JPG')) in out
    assert 'Dummy: %s %s' % (images[0].image_file, os.path.join(models, 'dummy.jpg')) in out


def test_a_name_listed_twice_is_made_once(tmp_path):
    from imageanalysis_amd import panda3d
    src, images = _project(tmp_path)
    an = str(tmp_path / 'analysis')
    before = dict(panda3d.texture_stats)
    panda3d.make_textures_opencv(src, an, [images[0], images[1], images[0]], resolution=128)
    after = panda3d.texture_stats
    assert after['made'] - before['made'] == 2 and after['decoded'] - before['decoded'] == 2
    assert after['skipped'] - before['skipped'] == 1
    _check_models(an, images[:2], 128)
