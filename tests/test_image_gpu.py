"""GPU: image preparation kernels and the Image.detect_features mirror (decode -> CLAHE ->
resize -> SIFT -> reference cache formats) against the oracle."""
import gzip
import os
import pickle

import numpy as np
import pytest

from test_sift_gpu import texture, _match

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('shape,scale', [((96, 128), 0.4), ((101, 77), 0.5), ((240, 320), 1.0)])
def test_equalize_resize_equals_oracle(shape, scale):
    from imageanalysis_amd import kernels
    from oracle import image_oracle as io
    rng = np.random.default_rng(shape[0])
    img = texture(shape[0], shape[1], 1)
    img[..., 1] = np.roll(img[..., 1], 7, axis=1)          # colourful: exercise the hue path
    img[::5, ::7] = rng.integers(0, 256, img[::5, ::7].shape, dtype=np.uint8)
    want = io.resize_linear_u8(io.equalize_bgr(img), scale)
    got = kernels.equalize_resize(img, scale).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want)          # (stage by stage: test_image_prep_gpu.py)
    plain = kernels.equalize_resize(img, scale, equalize=False).cpu().numpy()
    assert np.array_equal(plain, io.resize_linear_u8(img, scale))


def test_detect_features_end_to_end(tmp_path):
    from PIL import Image as PILImage
    from imageanalysis_amd import image as iimg
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd.hostlib import camera
    from oracle import image_oracle as io
    from oracle import sift_oracle as so
    proj = tmp_path / 'proj'
    (proj / 'images').mkdir(parents=True)
    an = proj / 'ImageAnalysis'
    (an / 'cache').mkdir(parents=True)
    (an / 'meta').mkdir()
    rgb = texture(300, 400, 11)[:, :, ::-1]
    PILImage.fromarray(np.ascontiguousarray(rgb)).save(str(proj / 'images' / 'T001.JPG'), quality=95)
    getNode('/config/directories', True).setString('project_dir', str(proj))
    getNode('/config/detector', True).setString('detector', 'SIFT')
    camera.set_image_params(400, 300)
    im = iimg.Image(str(an), 'T001')
    assert im.image_file.endswith('T001.JPG')
    im.detect_features(0.5)
    assert im.num_features == len(im.kp_list) > 100
    assert im.des_list.dtype == np.float32 and im.des_list.shape == (len(im.kp_list), 128)
    assert im.get_size() == (400, 300)
    # the cache files are the reference's formats (image.py:192-217); they are written in the
    # background: a reader outside our loaders waits for them
    from imageanalysis_amd import cacheio
    cacheio.wait()
    with gzip.open(im.features_file, 'rb') as f:
        feats = pickle.load(f)
    assert isinstance(feats, list) and len(feats[0]) == 6 and len(feats[0][0]) == 2
    with gzip.open(im.desc_file, 'rb') as f:
        des = np.load(f)
    assert des.dtype == np.float32 and np.array_equal(des, im.des_list)
    im2 = iimg.Image(str(an), 'T001')
    im2.detect_features(0.5)                          # served from the cache
    assert len(im2.kp_list) == len(im.kp_list) and np.array_equal(im2.des_list, im.des_list)
    assert im2.kp_list[3].pt == im.kp_list[3].pt and im2.kp_list[3].octave == im.kp_list[3].octave
    # against the oracle chain on the same decoded pixels
    bgr = iimg._decode_bgr(im.image_file)
    kps, odes = so.detect_and_compute(io.resize_linear_u8(io.equalize_bgr(bgr), 0.5))
    got = np.array([[k.pt[0] * 0.5, k.pt[1] * 0.5, k.size, k.angle, k.response] for k in im.kp_list])
    octv = np.array([k.octave for k in im.kp_list], np.int64)
    pairs = _match(kps, kps[:, 5].astype(np.int64), got, octv)
    assert len(pairs) >= 0.97 * len(kps)
    dd = np.abs(odes[pairs[:, 0]].astype(int) - im.des_list[pairs[:, 1]].astype(int))
    assert (dd == 0).mean() > 0.97
    # wrong camera size -> quit(), like the reference (image.py:300-306)
    camera.set_image_params(401, 300)
    with pytest.raises(SystemExit):
        iimg.Image(str(an), 'T001').detect_features(0.5, use_cache=False)


def test_detection_on_prefetch_workers_equals_the_serial_loop(tmp_path):
    """prefetch(images, scale=...) runs whole detections on the worker threads, several at a
    time in separate detector slots: keypoints, descriptors and cache files must be exactly what
    one detect_features() after the other gives"""
    from PIL import Image as PILImage
    from imageanalysis_amd import cacheio, image as iimg
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd.hostlib import camera
    proj = tmp_path / 'proj'
    (proj / 'images').mkdir(parents=True)
    getNode('/config/directories', True).setString('project_dir', str(proj))
    getNode('/config/detector', True).setString('detector', 'SIFT')
    camera.set_image_params(640, 480)
    names = ['W%03d' % k for k in range(12)]
    for k, name in enumerate(names):
        rgb = texture(480, 640, 20 + k)[:, :, ::-1]
        PILImage.fromarray(np.ascontiguousarray(rgb)).save(str(proj / 'images' / (name + '.JPG')), quality=93)

    def project(tag):
        an = proj / ('ImageAnalysis_' + tag)
        (an / 'cache').mkdir(parents=True)
        (an / 'meta').mkdir()
        return [iimg.Image(str(an), n) for n in names]

    serial = project('serial')
    for im in serial:
        im.detect_features(0.5)
    workers = project('workers')
    pf = iimg.prefetch(workers, depth=8, scale=0.5)
    for im in workers:
        im.detect_features(0.5)
    pf.close()
    cacheio.wait()
    for a, b in zip(serial, workers):
        assert len(a.kp_list) == len(b.kp_list) > 200
        assert np.array_equal(a.des_list, b.des_list)
        assert [k.pt for k in a.kp_list[:50]] == [k.pt for k in b.kp_list[:50]]
        assert b.get_size() == (640, 480)
        with gzip.open(b.desc_file, 'rb') as f:
            assert np.array_equal(np.load(f), a.des_list)
        with gzip.open(a.features_file, 'rb') as fa, gzip.open(b.features_file, 'rb') as fb:
            assert fa.read() == fb.read()
    # asked for at another scale than the workers were told: detected again, not reused
    other = project('other')
    pf = iimg.prefetch(other[:2], depth=2, scale=0.5)
    other[0].detect_features(0.4)
    pf.close()
    ref = project('ref04')[0]
    ref.detect_features(0.4)
    assert len(other[0].kp_list) == len(ref.kp_list) and np.array_equal(other[0].des_list, ref.des_list)


def test_full_chain_overlapping_views(tmp_path):
    """JPEG -> Image.detect_features -> matcher.bidirectional_pair_matches on two overlapping
    views of one scene, the second flown on the opposite heading (turned 180 deg): the chain
    must return many matches and they must all obey the known view-to-view transform."""
    from PIL import Image as PILImage
    from imageanalysis_amd import image as iimg, matcher
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd.hostlib import camera
    proj = tmp_path / 'proj'
    (proj / 'images').mkdir(parents=True)
    an = proj / 'ImageAnalysis'
    (an / 'cache').mkdir(parents=True)
    (an / 'meta').mkdir()
    W, H, dx, dy = 800, 600, 210, 90
    scene = texture(H + dy, W + dx, 21)
    a = scene[:H, :W]
    b = np.ascontiguousarray(scene[dy:dy + H, dx:dx + W][::-1, ::-1])     # shifted, then 180 deg
    for name, arr in (('V001', a), ('V002', b)):
        PILImage.fromarray(np.ascontiguousarray(arr[:, :, ::-1])).save(
            str(proj / 'images' / (name + '.JPG')), quality=92)
    getNode('/config/directories', True).setString('project_dir', str(proj))
    matcher.detector_node.setString('detector', 'SIFT')
    matcher.detector_node.setFloat('scale', 0.5)
    matcher.matcher_node.setFloat('match_ratio', 0.75)
    matcher.matcher_node.setInt('min_pairs', 25)
    camera.set_image_params(W, H)
    matcher.configure()
    i1, i2 = iimg.Image(str(an), 'V001'), iimg.Image(str(an), 'V002')
    for im in (i1, i2):
        im.detect_features(0.5, use_cache=False)
        assert len(im.kp_list) > 500
    fwd, rev = matcher.bidirectional_pair_matches(i1, i2)
    assert len(fwd) >= 150 and rev == [[q, p] for p, q in fwd]
    p1 = np.array([i1.kp_list[p].pt for p, _ in fwd])
    p2 = np.array([i2.kp_list[q].pt for _, q in fwd])
    # scene point s: view a at s, view b at (W-1, H-1) - (s - (dx, dy))
    want = np.array([W - 1, H - 1]) - (p1 - [dx, dy])
    err = np.linalg.norm(p2 - want, axis=1)
    assert np.median(err) < 1.5 and (err < 4.0).mean() > 0.97, (np.median(err), (err < 4.0).mean())
    # and the batched find_matches path gives the same lists as the single-pair call
    (f2, r2, _a, _b), = matcher._match_batch([(i1, i2)], 0.75)
    assert f2 == fwd and r2 == rev
