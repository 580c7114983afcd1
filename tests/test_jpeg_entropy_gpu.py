"""GPU: the device JPEG entropy decoder (csrc/jpeg_entropy.hip) against the host half
(iamx_jpeg_decode_coefficients): every coefficient equal, the status "synchronised", and the
pixels after iamx_jpeg_reconstruct equal to libjpeg-turbo's (Pillow), on the files the CPU suite
(tests/test_jpeg_entropy.py) runs through the host driver of the same decode routine.  The damaged
inputs here are the two the CPU build has already survived under the sanitizers; no fuzzing on a
shared machine."""
import ctypes
import io
import threading

import numpy as np
import pytest

from test_jpeg import encode, host_decode, pillow_bgr
from test_jpeg_entropy import (DAMAGED, N_SYNC_FILES, NOT_SYNCED, SYNCED, flat_files, prepare,
                               sync_files)

pytestmark = pytest.mark.gpu


def device_decode(data, stream=None, guard=False):
    """the raw device call -> (status, passes, coef [blocks (+1 guard row), 64] numpy, info, quant)"""
    import torch
    from imageanalysis_amd import _lib
    from imageanalysis_amd.kernels import _ptr, stream_ptr
    L = _lib.lib()
    dev = _lib.require_gpu()
    rc, info, quant, header = prepare(data)
    assert rc == 0
    n = len(data)
    raw = np.zeros((n + 15) // 16 * 16, np.uint8)
    raw[:n] = np.frombuffer(bytes(data), np.uint8)
    blocks = int(info[11])
    need = int(L.iamx_jpeg_entropy_workspace_bytes(header.ctypes.data_as(ctypes.c_void_p)))
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d_raw = torch.from_numpy(raw).to(dev)
        d_header = torch.from_numpy(header).to(dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        coef = torch.full((blocks + 1, 64), 12345, dtype=torch.int16, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        rc = L.iamx_jpeg_entropy_decode(_ptr(d_raw), raw.size, header.ctypes.data_as(ctypes.c_void_p),
                                        _ptr(d_header), _ptr(ws), need, _ptr(coef), blocks, _ptr(status),
                                        stream_ptr())
        assert rc == 0, L.iamx_last_error()
        st = status.cpu().numpy()
        out = coef.cpu().numpy()
    assert (out[blocks] == 12345).all(), 'guard row behind the coefficients'
    return int(st[0]), int(st[1]), (out if guard else out[:blocks]), info, quant


@pytest.mark.parametrize('k', range(N_SYNC_FILES))
def test_device_coefficients_equal_host_half(k):
    from imageanalysis_amd import kernels
    name, data = sync_files()[k]
    rc, _info, want, _q = host_decode(data)
    assert rc == 0
    status, passes, coef, _i, _q2 = device_decode(data)
    print(name, 'passes', passes, 'status', status)
    assert status == SYNCED, (name, status, passes)
    assert coef.shape == want.shape and np.array_equal(coef, want), (name, int((coef != want).sum()))
    before = dict(kernels.jpeg_device_stats)
    got = kernels.jpeg_decode(data, entropy='device')
    assert kernels.jpeg_device_stats['device'] == before['device'] + 1
    want_px = pillow_bgr(data)
    got = got.cpu().numpy()
    assert got.shape == want_px.shape and np.array_equal(got, want_px), int((got != want_px).sum())


@pytest.mark.parametrize('sub', [1, 2])
def test_full_frame_20mp_device_entropy(sub):
    import torch
    from PIL import Image
    from imageanalysis_amd import kernels, synth
    img = synth.make_survey_image(seed=3).cpu().numpy()
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(buf, 'JPEG', quality=93, subsampling=sub)
    data = buf.getvalue()
    before = dict(kernels.jpeg_device_stats)
    jc = kernels.jpeg_device_decode(data)
    assert jc is not None, 'refused'
    assert kernels.jpeg_device_stats['device'] == before['device'] + 1
    assert kernels.jpeg_device_stats['refused'] == before['refused']
    print('passes (maximum so far)', kernels.jpeg_device_stats['passes'])
    rc, _info, want, quant = host_decode(data)
    assert rc == 0 and np.array_equal(jc.quant, quant)
    assert np.array_equal(jc.coef.cpu().numpy(), want)
    got = kernels.jpeg_reconstruct(jc)
    want_px = pillow_bgr(data)
    assert np.array_equal(got.cpu().numpy(), want_px)
    got2 = kernels.jpeg_decode(data, entropy='device')
    assert torch.equal(got, got2)
    a = kernels.equalize_resize(got, 0.4)
    b = kernels.equalize_resize(np.ascontiguousarray(want_px), 0.4)
    assert torch.equal(a, b)


@pytest.mark.parametrize('k', [0, 1])
def test_flat_files_decode_whichever_way_they_go(k):
    from imageanalysis_amd import kernels
    name, data = flat_files()[k]
    before = dict(kernels.jpeg_device_stats)
    got = kernels.jpeg_decode(data, entropy='device')
    after = dict(kernels.jpeg_device_stats)
    went = [key for key in ('device', 'refused') if after[key] == before[key] + 1]
    print(name, 'went', went)
    assert len(went) == 1 and after['unsupported'] == before['unsupported'] and after['damaged'] == before['damaged']
    want = pillow_bgr(data)
    assert np.array_equal(got.cpu().numpy(), want)
    status, _passes, coef, _i, _q = device_decode(data)
    assert status == (SYNCED if went == ['device'] else NOT_SYNCED)
    if status == NOT_SYNCED:
        assert not coef.any()
    else:
        assert np.array_equal(coef, host_decode(data)[2])


def test_unsupported_file_goes_the_host_way():
    from PIL import Image
    from imageanalysis_amd import kernels
    from test_jpeg import scene
    buf = io.BytesIO()
    Image.fromarray(scene(64, 64, 1)).save(buf, 'JPEG', quality=90, progressive=True)
    before = dict(kernels.jpeg_device_stats)
    assert kernels.jpeg_device_decode(buf.getvalue()) is None
    assert kernels.jpeg_device_stats['unsupported'] == before['unsupported'] + 1
    assert kernels.jpeg_decode(buf.getvalue(), entropy='device') is None
    with pytest.raises(ValueError):
        kernels.jpeg_decode(buf.getvalue(), entropy='gpu')


def test_truncated_file_and_one_mcu_restart_interval_stay_inside_the_buffer():
    """(both inputs pass tests/test_jpeg_entropy.py under the sanitizers first)"""
    data = encode((64, 64), 2, 90, {})
    cut = data[:len(data) // 3]
    rc, _info, want, _q = host_decode(cut)
    assert rc == 0
    status, _passes, coef, _i, _q2 = device_decode(cut, guard=True)      # (asserts the guard row)
    assert status == DAMAGED
    written = coef[:-1, 1:].any(axis=1)               # decoding stops where the data ends
    assert 0 < int(written.sum()) < int(want[:, 1:].any(axis=1).sum())
    # (the block the data ends in is the only one that may differ: the host half completes it from zero bits)
    assert np.array_equal(coef[0], want[0]) and int((coef[:-1][written][:, 1:] != want[written][:, 1:]).any(axis=1).sum()) <= 1
    from imageanalysis_amd import kernels
    before = dict(kernels.jpeg_device_stats)
    got = kernels.jpeg_decode(cut, entropy='device')                  # damaged -> the host half
    assert kernels.jpeg_device_stats['damaged'] == before['damaged'] + 1
    assert np.array_equal(got.cpu().numpy(), kernels.jpeg_decode(cut).cpu().numpy())
    data = encode((130, 97), 2, 88, dict(restart_marker_blocks=1))
    rc, _info, want, _q = host_decode(data)
    status, _passes, coef, _i, _q2 = device_decode(data, guard=True)
    assert rc == 0 and status == SYNCED and np.array_equal(coef[:-1], want)


def test_detect_features_with_device_entropy(tmp_path):
    """Image.detect_features on a JPEG file: same keypoints / descriptors with the Huffman decode
    on the device and on the host; and four frames through image.prefetch with the switch on"""
    from PIL import Image as PILImage
    from imageanalysis_amd import image as iimg, kernels, matcher
    from imageanalysis_amd._deps import getNode
    from imageanalysis_amd.hostlib import camera
    from test_sift_gpu import texture
    proj = tmp_path / 'p'
    (proj / 'images').mkdir(parents=True)
    an = proj / 'ImageAnalysis'
    (an / 'cache').mkdir(parents=True)
    (an / 'meta').mkdir()
    names = ['A', 'B', 'C', 'D']
    for k, name in enumerate(names):
        tex = texture(480, 640, 4 + k)
        PILImage.fromarray(np.ascontiguousarray(tex[:, :, ::-1])).save(str(proj / 'images' / (name + '.JPG')),
                                                                       quality=92, subsampling=1 + k % 2)
    getNode('/config/directories', True).setString('project_dir', str(proj))
    matcher.detector_node.setString('detector', 'SIFT')
    camera.set_image_params(640, 480)
    assert iimg.DEVICE_JPEG_ENTROPY is False
    out = []
    try:
        for dev_entropy in (True, False):
            iimg.DEVICE_JPEG_ENTROPY = dev_entropy
            before = dict(kernels.jpeg_device_stats)
            im = iimg.Image(str(an), 'A')
            im.detect_features(1.0, use_cache=False)
            iimg.cacheio.wait()
            assert kernels.jpeg_device_stats['device'] == before['device'] + (1 if dev_entropy else 0)
            out.append((im.kp_list.xy().copy(), np.asarray(im.des_list).copy()))
        assert len(out[0][0]) > 500
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
        # the prefetch workers' streams are where this runs in production
        res = {}
        for dev_entropy in (False, True):
            iimg.DEVICE_JPEG_ENTROPY = dev_entropy
            before = dict(kernels.jpeg_device_stats)
            ims = [iimg.Image(str(an), name) for name in names]
            pf = iimg.prefetch(ims, scale=1.0)
            try:
                for im in ims:
                    im.detect_features(1.0, use_cache=False)
            finally:
                pf.close()
            iimg.cacheio.wait()
            assert kernels.jpeg_device_stats['device'] == before['device'] + (4 if dev_entropy else 0)
            res[dev_entropy] = [(im.kp_list.xy().copy(), np.asarray(im.des_list).copy()) for im in ims]
        for a, b in zip(res[False], res[True]):
            assert len(a[0]) > 500 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        iimg.DEVICE_JPEG_ENTROPY = False


def test_two_streams_from_two_threads():
    import torch
    files = [sync_files()[4][1], sync_files()[N_SYNC_FILES - 5][1]]
    serial = [device_decode(d) for d in files]
    out = [None, None]
    err = []

    def work(k):
        try:
            with torch.cuda.device(torch.cuda.current_device()):
                out[k] = device_decode(files[k], stream=torch.cuda.Stream())
        except Exception as e:             # noqa: BLE001
            err.append(e)

    for _round in range(3):
        th = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not err, err
        for k in (0, 1):
            assert out[k][0] == SYNCED == serial[k][0]
            assert np.array_equal(out[k][2], serial[k][2])
