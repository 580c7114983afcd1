"""GPU: the five image preparation kernels (csrc/image_prep.hip) stage by stage against
oracle/image_oracle.py, byte for byte.

Every comparison is np.array_equal; there is no tolerance in this file.  Both sides do the same
integer operations and the same separately rounded IEEE float32 operations (the file is compiled
with -ffp-contract=off), rintf and np.rint both round half to even: any differing byte is a bug on
one side.  The inputs are image_prep_cases.CASES; test_image_prep.py shows on the host that they
reach every branch and that the contracted float chains give other bytes on them."""
import ctypes

import numpy as np
import pytest

import image_prep_cases as cases
from oracle import image_oracle as io

pytestmark = pytest.mark.gpu

STAGES = ('hsv', 'hist', 'lut', 'equalised')


def _stages(h, w):
    from imageanalysis_amd import kernels
    return {k: t.cpu().numpy() for k, t in kernels.image_prep_stages(h, w).items()}


def _differing(got, want):
    """number of differing elements (the whole array where even the shape is wrong)"""
    got, want = np.asarray(got), np.asarray(want)
    return int((got != want).sum()) if got.shape == want.shape else max(got.size, want.size, 1)


@pytest.mark.parametrize('name', list(cases.CASES))
def test_every_stage_equals_the_oracle(name):
    """hsv, tile histograms (reflect-101 padded tiles), tile LUTs, equalised BGR, and the output at
    scales 1.0 and 0.4: the counts of differing elements are printed for all six before any is
    asserted, so that one run tells which stage departs first"""
    from imageanalysis_amd import kernels
    img, ref = cases.reference(name)
    h, w = img.shape[:2]
    out10 = kernels.equalize_resize(img, 1.0).cpu().numpy()
    st = _stages(h, w)
    bad = {k: _differing(st[k], ref[k]) for k in STAGES}
    bad['out 1.0'] = _differing(out10, io.resize_linear_u8(ref['equalised'], 1.0))
    out04 = kernels.equalize_resize(img, 0.4).cpu().numpy()
    bad['out 0.4'] = _differing(out04, io.resize_linear_u8(ref['equalised'], 0.4))
    print('STAGES', name, img.shape, bad)
    assert bad == dict.fromkeys(bad, 0)


@pytest.mark.parametrize('clip_limit', [1.0, 2.0, 3.0, 40.0, 0.01])
def test_clip_limits(clip_limit):
    """The kernel forms clip = (int)(clip_limit * area / 256) in float32 from a float argument, the
    oracle in double.  1, 2, 3 and 40 and their products with the tile area (130 here) are exact in
    float32, so both give the same integer.  At 40 the clip is 20 and no bin of this texture holds
    more than 15: nothing is clipped.  0.01 is not exact in float32, but either rounding gives
    0.005, which both raise to the minimum of 1.  Limits whose float32 rounding could move the
    integer are out of scope."""
    from imageanalysis_amd import kernels
    img, ref = cases.reference('texture_101x77')
    v, luts = io.clahe(ref['hsv'][..., 2], clip_limit, return_luts=True)
    want = io.hsv_to_bgr(np.concatenate([ref['hsv'][..., :2], v[..., None]], -1))
    out = kernels.equalize_resize(img, 1.0, clip_limit=clip_limit).cpu().numpy()
    st = _stages(101, 77)
    bad = {'lut': _differing(st['lut'], luts.reshape(64, 256)),
           'equalised': _differing(st['equalised'], want), 'out': _differing(out, want)}
    print('CLIP', clip_limit, bad)
    assert bad == dict.fromkeys(bad, 0)
    if clip_limit == 40.0:
        assert ref['hist'].max() <= 20                      # nothing clipped
    if clip_limit == 0.01:
        assert (np.minimum(ref['hist'], 1) != ref['hist']).any()      # clip 1 cuts


RESIZE_SCALES = (1.0, 0.999, 0.5, 0.4, 1 / 3, 0.25, 0.1, 1.5, 2.0, 3.7)


@pytest.mark.parametrize('shape', [(8, 8), (9, 13), (101, 77), (240, 320)])
def test_resize_alone(shape):
    from imageanalysis_amd import _lib, kernels
    img = cases.texture_image(*shape)
    bad = {}
    for scale in RESIZE_SCALES:
        got = kernels.equalize_resize(img, scale, equalize=False).cpu().numpy()
        want = io.resize_linear_u8(img, scale)
        assert got.shape == want.shape, (scale, got.shape, want.shape)
        bad[scale] = _differing(got, want)
        if scale == 1.0:
            assert np.array_equal(got, img)
        if shape == (8, 8) and scale == 0.1:
            assert got.shape == (1, 1, 3)
    print('RESIZE', shape, bad)
    assert bad == dict.fromkeys(bad, 0)
    if shape == (8, 8):
        with pytest.raises(_lib.IamxError):
            kernels.equalize_resize(img, 0.01, equalize=False)


def _raw(img, scale, ws_fill=0xFF):
    """the C ABI itself, with 256 guard bytes of 0xA5 behind the output and behind the workspace
    and the workspace proper filled with `ws_fill` -> (output, output tail, workspace tail)"""
    import torch
    from imageanalysis_amd import _lib, kernels
    L = _lib.lib()
    h, w = img.shape[:2]
    dh, dw = int(round(h * scale)), int(round(w * scale))
    need = int(L.iamx_image_prep_workspace_bytes(h, w))
    dev = _lib.require_gpu()
    src = torch.from_numpy(np.array(img, order='C')).to(dev)
    out = torch.full((dh * dw * 3 + 256,), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    ws[:need] = ws_fill
    _lib.check(L.iamx_image_equalize_resize(kernels._ptr(src), h, w, 1, 3.0, scale, kernels._ptr(ws),
                                            need, kernels._ptr(out), _lib.stream_ptr()),
               'iamx_image_equalize_resize')
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    return out[:dh * dw * 3].reshape(dh, dw, 3), out[dh * dw * 3:], ws[need:]


@pytest.mark.parametrize('name,scale', [('texture_101x77', 0.4), ('texture_17x23', 1.0),
                                        ('texture_523x601', 0.4)])
def test_raw_call_keeps_to_its_buffers_and_ignores_a_dirty_workspace(name, scale):
    """the workspace is all 0xFF before the call (histograms of -1 if the memset were missing)"""
    from imageanalysis_amd import kernels
    img, ref = cases.reference(name)
    got, out_tail, ws_tail = _raw(img, scale)
    assert np.all(out_tail == 0xA5) and len(out_tail) == 256
    assert np.all(ws_tail == 0xA5) and len(ws_tail) == 256
    assert np.array_equal(got, io.resize_linear_u8(ref['equalised'], scale))
    assert np.array_equal(got, kernels.equalize_resize(img, scale).cpu().numpy())


def test_a_smaller_image_after_a_larger_one_in_the_same_slot():
    from imageanalysis_amd import kernels
    big, _ = cases.reference('texture_96x128')
    small, ref = cases.reference('texture_17x23')
    kernels.equalize_resize(big, 1.0)
    out = kernels.equalize_resize(small, 1.0).cpu().numpy()
    st = _stages(17, 23)
    for k in STAGES:
        assert np.array_equal(st[k], ref[k]), k
    assert np.array_equal(out, ref['equalised'])


def test_refusals_come_before_any_launch():
    import torch
    from imageanalysis_amd import _lib, kernels
    L = _lib.lib()
    dev = _lib.require_gpu()
    need = int(L.iamx_image_prep_workspace_bytes(8, 8))
    src = torch.zeros((8, 8, 3), dtype=torch.uint8, device=dev)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((8 * 8 * 3,), 0xA5, dtype=torch.uint8, device=dev)
    p, st = kernels._ptr, _lib.stream_ptr()

    def call(src_p, h, w, ws_p, ws_bytes, out_p):
        return L.iamx_image_equalize_resize(src_p, h, w, 1, 3.0, 1.0, ws_p, ws_bytes, out_p, st)

    assert call(p(src), 7, 8, p(ws), need, p(out)) == -1 and b'bad size' in L.iamx_last_error()
    assert call(p(src), 8, 7, p(ws), need, p(out)) == -1 and b'bad size' in L.iamx_last_error()
    assert call(p(src), 8, 8, p(ws), need - 1, p(out)) == -1 and b'workspace too small' in L.iamx_last_error()
    assert call(None, 8, 8, p(ws), need, p(out)) == -1 and b'null pointer' in L.iamx_last_error()
    assert call(p(src), 8, 8, None, need, p(out)) == -1 and b'null pointer' in L.iamx_last_error()
    assert call(p(src), 8, 8, p(ws), need, None) == -1 and b'null pointer' in L.iamx_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()) and bool((out == 0xA5).all())       # nothing ran
    off, nbytes = ctypes.c_int64(-7), ctypes.c_int64(-7)
    for stage in (-1, 4, 1 << 20):
        assert L.iamx_image_prep_stage(8, 8, stage, ctypes.byref(off), ctypes.byref(nbytes)) == -1
        assert b'no such stage' in L.iamx_last_error()
    assert L.iamx_image_prep_stage(8, 8, 0, None, ctypes.byref(nbytes)) == -1
    assert L.iamx_image_prep_stage(8, 8, 0, ctypes.byref(off), None) == -1
    assert b'null pointer' in L.iamx_last_error()
    # and the layout it reports: the four stages in order, inside the workspace, hist 4-byte aligned
    end = 0
    for stage, want_bytes in enumerate((8 * 8 * 3, 8 * 8 * 3, 64 * 256 * 4, 64 * 256)):
        assert L.iamx_image_prep_stage(8, 8, stage, ctypes.byref(off), ctypes.byref(nbytes)) == 0
        assert nbytes.value == want_bytes and off.value >= end
        end = off.value + nbytes.value
        if stage == 2:
            assert off.value % 4 == 0
    assert end <= need
