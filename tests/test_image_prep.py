"""CPU: the inputs of the image preparation tests are fair and oracle/image_oracle.py is pinned
where a closed form exists.  What the device computes is in test_image_prep_gpu.py; here the
colour cube is shown to be complete, the redistribution image to hold the residuals it promises,
and three inputs to tell the oracle's separately rounded float chains from the contracted ones
(image_prep_cases.clahe_fused / hsv_to_bgr_fused), which is what makes the device's byte equality
with the oracle a statement about -ffp-contract=off."""
import numpy as np
import pytest

import image_prep_cases as cases
from oracle import image_oracle as io


def _flat_lut(area, value, clip_limit=3.0):
    """closed form of the LUT of a tile that holds `area` pixels of one value"""
    clip = max(int(clip_limit * area / 256), 1)
    batch, residual = divmod(area - clip, 256)
    i = np.arange(256)
    hist = np.full(256, batch, np.int64)
    if residual:
        step = max(256 // residual, 1)
        hist += (i % step == 0) & (i // step < residual)
    hist[value] += clip
    assert hist.sum() == area
    return np.rint(np.cumsum(hist).astype(np.float32) * (np.float32(255.0) / np.float32(area)))


@pytest.mark.parametrize('shape,area', [((8, 8), 1), ((80, 104), 130), ((256, 256), 1024),
                                        ((523, 601), 5016)])
@pytest.mark.parametrize('value', [0, 137, 255])
def test_clahe_of_a_flat_image_is_the_closed_form(shape, area, value):
    """every tile (padding included) has the same one-bin histogram, so every LUT is the closed
    form and the blend of four equal LUT values is that value"""
    ph, pw, th, tw = cases.tile_geometry(*shape)
    assert th * tw == area
    v = cases.flat_image(value, *shape)[..., 0]
    res, luts = io.clahe(v, return_luts=True)
    want = _flat_lut(area, value)
    assert np.array_equal(luts.reshape(64, 256), np.broadcast_to(want, (64, 256)))
    assert np.array_equal(res, np.full(shape, want[value]))
    if area == 1:
        assert want[value] == 255 and np.all(want[:value] == 0)


@pytest.mark.parametrize('tile', [(32, 32), (30, 34)])
def test_residual_image_has_the_promised_excesses(tile):
    th, tw = tile
    area = th * tw
    clip = max(int(3.0 * area / 256.0), 1)
    img = cases.residual_image(th, tw)
    assert img.shape == (8 * th, 8 * tw, 3)
    assert np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
    hist = cases.tile_histograms(img[..., 0])
    ex = cases.residual_excesses(th, tw)
    assert np.array_equal(cases.clipped_totals(hist, clip), ex)
    assert len(set(ex.tolist())) == 64
    # one dominant value per tile, at a place of its own; nothing else reaches the clip
    dom = hist.argmax(axis=1)
    assert len(set(dom.tolist())) == 64
    assert np.array_equal(hist[np.arange(64), dom], clip + ex)
    rest = hist.copy()
    rest[np.arange(64), dom] = 0
    assert rest.max() <= clip
    top = area - clip
    promised = set(cases.PROMISED_EXCESSES[:-1]) | {top}
    if tile == (32, 32):
        assert clip == 12 and promised == set(cases.PROMISED_EXCESSES)
    assert promised <= set(ex.tolist())
    batch, residual = ex // 256, ex % 256
    assert set(batch.tolist()) == {0, 1, 2, 3}
    assert {0, 1, 2, 85, 86, 127, 128, 129, 255} <= set(residual.tolist())
    step = np.maximum(256 // np.maximum(residual, 1), 1)[residual > 0]
    assert {1, 2, 3, 128, 256} <= set(step.tolist())


def test_colour_slabs_hold_the_cube_and_reach_every_branch():
    seen = np.zeros(1 << 24, np.uint8)
    v_is = {'r': False, 'g': False, 'b': False}
    grey = wrap = s0 = False
    sectors = set()
    for k in range(16):
        slab = cases.colour_slab(k)
        assert slab.shape == (256, 4096, 3) and slab.dtype == np.uint8
        assert np.all(slab[..., 0] >> 4 == k)
        b, g, r = (slab[..., c].astype(np.int64).ravel() for c in range(3))
        packed = (b << 16) | (g << 8) | r
        assert np.all(np.diff(packed) == 1)                 # lexicographic (b, g, r)
        np.add.at(seen, packed, 1)
        v = np.maximum(np.maximum(b, g), r)
        diff = v - np.minimum(np.minimum(b, g), r)
        v_is['r'] |= bool(np.any((v == r) & (diff > 0)))
        v_is['g'] |= bool(np.any((v != r) & (v == g)))
        v_is['b'] |= bool(np.any((v != r) & (v != g)))
        grey |= bool(np.any(diff == 0))
        # the hue before the wrap is negative exactly where v == r and g < b
        wrap |= bool(np.any((v == r) & (g < b)))
        hsv = io.bgr_to_hsv(slab[::7, ::5])
        assert hsv[..., 0].max() < 180
        s0 |= bool(np.any(hsv[..., 1] == 0))
        sectors |= set(np.unique(np.floor(hsv[..., 0][hsv[..., 1] > 0].astype(np.float32)
                                          * np.float32(6.0 / 180.0)).astype(int)).tolist())
    assert seen.min() == 1 and seen.max() == 1              # every 24-bit colour exactly once
    assert all(v_is.values()) and grey and wrap and s0
    assert sectors == {0, 1, 2, 3, 4, 5}


def test_tie_colours_and_grey_ramp_are_what_they_say():
    t = cases.tie_colours()
    assert t.shape[0] >= 64 and t.shape[1] >= 64
    cols, counts = np.unique(t.reshape(-1, 3), axis=0, return_counts=True)
    assert len(cols) == 216 and counts.min() == counts.max() == 24
    g = cases.grey_ramp(64, 71)
    hsv = io.bgr_to_hsv(g)
    assert np.all(hsv[..., 1] == 0) and np.all(hsv[..., 0] == 0)
    assert len(np.unique(hsv[..., 2])) == 256
    for axis in (0, 1):
        two = cases.two_level_image(64, 71, axis)
        assert set(np.unique(two).tolist()) == {0, 255}
        assert np.all(two[0, 0] == 0) and np.all(two[-1, -1] == 255)


# input -> (V bytes, BGR bytes) that differed between the oracle and the contracted restatement
# when this was written (DESIGN.md records them; the assertions below only need them non-zero)
FUSED_COUNTS = {'texture_523x601': (87, 265), 'slab07': (0, 83), 'slab07_cropped': (44, 143),
                'residual': (0, 0), 'residual_30x34': (19, 57)}


@pytest.mark.parametrize('name', sorted(FUSED_COUNTS))
def test_inputs_tell_contraction_from_the_oracle(name):
    """The device's equality with the oracle says something about contraction only on inputs where
    the contracted chains give other bytes.  colour_slab(7) and residual_image() have 32-pixel
    tiles: 1/32 and every blend weight are dyadic, every product and sum of the blend is exact,
    and contraction cannot show in V (in residual_image(), grey, not at all).  Their siblings
    (the slab cropped to 250x4000, the residual image with 30x34 tiles) stand in for them here
    and run on the device next to them."""
    img, ref = cases.reference(name)
    v = ref['hsv'][..., 2]
    dv = cases.clahe_fused(v) != io.clahe(v)
    dbgr = cases.equalize_bgr_fused(img) != ref['equalised']
    got = (int(dv.sum()), int(dbgr.sum()))
    print(name, 'V bytes', got[0], 'of', dv.size, 'BGR bytes', got[1], 'of', dbgr.size)
    if name == 'residual':
        assert got == (0, 0)
    elif name == 'slab07':
        assert got[0] == 0 and got[1] >= 1
    else:
        assert got[0] >= 1 and got[1] >= 1
    diff = np.abs(cases.equalize_bgr_fused(img).astype(int) - ref['equalised'].astype(int))
    assert diff.max() <= 1


def test_resize_identity_and_hand_cases():
    img = cases.texture_image(17, 23)
    assert np.array_equal(io.resize_linear_u8(img, 1.0), img)
    # 2x2 -> 4x4: f = (d + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25 -> taps (0, t = 0), (0, 0.25),
    # (0, 0.75), (1, 0): weights 2048 a = 2048, 1536, 512, 0 on the first sample
    src = np.array([[0, 200], [100, 40]], np.uint8)
    a = np.array([2048, 1536, 512, 0])
    rows0 = src[0, 0] * a + src[0, 1] * (2048 - a)
    rows1 = src[1, 0] * a + src[1, 1] * (2048 - a)
    want = ((a[:, None] * (rows0 >> 4)[None, :] >> 16) + ((2048 - a)[:, None] * (rows1 >> 4)[None, :] >> 16) + 2) >> 2
    assert np.array_equal(want, [[0, 50, 150, 200], [25, 59, 126, 160], [75, 76, 79, 80], [100, 85, 55, 40]])
    assert np.array_equal(io.resize_linear_u8(src, 2.0), want)
    # 4x4 -> 2x2: f = (d + 0.5) * 2 - 0.5 = 0.5, 2.5: the mean of a 2x2 block, rounded half up
    src = np.array([[0, 10, 20, 31], [2, 12, 22, 33], [255, 255, 0, 0], [255, 254, 0, 1]], np.uint8)
    assert np.array_equal(io.resize_linear_u8(src, 0.5), [[6, 27], [255, 0]])
