"""Shared inputs and restatements for the image preparation tests (csrc/image_prep.hip against
oracle/image_oracle.py): test_image_prep.py proves on the host that these inputs are fair,
test_image_prep_gpu.py runs them on the device.  No test functions here.

clahe_fused / hsv_to_bgr_fused are NOT an oracle.  They restate the oracle's two float chains with
the seven contractions the compiler made in clahe_apply_kernel while the file was built without
-ffp-contract=off (read off its assembly):
    tyf  = fma(y, 1/th, -0.5)                 txf = fma(x, 1/tw, -0.5)
    top  = fma(xa, l12, rn(xa1 * l11))        bot = fma(xa, l22, rn(xa1 * l21))
    res  = fma(ya1, top, rn(ya * bot))
    f    = fma(H, 6/180, -sector)             (sector from the separately rounded product)
    tab3 = v * fma(-s, 1 - f, 1)
They exist so that the host tests can show that an input tells the two forms apart, which is what
makes the device's equality with the oracle a statement about contraction."""
import functools

import numpy as np

from oracle import image_oracle as io
from test_sift_gpu import texture

TILES = 8

# the excesses residual_image() promises: residual 0, step 256 / 128 / 3 / 2 / 1, batches 0..3 and
# the largest excess a 32x32 tile can have at clip 12
PROMISED_EXCESSES = (0, 1, 2, 85, 86, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 1012)
TEXTURE_SHAPES = ((8, 8), (8, 9), (9, 8), (15, 17), (16, 16), (17, 23), (64, 71), (101, 77),
                  (96, 128), (8, 4099), (4099, 8), (523, 601))


def colour_slab(k):
    """256x4096x3: the 2^20 colours with b >> 4 == k in lexicographic (b, g, r) order; the sixteen
    slabs hold every 24-bit colour exactly once"""
    n = np.arange(1 << 20, dtype=np.int64) + (int(k) << 20)
    return np.stack([n >> 16, (n >> 8) & 255, n & 255], -1).astype(np.uint8).reshape(256, 4096, 3)


def residual_excesses(th=32, tw=32):
    """the 64 distinct excesses E_t of residual_image(th, tw), tile by tile: the promised ones (the
    last replaced by area - clip where the tile is not 32x32) and 48 more, 20 apart"""
    area = th * tw
    top = area - max(int(3.0 * area / 256.0), 1)
    promised = [e for e in PROMISED_EXCESSES[:-1]] + [top]
    rest = [e for e in range(3, top, 20) if e not in promised][:64 - len(promised)]
    ex = np.array(promised + rest, np.int64)
    assert len(ex) == 64 and len(set(ex.tolist())) == 64 and ex.max() == top
    return ex[(np.arange(64) * 27) % 64]                      # (27 is odd: a permutation of the tiles)


def residual_image(th=32, tw=32):
    """(8 th)x(8 tw) grey as BGR; the default has 32x32 tiles (area 1024, clip 12).  Tile t holds one
    dominant value (37 t + 11) % 256 with count clip + E_t; the other area - clip - E_t pixels are
    spread evenly over the other 255 values (at most 4 of each), so the clipped total of tile t is
    exactly E_t.  32x32 tiles make every float of the blend exact (1/32 and the weights are dyadic),
    so residual_image(30, 34) is its sibling on which contraction shows."""
    rng = np.random.default_rng(20)
    ex = residual_excesses(th, tw)
    area = th * tw
    clip = max(int(3.0 * area / 256.0), 1)
    v = np.zeros((TILES * th, TILES * tw), np.uint8)
    for t in range(64):
        dom = (37 * t + 11) % 256
        rest = area - clip - int(ex[t])
        others = (dom + 1 + np.arange(255)) % 256
        counts = rest // 255 + (np.arange(255) < rest % 255)
        px = np.concatenate([np.full(clip + int(ex[t]), dom), np.repeat(others, counts)])
        j, i = divmod(t, TILES)
        v[j * th:(j + 1) * th, i * tw:(i + 1) * tw] = rng.permutation(px).reshape(th, tw)
    return np.repeat(v[..., None], 3, axis=2)


def colour_slab_cropped(k):
    """colour_slab(k)[:250, :4000]: 32x500 tiles, whose 1/500 is not dyadic, so that contraction
    shows in V too (the whole slab's 32x512 tiles make the blend exact)"""
    return np.ascontiguousarray(colour_slab(k)[:250, :4000])


def flat_image(value, h, w):
    return np.full((h, w, 3), value, np.uint8)


def two_level_image(h, w, axis):
    """axis 1: left half 0, right half 255; axis 0: top half 0, bottom half 255"""
    img = np.zeros((h, w, 3), np.uint8)
    if axis == 1:
        img[:, w // 2:] = 255
    else:
        img[h // 2:] = 255
    return img


def grey_ramp(h, w):
    """b = g = r: S = 0 everywhere, every V value present"""
    v = (2 * np.arange(h)[:, None] + 3 * np.arange(w)[None, :]) % 256
    return np.repeat(v.astype(np.uint8)[..., None], 3, axis=2)


def tie_colours():
    """72x72: every (b, g, r) over {0, 1, 127, 128, 254, 255}, 24 times each: all the ties of the
    max channel, all orders of the channels, diff == 0"""
    lv = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    cols = np.stack(np.meshgrid(lv, lv, lv, indexing='ij'), -1).reshape(-1, 3)
    return cols[(np.arange(72 * 72) * 7) % 216].reshape(72, 72, 3)       # (7 and 216 are coprime)


def texture_image(h, w):
    """the colour texture of test_image_gpu.test_equalize_resize_equals_oracle at any shape"""
    rng = np.random.default_rng(h)
    img = texture(h, w, 1)
    img[..., 1] = np.roll(img[..., 1], 7, axis=1)          # colourful: exercise the hue path
    img[::5, ::7] = rng.integers(0, 256, img[::5, ::7].shape, dtype=np.uint8)
    return img


CASES = {}
for _k in range(16):
    CASES['slab%02d' % _k] = functools.partial(colour_slab, _k)
CASES['slab07_cropped'] = functools.partial(colour_slab_cropped, 7)
CASES['residual'] = residual_image
CASES['residual_30x34'] = functools.partial(residual_image, 30, 34)
CASES['flat0_8x8'] = functools.partial(flat_image, 0, 8, 8)
CASES['flat137_80x104'] = functools.partial(flat_image, 137, 80, 104)
CASES['flat255_523x601'] = functools.partial(flat_image, 255, 523, 601)
CASES['two_level_lr'] = functools.partial(two_level_image, 64, 71, 1)
CASES['two_level_tb'] = functools.partial(two_level_image, 67, 64, 0)
CASES['grey_ramp'] = functools.partial(grey_ramp, 64, 71)
CASES['tie_colours'] = tie_colours
for _h, _w in TEXTURE_SHAPES:
    CASES['texture_%dx%d' % (_h, _w)] = functools.partial(texture_image, _h, _w)


def tile_geometry(h, w):
    """(padded height, padded width, tile height, tile width) of the 8x8 CLAHE grid"""
    ph = h if h % TILES == 0 else h + (TILES - h % TILES)
    pw = w if w % TILES == 0 else w + (TILES - w % TILES)
    return ph, pw, ph // TILES, pw // TILES


def tile_histograms(v):
    """int64 [64, 256]: np.bincount over each reflect-101 padded tile of v, row = ty * 8 + tx"""
    h, w = v.shape
    ph, pw, th, tw = tile_geometry(h, w)
    src = v[io._reflect101(np.arange(ph), h)][:, io._reflect101(np.arange(pw), w)]
    tiles = src.reshape(TILES, th, TILES, tw).transpose(0, 2, 1, 3).reshape(64, th * tw)
    return np.stack([np.bincount(t, minlength=256) for t in tiles]).astype(np.int64)


def clipped_totals(hist, clip):
    """loop-free: what the clip at `clip` cuts off each histogram row"""
    return np.maximum(hist - clip, 0).sum(axis=1)


def _fma(a, b, c):
    """a * b + c as a float64 product plus a float64 add, rounded once to float32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def clahe_fused(v, clip_limit=3.0):
    """io.clahe's blend of the oracle's own LUTs with the five contractions of the tile
    coordinates and the three blends (module docstring)"""
    h, w = v.shape
    _ph, _pw, th, tw = tile_geometry(h, w)
    luts = io.clahe(v, clip_limit, return_luts=True)[1]
    f1 = np.float32(1)

    def coords(n, tile):
        f = _fma(np.arange(n, dtype=np.float32), np.float32(1.0 / tile), np.float32(-0.5))
        t1 = np.floor(f).astype(np.int64)
        a = f - t1.astype(np.float32)
        return np.maximum(t1, 0), np.minimum(t1 + 1, TILES - 1), a.astype(np.float32)

    y1, y2, ya = coords(h, th)
    x1, x2, xa = coords(w, tw)
    ya, xa = ya[:, None], xa[None, :]
    vv = v.astype(np.int64)
    l11 = luts[y1[:, None], x1[None, :], vv].astype(np.float32)
    l12 = luts[y1[:, None], x2[None, :], vv].astype(np.float32)
    l21 = luts[y2[:, None], x1[None, :], vv].astype(np.float32)
    l22 = luts[y2[:, None], x2[None, :], vv].astype(np.float32)
    xa1, ya1 = f1 - xa, f1 - ya
    top = _fma(xa, l12, xa1 * l11)
    bot = _fma(xa, l22, xa1 * l21)
    res = _fma(ya1, top, ya * bot)
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def hsv_to_bgr_fused(hsv):
    """io.hsv_to_bgr with f = fma(H, 6/180, -sector) and tab3 = v * fma(-s, 1 - f, 1)"""
    f1 = np.float32(1)
    c6 = np.float32(6.0 / 180.0)
    hb = hsv[..., 0].astype(np.float32)
    s = hsv[..., 1].astype(np.float32) * np.float32(1.0 / 255.0)
    v = hsv[..., 2].astype(np.float32) * np.float32(1.0 / 255.0)
    sector = np.floor(hb * c6).astype(np.int64)
    f = _fma(hb, c6, -sector.astype(np.float32))
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    f = np.where(bad, np.float32(0), f)
    tab = np.stack([v, v * (f1 - s), v * (f1 - s * f), v * _fma(-s, f1 - f, f1)], -1)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    out = np.take_along_axis(tab, sd[sector], axis=-1)
    out = np.where((hsv[..., 1] == 0)[..., None], v[..., None], out)
    return np.clip(np.rint(out * np.float32(255.0)), 0, 255).astype(np.uint8)


def equalize_bgr_fused(bgr):
    hsv = io.bgr_to_hsv(bgr)
    hsv[..., 2] = clahe_fused(hsv[..., 2])
    return hsv_to_bgr_fused(hsv)


@functools.lru_cache(maxsize=4)
def reference(name):
    """(input, oracle stages) of CASES[name], computed once and shared; treat as read-only:
    'hsv' io.bgr_to_hsv, 'hist' tile_histograms of V, 'lut' [64, 256] and 'equalised' of io.clahe /
    io.equalize_bgr"""
    img = CASES[name]()
    hsv = io.bgr_to_hsv(img)
    v, luts = io.clahe(hsv[..., 2], return_luts=True)
    eq = io.hsv_to_bgr(np.concatenate([hsv[..., :2], v[..., None]], -1))
    ref = {'hsv': hsv, 'hist': tile_histograms(hsv[..., 2]), 'lut': luts.reshape(64, 256), 'equalised': eq}
    for a in (img, *ref.values()):
        a.setflags(write=False)
    return img, ref
