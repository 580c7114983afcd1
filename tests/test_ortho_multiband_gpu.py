"""Mode multiband on the device (csrc/ortho_raster.hip through imageanalysis_amd/ortho.py) against
the numpy restatement of its rules (tests/ortho_multiband_restatement.py): bgr, index and count byte
for byte and every accumulator level bit for bit.  The reduce, accumulate and collapse kernels also
go through the C ABI on bare planes, with poison-filled outputs, guard elements behind every output
and NaN behind every input."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest

import ortho_common as oc
import ortho_multiband_common as mc
import ortho_multiband_restatement as mb
import step5_common as s5
from test_ortho_gpu import LIB_STANDIN, project  # noqa: F401  (the stand-in project, a module fixture)

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = -999.0


def _dev(frames):
    import torch
    return [torch.from_numpy(np.array(f)).cuda() for f in frames]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _compose(grids, uv, frames, width, height, gsd, bands=5, names=None):
    """the device's composer step by step -> (Mosaic, [(N, D)] as numpy, taken before the collapse)"""
    from imageanalysis_amd import ortho
    comp = ortho._Composer(grids, uv, width, height, gsd, 'multiband', names, bands)
    for k, f in enumerate(frames):
        comp.add(k, f)
    acc = [(n.cpu().numpy(), d.cpu().numpy()) for n, d in comp.accumulators()]
    m = comp.finish()
    with pytest.raises(RuntimeError):
        comp.accumulators()
    return m, acc


def _equal(m, acc, ref, what):
    bgr, index, count = m.bgr.cpu().numpy(), m.index.cpu().numpy(), m.count.cpu().numpy()
    assert m.mode == 'multiband' and m.bands == ref['bands'] == len(acc), what
    assert bgr.shape == ref['bgr'].shape and index.dtype == np.int32 and count.dtype == np.uint16, what
    bad = [int((_n != ref['N'][l]).sum() + (_d != ref['D'][l][:, :, 0]).sum()) for l, (_n, _d) in enumerate(acc)]
    print('%s: %d x %d, %d levels, covered %d, bgr bytes differing %d, accumulator floats differing per level %s'
          % (what, bgr.shape[1], bgr.shape[0], m.bands, int((ref['count'] > 0).sum()), int((bgr != ref['bgr']).sum()), bad))
    assert _bits(index) == _bits(ref['index']) and _bits(count) == _bits(ref['count']), what
    for l, (n, d) in enumerate(acc):
        assert n.dtype == np.float32 and n.shape == ref['N'][l].shape, (what, l)
        assert _bits(n) == _bits(ref['N'][l]) and _bits(d) == _bits(ref['D'][l][:, :, 0]), (what, l)
    assert _bits(bgr) == _bits(ref['bgr']), what
    assert (m.x0, m.y1, m.gsd) == (ref['frame']['x0'], ref['frame']['y1'], ref['frame']['gsd'])


def _both(key, grids, uv, frames, gsd=1.0, bands=5):
    ref = mc.restated(key, grids, uv, frames, gsd, 'multiband', bands)
    m, acc = _compose(grids, uv, _dev(frames), mc.WIDTH, mc.HEIGHT, gsd, bands)
    _equal(m, acc, ref, '%s bands=%d' % (key, bands))
    return m, ref


# ---- the recorded Step 5 grids ----
@pytest.mark.parametrize('scene', ['step5_mid_default', 'step5_mid_tilted'])
def test_recorded_grids_equal_the_restatement(scene):
    """30 images at 3 m, up to 20 over one pixel; mid_tilted: NaN vertices and the all-sky image.  Also:
    index and count are mode best's, and a second run gives the same bytes"""
    from imageanalysis_amd import ortho
    names, grids, uv, width, height = oc.scene_input(scene)
    ref = mc.golden(scene, 'multiband')
    frames = _dev([oc.hash_frame(k) for k in range(len(grids))])
    m, acc = _compose(grids, uv, frames, width, height, mc.GOLDEN_GSD, names=names)
    _equal(m, acc, ref, scene)
    assert m.names == names and m.bands == 5 and ref['count'].max() >= 15
    best = ortho.compose(grids, uv, frames, width, height, mc.GOLDEN_GSD, 'best')
    assert _bits(best.index.cpu().numpy()) == _bits(m.index.cpu().numpy())
    assert _bits(best.count.cpu().numpy()) == _bits(m.count.cpu().numpy())
    assert (best.bgr.cpu().numpy() != m.bgr.cpu().numpy()).any()
    again = ortho.compose(grids, uv, frames, width, height, mc.GOLDEN_GSD, 'multiband', names=names)
    for a, b in ((again.bgr, m.bgr), (again.index, m.index), (again.count, m.count)):
        assert _bits(a.cpu().numpy()) == _bits(b.cpu().numpy())
    assert again.bands == 5 and again.mode == 'multiband'


# ---- the kernels on bare planes, through the C ABI ----
SIZES = [(1, 1), (1, 7), (2, 2), (3, 5), (15, 15), (16, 16), (17, 17), (17, 33)]


def _corner_regions(h, w):
    """a region in each corner of the level, and the level: inclusive (y0, x0, y1, x1)"""
    rh, rw = (h + 1) // 2, (w + 1) // 2
    out = [(0, 0, rh - 1, rw - 1), (0, w - rw, rh - 1, w - 1), (h - rh, 0, h - 1, rw - 1), (h - rh, w - rw, h - 1, w - 1),
           (0, 0, h - 1, w - 1)]
    return sorted(set(out))


def _cut(plane, r):
    return np.ascontiguousarray(plane[r[0]:r[2] + 1, r[1]:r[3] + 1])


def _only(plane, r):
    """the plane, 0 outside the region"""
    out = np.zeros_like(plane)
    out[r[0]:r[2] + 1, r[1]:r[3] + 1] = plane[r[0]:r[2] + 1, r[1]:r[3] + 1]
    return out


class _Planes(object):
    """device buffers of float4 pixels: inputs with NaN behind them, outputs poison-filled with guards"""

    def __init__(self):
        import torch
        from imageanalysis_amd import _lib
        self.torch, self.L = torch, _lib.lib()
        self.dev = torch.device('cuda', 0)
        self.outputs = []

    def inp(self, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        return self.torch.from_numpy(np.concatenate([a, np.full(4 * GUARD, np.nan, np.float32)])).to(self.dev)

    def out(self, name, a=None, floats=0, dtype=np.float32):
        """poison-filled (a None) or holding `a`, with guards behind"""
        poison = 0xAB if dtype == np.uint8 else POISON
        body = np.full(floats, poison, dtype) if a is None else np.ascontiguousarray(a, dtype).reshape(-1)
        t = self.torch.from_numpy(np.concatenate([body, np.full(4 * GUARD, poison, dtype)])).to(self.dev)
        self.outputs.append((name, t, len(body)))
        return t

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def check(self, rc):
        assert rc == 0, self.L.iamx_last_error()

    def read(self, t):
        """after the call: the guards are whole -> the buffer's body"""
        self.torch.cuda.synchronize()
        for name, o, used in self.outputs:
            tail = o[used:].cpu().numpy()
            assert (tail == (0xAB if tail.dtype == np.uint8 else POISON)).all(), 'guard behind %s written' % name
        used = [u for _n, o, u in self.outputs if o is t][0]
        return t[:used].cpu().numpy()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize('size', SIZES)
def test_reduce_kernel_on_bare_planes(size):
    """the source given over a region (0 outside it), the destination over the region it can reach
    and over the whole coarser level"""
    from imageanalysis_amd import ortho
    h, w = size
    rng = np.random.default_rng(h * 100 + w)
    plane = rng.normal(0.0, 100.0, (h, w, 4)).astype(np.float32)
    sizes = [(h, w), ((h + 1) // 2, (w + 1) // 2)]
    for sr in _corner_regions(h, w):
        want = mb.reduce(_only(plane, sr))
        reach = ortho.level_regions((sr[1], sr[0], sr[3], sr[2]), sizes)[1]
        assert (want != 0).any(axis=2).sum() <= (reach[2] - reach[0] + 1) * (reach[3] - reach[1] + 1)
        assert _bits(_only(want, reach)) == _bits(want)                  # nothing non-zero outside the derived extent
        for dr in sorted({reach, (0, 0, sizes[1][0] - 1, sizes[1][1] - 1)}):
            P = _Planes()
            src = P.inp(_cut(plane, sr))
            dst = P.out('dst', floats=4 * (dr[2] - dr[0] + 1) * (dr[3] - dr[1] + 1))
            P.check(P.L.iamx_ortho_mb_reduce(h, w, _p(src), *sr, _p(dst), *dr, P.stream()))
            got = P.read(dst)
            assert _bits(got) == _bits(_cut(want, dr)), (size, sr, dr)


@pytest.mark.parametrize('size', SIZES)
def test_accumulate_kernel_on_bare_planes(size):
    """N += A (C - E(C')), D += A over a region of a level holding earlier sums; the coarser layer over
    the region the finer one reaches; and the top level's form without a coarser layer"""
    from imageanalysis_amd import ortho
    h, w = size
    ch, cw = (h + 1) // 2, (w + 1) // 2
    rng = np.random.default_rng(h * 1000 + w)
    fine = rng.normal(0.0, 100.0, (h, w, 4)).astype(np.float32)
    fine[:, :, 3] = rng.random((h, w)).astype(np.float32) * (rng.random((h, w)) < 0.7)      # A: some exact zeros
    coarse = rng.normal(0.0, 100.0, (ch, cw, 4)).astype(np.float32)
    before = rng.normal(0.0, 50.0, (h, w, 4)).astype(np.float32)
    for fr in _corner_regions(h, w):
        cr = ortho.level_regions((fr[1], fr[0], fr[3], fr[2]), [(h, w), (ch, cw)])[1]
        f = _only(fine, fr)
        for top in (False, True):
            lp = f[:, :, :3] if top else f[:, :, :3] - mb.expand(_only(coarse, cr)[:, :, :3], h, w)
            want = before.copy()
            want[:, :, :3] = before[:, :, :3] + f[:, :, 3:] * lp
            want[:, :, 3] = before[:, :, 3] + f[:, :, 3]
            want = np.where(_only(np.ones_like(before), fr) > 0, want, before)     # outside the region: untouched
            P = _Planes()
            acc = P.out('acc', before)
            d_fine, d_coarse = P.inp(_cut(fine, fr)), (None if top else P.inp(_cut(coarse, cr)))
            P.check(P.L.iamx_ortho_mb_accumulate(h, w, _p(d_fine), *fr, _p(d_coarse), *(cr if not top else (0, 0, 0, 0)),
                                                 _p(acc), P.stream()))
            assert _bits(P.read(acc)) == _bits(want), (size, fr, top)


@pytest.mark.parametrize('size', SIZES)
def test_collapse_kernel_on_bare_planes(size):
    """M = N / D (0 where D is 0) + E(M'), in place; the level-0 form that ends in bgr"""
    h, w = size
    ch, cw = (h + 1) // 2, (w + 1) // 2
    rng = np.random.default_rng(h * 10 + w)
    acc = rng.normal(60.0, 120.0, (h, w, 4)).astype(np.float32)
    acc[:, :, 3] = (rng.random((h, w)) * (rng.random((h, w)) < 0.8)).astype(np.float32)
    acc[:, :, :3] *= acc[:, :, 3:]
    up = rng.normal(0.0, 40.0, (ch, cw, 4)).astype(np.float32)
    count = (rng.random((h, w)) < 0.8).astype(np.uint16) * 3
    q = mb.quotient(acc[:, :, :3], acc[:, :, 3:])
    for with_up in (True, False):
        m = q + mb.expand(up[:, :, :3], h, w) if with_up else q
        want = np.concatenate([m, acc[:, :, 3:]], axis=2)
        P = _Planes()
        a, u = P.out('acc', acc), (P.inp(up) if with_up else None)
        P.check(P.L.iamx_ortho_mb_collapse(h, w, _p(a), _p(u), None, None, P.stream()))
        assert _bits(P.read(a)) == _bits(want), (size, with_up)
        bgr = np.floor(np.minimum(np.maximum(m, np.float32(0)), np.float32(255)) + np.float32(0.5)).astype(np.uint8)
        bgr[count == 0] = 0
        P = _Planes()
        a, u = P.out('acc', acc), (P.inp(up) if with_up else None)
        c = P.torch.from_numpy(count).to(P.dev)
        out = P.out('bgr', floats=3 * h * w, dtype=np.uint8)
        P.check(P.L.iamx_ortho_mb_collapse(h, w, _p(a), _p(u), _p(c), _p(out), P.stream()))
        assert _bits(P.read(out)) == _bits(bgr) and _bits(P.read(a)) == _bits(acc), (size, with_up)


# ---- bands and mosaic sizes ----
@pytest.mark.parametrize('size', [(1, 1), (15, 17), (16, 16), (17, 33), (33, 15)])
def test_bands_and_mosaic_sizes_around_the_block(size):
    """an image over the whole mosaic and one over its south-east part; bands 1, 2, the capped
    maximum and 16"""
    W, H = size
    cap = 1 + (max(W, H) - 1).bit_length()
    grids = [mc.grid(mc.lattice(2, 0.0, 0.0, float(W), float(H)), float(H)),
             mc.grid(mc.lattice(2, 0.4 * W, 0.3 * H, float(W), float(H)), float(H))]
    frames = [oc.hash_frame(8), oc.hash_frame(9)]
    for bands in sorted({1, 2, cap, 16}):
        m, ref = _both('size %d x %d' % size, grids, mc.uv(2), frames, bands=bands)
        assert ref['bgr'].shape == (H, W, 3) and m.bands == min(bands, cap) and (ref['count'] >= 1).all()
        assert W == 1 or ref['count'].max() == 2


# ---- degenerate groups ----
def test_an_image_without_a_used_cell_one_that_never_wins_and_twins():
    from imageanalysis_amd import ortho
    big = mc.grid(mc.lattice(2, 0.0, 0.0, 60.0, 40.0), 40.0)
    other = mc.grid(mc.lattice(2, 30.0, 0.0, 90.0, 40.0), 40.0)
    inner = mc.grid(mc.lattice(2, 20.0, 10.0, 70.0, 30.0), 40.0)
    inner[:, 2] = np.linspace(0.0, 4000.0, len(inner))                  # a tall span: its metric loses everywhere
    sky = np.full_like(big, np.nan)
    frames = [oc.hash_frame(k) for k in (1, 2, 3, 4)]
    m, ref = _both('sky and loser', [big, sky, other, inner], mc.uv(2), frames)
    assert not np.isin(ref['index'], (1, 3)).any() and ref['count'].max() == 3
    without, _acc = _compose([big, other], mc.uv(2), _dev(frames[:1] + frames[2:3]), mc.WIDTH, mc.HEIGHT, 1.0)
    assert _bits(without.bgr.cpu().numpy()) == _bits(m.bgr.cpu().numpy())
    assert (without.count.cpu().numpy() != m.count.cpu().numpy()).sum() >= 900
    twin = mc.grid(mc.lattice(2, 0.25, 0.25, 20.75, 18.75), 19.0)
    m, ref = _both('twins', [twin, twin.copy()], mc.uv(2), [oc.hash_frame(1), oc.hash_frame(2)])
    covered = ref['count'] > 0
    assert covered.sum() > 300 and (ref['count'][covered] == 2).all() and (ref['index'][covered] == 0).all()
    alone = ortho.compose([twin], mc.uv(2), _dev([oc.hash_frame(1)]), mc.WIDTH, mc.HEIGHT, 1.0, 'multiband')
    assert _bits(alone.bgr.cpu().numpy()) == _bits(m.bgr.cpu().numpy())          # the later twin adds nothing


# ---- what the mode is for ----
def test_seam_and_detail_on_the_device():
    from imageanalysis_amd import ortho

    def device(frames, mode):
        return ortho.compose(mc.PAIR, mc.uv(1), _dev(frames), mc.WIDTH, mc.HEIGHT, 1.0, mode).bgr.cpu().numpy()
    m, _ref = _both('seam', mc.PAIR, mc.uv(1), mc.SEAM_FRAMES)
    mc.check_seam(device(mc.SEAM_FRAMES, 'best'), m.bgr.cpu().numpy())
    m, _ref = _both('detail', mc.PAIR, mc.uv(1), mc.DETAIL_FRAMES)
    mc.check_detail(device(mc.DETAIL_FRAMES, 'best'), m.bgr.cpu().numpy(), device(mc.DETAIL_FRAMES, 'feather'))


# ---- refusals ----
def test_refusals_on_the_device_path():
    from imageanalysis_amd import ortho
    g = mc.grid(mc.lattice(1, 0.0, 0.0, 8.0, 8.0), 8.0)
    frames = _dev([oc.hash_frame(1)])
    with pytest.raises(MemoryError, match=r'800000 x 800000 pixel mosaic \(mode multiband\) needs [0-9.]+ GB of accumulators'):
        ortho.compose([g], mc.uv(1), frames, mc.WIDTH, mc.HEIGHT, 1.0 / 100000, 'multiband')
    with pytest.raises(ValueError, match='bands'):
        ortho.compose([g], mc.uv(1), frames, mc.WIDTH, mc.HEIGHT, 1.0, 'multiband', bands=17)
    with pytest.raises(ValueError, match='frames'):
        ortho.compose([g, g], mc.uv(1), frames, mc.WIDTH, mc.HEIGHT, 1.0, 'multiband')
    with pytest.raises(ValueError, match='device uint8'):
        ortho.compose([g], mc.uv(1), [oc.hash_frame(1)], mc.WIDTH, mc.HEIGHT, 1.0, 'multiband')
    comp = ortho._Composer([g], mc.uv(1), mc.WIDTH, mc.HEIGHT, 1.0, 'best')
    with pytest.raises(RuntimeError, match='multiband'):
        comp.accumulators()


# ---- render() and the command line ----
GSD = 3.0


def test_render_equals_compose_on_the_prepared_frames(project, tmp_path):  # noqa: F811
    from imageanalysis_amd import ortho
    proj, g = project
    names = list(g['groups'][0])
    frames = _dev([oc.hash_frame(k) for k in range(len(names))])
    with contextlib.redirect_stdout(io.StringIO()):
        m = ortho.render(proj, g['groups'], 0, GSD, mode='multiband', frames=frames, bands=3)
    assert (m.mode, m.bands, m.names) == ('multiband', 3, names) and ortho.render_stats['images'] == 30
    grids = np.array([proj.findImageByName(n).grid_list for n in names], np.float64)
    uv = np.array(proj.findImageByName(names[0]).distorted_uv, np.float64)
    cells, _v = ortho.used_cells(grids)
    ready = [ortho.prepare_frame(f, n, grids[k], cells[k], GSD)[0] for k, (f, n) in enumerate(zip(frames, names))]
    want = ortho.compose(grids, uv, ready, g['width'], g['height'], GSD, 'multiband', bands=3)
    for a, b in ((m.bgr, want.bgr), (m.index, want.index), (m.count, want.count)):
        assert _bits(a.cpu().numpy()) == _bits(b.cpu().numpy())
    ref = mb.compose(grids, uv, [f.cpu().numpy() for f in ready], g['width'], g['height'], GSD, 3)
    assert _bits(m.bgr.cpu().numpy()) == _bits(ref['bgr']) and int(ref['count'].max()) >= 15
    info = ortho.save(m, str(tmp_path), tile=64, fmt='png')
    assert (info['mode'], info['bands']) == ('multiband', 3) and len(info['tiles']) == 2 * 2


def test_script_writes_tiles_and_ortho_json(project, tmp_path):  # noqa: F811
    """5c-ortho.py --mode multiband --bands 3 in a process of its own; its tiles are the mosaic
    render() makes in this process from the same decoded frames"""
    import subprocess
    import sys
    from PIL import Image
    from imageanalysis_amd import image, ortho, panda3d
    proj, g = project
    names = list(g['groups'][0])
    lib = tmp_path / 'standin' / 'lib'
    lib.mkdir(parents=True)
    for name, text in LIB_STANDIN.items():
        (lib / name).write_text(text)
    pdir = tmp_path / 'project'
    (pdir / 'images').mkdir(parents=True)
    (pdir / 'ImageAnalysis').mkdir()
    (pdir / 'ImageAnalysis' / 'matches_grouped').write_bytes(g['matches_in'])
    decoded = []
    for k, n in enumerate(names):
        path = str(pdir / 'images' / (n + '.JPG'))
        with open(path, 'wb') as fp:
            fp.write(panda3d.encode_jpeg(np.array(oc.hash_frame(k))))
        decoded.append(image._decode_bgr(path))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path / 'standin'), s5.REPO,
                                                       os.path.join(s5.REPO, 'tests')]))
    script = os.path.join(s5.REPO, 'imageanalysis_amd', 'scripts', '5c-ortho.py')
    cmd = ['timeout', '-k', '10', '120', sys.executable, script, str(pdir), '--gsd', str(GSD), '--mode', 'multiband',
           '--bands', '3', '--tile', '64', '--format', 'png']
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    assert '30 images' in p.stdout and 'Wrote 4 tiles' in p.stdout
    out = pdir / 'ImageAnalysis' / 'ortho'
    info = json.loads((out / 'ortho.json').read_text())
    assert (info['mode'], info['bands'], info['gsd'], info['images']) == ('multiband', 3, GSD, names)
    with contextlib.redirect_stdout(io.StringIO()):
        want = ortho.render(proj, g['groups'], 0, GSD, mode='multiband', frames=_dev(decoded), bands=3).bgr.cpu().numpy()
    assert (want.sum(axis=2) > 0).mean() > 0.5 and want.shape[:2] == (info['height'], info['width'])
    for t in info['tiles']:
        with Image.open(str(out / t['file'])) as im:
            px = np.asarray(im.convert('RGB'))[:, :, ::-1]
        r0, c0 = t['row'] * 64, t['col'] * 64
        assert _bits(px) == _bits(want[r0:r0 + t['height'], c0:c0 + t['width']]), t['file']
        assert (out / t['world_file']).is_file()
