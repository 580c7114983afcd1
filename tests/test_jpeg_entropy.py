"""CPU: the device JPEG entropy decoder's decode routine (csrc/jpeg_entropy.h, shared by the
kernels of csrc/jpeg_entropy.hip) run by its host driver tools/jpeg_entropy_host.cpp, which this
file builds with the host compiler -- under AddressSanitizer + UBSan when the compiler links them
and the result starts (_driver['sanitized'] says which) -- against the host half
iamx_jpeg_decode_coefficients: every one of the blocks x 64 values equal, on files that
synchronise, on files that never do (then: equal or refused, and equal once the pass bound is the
number of sub-sequences), on damaged files (returns, guard row intact) and with stuffed FF 00 pairs
across sub-sequence boundaries.  Plus the argument checks of the new entry points, which need no
device.  The kernels themselves are compared in tests/test_jpeg_entropy_gpu.py."""
import ctypes
import io
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO
from test_jpeg import CASES, encode, host_decode

SYNCED, NOT_SYNCED, DAMAGED = 1, 2, 3

_driver = {}


def driver():
    """path of the host driver, built once per session; _driver['sanitized'] says how"""
    if 'path' in _driver:
        return _driver['path']
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    out = os.path.join(tempfile.mkdtemp(prefix='iamx_jeh_'), 'jpeg_entropy_host')
    src = os.path.join(REPO, 'tools', 'jpeg_entropy_host.cpp')
    base = [cxx, '-O1', '-g', '-std=c++17', '-Wall', '-o', out, src]
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    err = ''
    for flags in (san + ['-static-libasan'], san, []):
        r = subprocess.run(base + flags, capture_output=True, text=True)
        err = r.stderr
        # (a build counts when the program starts: without arguments it prints its usage, exit 2)
        if r.returncode == 0 and subprocess.run([out], capture_output=True, env=_env()).returncode == 2:
            _driver['sanitized'] = bool(flags)
            _driver['path'] = out
            break
    assert 'path' in _driver, err
    print('jpeg_entropy_host built %s sanitizers' % ('WITH' if _driver['sanitized'] else 'WITHOUT'))
    return out


def _env():
    return dict(os.environ, ASAN_OPTIONS='detect_leaks=0')


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def prepare(data):
    """iamx_jpeg_entropy_prepare -> (rc, info, quant, header bytes)"""
    from imageanalysis_amd import _lib
    L = _lib.lib()
    raw = np.frombuffer(bytes(data), np.uint8)
    info = np.zeros(16, np.int32)
    quant = np.zeros((3, 64), np.uint16)
    header = np.zeros(int(L.iamx_jpeg_entropy_header_bytes()), np.uint8)
    rc = L.iamx_jpeg_entropy_prepare(_p(raw), len(raw), _p(info), _p(quant), _p(header), len(header))
    return rc, info, quant, header


def run_driver(data, max_passes=None):
    """-> (status, passes, coef [blocks, 64], guard row, sub-sequences) of the host driver, or None
    when the host parser turns the file down"""
    rc, info, _quant, header = prepare(data)
    if rc != 0:
        return None
    d = tempfile.mkdtemp(prefix='iamx_je_')
    try:
        hp, fp, op = (os.path.join(d, n) for n in ('h.bin', 'f.jpg', 'o.bin'))
        header.tofile(hp)
        with open(fp, 'wb') as f:
            f.write(bytes(data))
        cmd = [driver(), hp, fp, op] + ([str(int(max_passes))] if max_passes else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=_env())
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        out = np.fromfile(op, np.uint8)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    head = out[:16].view(np.int32)
    blocks = int(head[2])
    assert blocks == int(info[11])
    coef = out[16:].view(np.int16).reshape(blocks + 1, 64)
    return int(head[0]), int(head[1]), coef[:blocks], coef[blocks], int(head[3])


def tex(h, w, seed):
    """the textured frame with a saturated flat band of the synchronisation study"""
    r = np.random.default_rng(seed)
    a = r.normal(0, 1, (h // 8 + 2, w // 8 + 2, 3))
    a = np.kron(a, np.ones((8, 8, 1)))[:h, :w] * 30
    a += r.normal(0, 12, (h, w, 3))
    a += 127
    yy, xx = np.mgrid[0:h, 0:w]
    a[:, :, 0] += 50 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
    a[h // 4:h // 3] = 255
    return np.clip(a, 0, 255).astype(np.uint8)


def enc(arr, q, sub=None, **kw):
    from PIL import Image
    buf = io.BytesIO()
    if sub is None:
        Image.fromarray(arr).save(buf, 'JPEG', quality=q, **kw)
    else:
        Image.fromarray(arr).save(buf, 'JPEG', quality=q, subsampling=sub, **kw)
    return buf.getvalue()


def study_files():
    """(name, bytes): the files of the study that must synchronise, and a 4:2:0 file with a restart
    interval of one MCU row"""
    return [('texture 4:2:0 q93', enc(tex(768, 1024, 1), 93, 2)),
            ('texture 4:2:2 q93 optimised', enc(tex(768, 1024, 2), 93, 1, optimize=True)),
            ('texture 4:4:4 q50', enc(tex(768, 1024, 3), 50, 0)),
            ('grey q90', enc(tex(600, 800, 4)[:, :, 0], 90)),
            ('texture 4:2:0 restart row', enc(tex(384, 512, 6), 90, 2, restart_marker_rows=1))]


N_SYNC_FILES = len(CASES) + 5
_cache = {}


def sync_files():
    """every file that must be decoded by the device path: none of them may be refused"""
    if 'sync' not in _cache:
        out = [('case %s %s q%s %s' % (shape, sub, q, extra), encode(shape, sub, q, extra, seed=q))
               for shape, sub, q, extra in CASES]
        _cache['sync'] = out + study_files()
        assert len(_cache['sync']) == N_SYNC_FILES
    return _cache['sync']


def flat_files():
    """files that (partly) never synchronise: a flat frame, and one whose upper half is flat"""
    if 'flat' not in _cache:
        half = tex(1024, 1024, 7)
        half[:512] = 200
        _cache['flat'] = [('flat 512x512 4:2:0', enc(np.full((512, 512, 3), 200, np.uint8), 90, 2)),
                          ('upper half flat 1024x1024 4:2:0', enc(half, 90, 2))]
    return _cache['flat']


@pytest.mark.parametrize('k', range(N_SYNC_FILES))
def test_host_driver_equals_host_half(k):
    name, data = sync_files()[k]
    rc, _info, want, _q = host_decode(data)
    assert rc == 0
    status, passes, coef, guard, nsub = run_driver(data)
    print(name, 'sub-sequences', nsub, 'passes', passes, 'status', status)
    assert status == SYNCED, (name, status, passes)
    assert (guard == 12345).all()
    assert coef.shape == want.shape and np.array_equal(coef, want), (name, int((coef != want).sum()))


@pytest.mark.parametrize('k', [0, 1])
def test_flat_files_are_exact_or_refused(k):
    name, data = flat_files()[k]
    rc, _info, want, _q = host_decode(data)
    assert rc == 0
    status, passes, coef, guard, nsub = run_driver(data)
    print(name, 'sub-sequences', nsub, 'passes', passes, 'status', status)
    assert (guard == 12345).all()
    assert status in (SYNCED, NOT_SYNCED)
    if status == SYNCED:
        assert np.array_equal(coef, want)
    else:
        assert not coef.any()              # nothing is written from an unverified state
    # with as many passes as sub-sequences the fixed point is reached whether or not anything
    # ever synchronises -- and it is the truth.  The driver's bound counts launches the way the
    # device does: pass 0 is the cold pass, which makes no lane true but lane 0's successor input,
    # pass j >= 1 makes lane j - 1 true, and the last pass only confirms that nothing changed.  So
    # n sub-sequences that never synchronise are verified by exactly n + 1 passes: "the number of
    # sub-sequences" true-making passes plus the cold one.
    status, passes, coef, guard, nsub = run_driver(data, max_passes=nsub + 1)
    print(name, 'bound', nsub + 1, 'passes', passes, 'status', status)
    assert status == SYNCED
    assert (guard == 12345).all() and np.array_equal(coef, want), int((coef != want).sum())


def test_host_driver_survives_damaged_files():
    """the recipe of test_jpeg.test_host_half_survives_damaged_files, own seed: the driver returns
    (the sanitizers watch every index), the guard row is intact, the status is a documented one"""
    from PIL import Image as PILImage
    rng = np.random.default_rng(2024)
    img = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    seen = set()
    for sub, rst in ((0, 0), (2, 0), (2, 4)):
        buf = io.BytesIO()
        PILImage.fromarray(img).save(buf, 'JPEG', quality=85, subsampling=sub, restart_marker_blocks=rst)
        good = np.frombuffer(buf.getvalue(), np.uint8)
        sos = int(np.nonzero((good[:-1] == 0xFF) & (good[1:] == 0xDA))[0][0]) + 14
        for trial in range(40):
            raw = good.copy()
            kind = trial % 4
            if kind == 0:
                idx = rng.integers(sos, len(raw) - 2, 12)
                raw[idx] = rng.integers(0, 256, 12, dtype=np.uint8)
            elif kind == 1:
                raw = raw[:int(rng.integers(sos, len(raw)))].copy()
            elif kind == 2:
                raw[sos + 5:] = 0xFF
            else:
                raw[int(rng.integers(sos, len(raw) - 2))] = 0xFF
            res = run_driver(raw.tobytes())
            if res is None:
                continue
            status, _passes, _coef, guard, _nsub = res
            seen.add(status)
            assert status in (SYNCED, NOT_SYNCED, DAMAGED)
            assert (guard == 12345).all()
    print('statuses met:', sorted(seen))


def test_truncated_file_stops_at_the_end_of_the_data():
    """cut at a third: what the data holds is decoded as the host half decodes it, nothing is made
    up behind it (the host half goes on with zero bits there), status: damaged"""
    data = encode((64, 64), 2, 90, {})
    cut = data[:len(data) // 3]
    rc, _info, want, _q = host_decode(cut)
    assert rc == 0
    status, _passes, coef, guard, _nsub = run_driver(cut)
    assert status == DAMAGED and (guard == 12345).all()
    assert np.array_equal(coef[0], want[0])                              # the frame's first block
    written = coef[:, 1:].any(axis=1)
    # AC of every block that has any; the block the data ends in is the only one that may differ
    # (the host half completes it from zero bits)
    assert int((coef[written][:, 1:] != want[written][:, 1:]).any(axis=1).sum()) <= 1
    assert 0 < int(written.sum()) < int(want[:, 1:].any(axis=1).sum())


def test_small_scan_under_a_large_claimed_frame():
    """the work of a lane is bounded by its sub-sequence, not by the frame size the file claims: a
    64 x 64 scan whose SOF says 4096 x 4096 (393 216 blocks) ends with "damaged" and with AC
    coefficients in at most the sixteen MCUs the data holds"""
    raw = np.frombuffer(encode((64, 64), 2, 90, {}), np.uint8).copy()
    sof = int(np.nonzero((raw[:-1] == 0xFF) & (raw[1:] == 0xC0))[0][0])
    raw[sof + 5:sof + 9] = [0x10, 0x00, 0x10, 0x00]                     # height, width = 4096
    rc, info, _quant, _header = prepare(raw.tobytes())
    assert rc == 0 and int(info[0]) == 4096 and int(info[1]) == 4096 and int(info[11]) == 256 * 256 * 6
    status, _passes, coef, guard, nsub = run_driver(raw.tobytes())
    assert status == DAMAGED and (guard == 12345).all()
    assert nsub <= 64
    assert 0 < int(coef[:, 1:].any(axis=1).sum()) <= 16 * 6


def test_bytes_behind_the_end_of_image_do_not_matter():
    """camera files carry previews and maker blobs behind EOI: the scan the lanes cover ends at
    the first marker that is not a restart marker, as it does for the host half"""
    rng = np.random.default_rng(77)
    for extra in ({}, dict(restart_marker_blocks=5)):
        data = encode((240, 321), 2, 90, extra)
        rc, _info, want, _q = host_decode(data)
        ref = run_driver(data)
        assert rc == 0 and ref[0] == SYNCED
        for tail in (rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), data, data * 4):
            both = data + tail
            rc2, _info2, want2, _q2 = host_decode(both)
            assert rc2 == 0 and np.array_equal(want2, want)
            status, passes, coef, guard, nsub = run_driver(both)
            assert status == SYNCED and (guard == 12345).all() and np.array_equal(coef, want)
            assert (passes, nsub) == (ref[1], ref[4])


def test_stray_marker_in_the_scan_is_damaged_not_refused():
    data = np.frombuffer(encode((240, 321), 2, 90, {}), np.uint8).copy()
    _rc, _info, _quant, header = prepare(data.tobytes())
    scan_off, scan_len = (int(v) for v in header[36:44].view(np.uint32))
    at = scan_off + scan_len // 2
    data[at:at + 3] = [0xFF, 0xFF, 0xD3]
    status, _passes, _coef, guard, _nsub = run_driver(data.tobytes())
    assert status == DAMAGED and (guard == 12345).all()


def test_file_that_ends_behind_sos_goes_the_host_way():
    data = encode((64, 64), 2, 90, {})
    _rc, _info, _quant, header = prepare(data)
    scan_off = int(header[36:40].view(np.uint32)[0])
    assert host_decode(data[:scan_off])[0] in (0, -1)
    if host_decode(data[:scan_off])[0] == 0:
        assert prepare(data[:scan_off])[0] == -4


def straddled_boundaries(data):
    """sub-sequence boundaries of the file's scan that fall between an FF and its stuffed 00"""
    raw = np.frombuffer(data, np.uint8)
    rc, _info, _quant, header = prepare(data)
    assert rc == 0
    scan_off, scan_len = (int(v) for v in header[36:44].view(np.uint32))   # ScanHeader.scan_off / scan_len
    subseq = int(header[52:56].view(np.int32)[0])                          # ScanHeader.subseq_bytes
    assert subseq >= 128 and subseq & (subseq - 1) == 0
    # (from the byte behind SOS to the EOI marker)
    assert scan_off + scan_len == len(raw) - 2 and raw[scan_off - 14] == 0xFF and raw[scan_off - 13] == 0xDA
    assert raw[-2] == 0xFF and raw[-1] == 0xD9
    scan = raw[scan_off:]
    bounds = np.arange(subseq, scan_len, subseq)          # counted from the scan's first byte
    return int(((scan[bounds - 1] == 0xFF) & (scan[bounds] == 0x00)).sum()), scan_len, subseq


def stuffed_file():
    rgb = np.random.default_rng(0).integers(0, 256, (256, 256, 3)).astype(np.uint8)
    return enc(rgb, 100, 2)


def test_stuffed_pairs_straddle_sub_sequence_boundaries():
    data = stuffed_file()
    straddled, scan_len, subseq = straddled_boundaries(data)
    print('scan bytes', scan_len, 'sub-sequence', subseq, 'boundaries between FF and 00:', straddled)
    assert straddled >= 1
    rc, _info, want, _q = host_decode(data)
    status, _passes, coef, guard, _nsub = run_driver(data)
    assert rc == 0 and status == SYNCED and (guard == 12345).all()
    assert np.array_equal(coef, want)


def test_argument_checks_do_not_need_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    data = encode((96, 128), 2, 95, {})
    raw = np.frombuffer(data, np.uint8)
    info = np.zeros(16, np.int32)
    quant = np.zeros((3, 64), np.uint16)
    nb = int(L.iamx_jpeg_entropy_header_bytes())
    header = np.zeros(nb, np.uint8)
    assert L.iamx_jpeg_entropy_prepare(None, len(raw), _p(info), _p(quant), _p(header), nb) == -1
    assert b'null pointer' in L.iamx_last_error()
    assert L.iamx_jpeg_entropy_prepare(_p(raw), len(raw), _p(info), _p(quant), _p(header), nb - 1) == -1
    assert L.iamx_jpeg_entropy_prepare(_p(raw), len(raw), _p(info), _p(quant), _p(header), nb) == 0
    ref = np.zeros(16, np.int32)
    assert L.iamx_jpeg_info(_p(raw), len(raw), _p(ref)) == 0 and np.array_equal(info, ref)
    assert np.array_equal(quant, host_decode(data)[3])
    ws = int(L.iamx_jpeg_entropy_workspace_bytes(_p(header)))
    assert ws > 0
    assert L.iamx_jpeg_entropy_workspace_bytes(None) == 0
    assert L.iamx_jpeg_entropy_workspace_bytes(_p(np.zeros(nb, np.uint8))) == 0
    blocks = int(info[11])
    fake = ctypes.c_void_p(4096)           # aligned, never dereferenced: the checks come first
    size = (len(raw) + 15) // 16 * 16
    args = lambda **kw: [kw.get('data', fake), kw.get('size', size), kw.get('header', _p(header)),
                         kw.get('d_header', fake), kw.get('ws', fake), kw.get('ws_bytes', ws),
                         kw.get('coef', fake), kw.get('blocks', blocks), kw.get('status', fake), None]
    for bad in (dict(data=None), dict(header=None), dict(d_header=None), dict(ws=None), dict(coef=None),
                dict(status=None), dict(size=len(raw) - 1), dict(ws_bytes=ws - 1), dict(blocks=blocks - 1),
                dict(data=ctypes.c_void_p(4097)), dict(header=_p(np.zeros(nb, np.uint8)))):
        assert L.iamx_jpeg_entropy_decode(*args(**bad)) == -1, bad


def test_unsupported_files_return_what_the_host_parser_returns():
    from PIL import Image
    from test_jpeg import scene
    buf = io.BytesIO()
    Image.fromarray(scene(64, 64, 1)).save(buf, 'JPEG', quality=90, progressive=True)
    assert prepare(buf.getvalue())[0] == -4 == host_decode(buf.getvalue())[0]
    buf = io.BytesIO()
    Image.fromarray(scene(64, 64, 1)).convert('CMYK').save(buf, 'JPEG', quality=90)
    assert prepare(buf.getvalue())[0] == -4
    assert prepare(b'\x89PNG\r\n\x1a\n' + b'0' * 64)[0] == -1
