"""Thin python bindings over the C ABI: torch tensors are device-buffer containers only,
every number is produced by a hand-written HIP kernel in libiamx.so (csrc/*.hip)."""
import math
import os
import threading

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, require_gpu, stream_ptr

I8, I32, I64, F64, U8 = torch.int8, torch.int32, torch.int64, torch.float64, torch.uint8
I16 = torch.int16                        # the bits of a uint16 total of the semi-global mode (at most 4072)


def _ptr(t):
    return _lib.c_void_p(t.data_ptr()) if t is not None else _lib.c_void_p(0)


def _dev(x, dtype):
    """numpy / tensor -> contiguous device tensor of `dtype` (a copy, not a compute step)."""
    dev = require_gpu()
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype).contiguous()
    x = np.ascontiguousarray(x)
    if not x.flags.writeable:
        import warnings
        with warnings.catch_warnings():       # a read-only source (bytes of a decoder) is only read
            warnings.simplefilter('ignore', UserWarning)
            return torch.from_numpy(x).to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(x).to(device=dev, dtype=dtype).contiguous()


# --------------------------------------------------------------------------------------
# descriptor store
# --------------------------------------------------------------------------------------
# Upload staging of DescriptorStore.set_images: two page-locked host buffers (a group of images is
# gathered into one while the copy out of the other runs), one device buffer the pack kernels read
# (re-used in stream order) and their scratch.  One set per device, kept for the process.
STAGE_BYTES = 64 << 20
STAGE_TAIL = 64 << 10            # int64 offsets of up to 8191 images per group
_stages = {}
_stage_lock = threading.Lock()


def _upload_stage(dev, nbytes):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _stages.get(key)
    if st is None or st['bytes'] < nbytes:
        rows = (nbytes + 127) // 128
        # (+ STAGE_TAIL bytes behind the rows: the group's row offsets travel with the same copy -- a
        #  pageable `tensor.to(device)` of their own would make the host wait for the device per group)
        st = _stages[key] = dict(bytes=rows * 128,
                                 pin=[torch.empty(rows * 128 + STAGE_TAIL, dtype=U8).pin_memory() for _ in range(2)],
                                 dev=torch.empty(rows * 128 + STAGE_TAIL, dtype=U8, device=dev),
                                 scratch=torch.empty(3 * rows, dtype=I32, device=dev),
                                 ev=[torch.cuda.Event(), torch.cuda.Event()], used=[False, False], next=0)
    return st


def prewarm_upload_stage():
    """Allocate the upload staging of the current device on a helper thread (page-locking its two
    64 MB host buffers takes 0.1-0.2 s: matcher.configure() starts it, find_matches finds it done)."""
    if not torch.cuda.is_available():
        return None
    idx = torch.cuda.current_device()

    def _go():
        try:
            with torch.cuda.device(idx), _stage_lock:
                _upload_stage(torch.device('cuda', idx), STAGE_BYTES)
        except Exception:                     # noqa: BLE001  (best effort: set_images allocates what is missing)
            pass
    th = threading.Thread(target=_go, name='iamx-stage', daemon=True)
    th.start()
    return th


class DescriptorStore(object):
    """All images' SIFT descriptors packed back to back in HBM (include/iamx.h, 'Descriptor
    store'): int8 rows (value-128), each image zero-padded to 128 rows, + two int32 norms
    per row.  288 GB of HBM hold > 10^9 descriptors, so a whole survey stays resident."""

    # The arena's three layouts, in one place: (suffix of the layout's offsets / img_off attributes,
    # rows an image of n rows takes, per-row buffers that hold image data, per-row scratch) with
    # (attribute, elements per row, dtype) per buffer.  Offsets, allocation, the growth copy and the
    # bytes per row all come from here; a scratch buffer holds nothing of an image, so growth
    # does not copy it.
    LAYOUTS = (
        # original order: the general kernel, the exact stage of the symmetric form
        ('', 'iamx_desc_padded_rows', (('desc', 128, I8), ('norm_q', 1, I32), ('norm_t', 1, I32)),
         (('key_t', 1, I32),)),                              # key_t: scratch of iamx_knn2sym_exact
        # parity partitioned (include/iamx.h "desc2"): the one-direction fast sweep, train_layout only
        ('2', 'iamx_desc2_rows_cap', (('desc2', 128, I8), ('norm2', 1, I32), ('cinit', 1, I32),
                                      ('perm', 1, I32)), ()),
        # rows ordered by |a-128|^2 (include/iamx.h "desc3"): the symmetric sweep
        ('3', 'iamx_desc3_rows_cap', (('desc3', 128, I8), ('sn2', 1, I32), ('sct', 1, I32),
                                      ('sperm', 1, I32), ('sinv', 1, I32)), ()),
    )
    # bytes per reserved row a caller may budget with: row_bytes(False) = 284 plus slack
    RESERVE_ROW_BYTES = 290

    @classmethod
    def row_bytes(cls, train_layout):
        """device bytes per (padded) descriptor row, all layouts together"""
        return sum(w * torch.iinfo(dt).bits // 8 for sfx, _cap, data, scratch in cls.LAYOUTS
                   if train_layout or sfx != '2' for _name, w, dt in data + scratch)

    @classmethod
    def _layout_offsets(cls, counts):
        """cumulative row offsets (int64 [len(counts) + 1]) of images of `counts` rows, per layout"""
        L = lib()
        offs = []
        for _sfx, cap, _data, _scratch in cls.LAYOUTS:
            o = np.zeros(len(counts) + 1, np.int64)
            np.cumsum([int(getattr(L, cap)(c)) for c in counts], out=o[1:])
            offs.append(o)
        return offs

    def _has(self, sfx):
        return sfx != '2' or self.has_train_layout

    def _set_tables(self, counts, offs):
        """the small per-image tables of `counts` (host offsets, device img_off* / img_n)"""
        dev = self.desc.device
        self.counts = counts
        for (sfx, _cap, _data, _scratch), o in zip(self.LAYOUTS, offs):
            setattr(self, 'offsets' + sfx, o)
            setattr(self, 'img_off' + sfx, torch.from_numpy(o[:-1].astype(np.int32)).to(dev))
        self.caps3 = np.diff(offs[2])
        self.img_n = torch.tensor(counts, dtype=I32, device=dev) if counts else \
            torch.zeros(0, dtype=I32, device=dev)

    def __init__(self, counts, train_layout=True, reserve_rows=0, reserve_images=0):
        """train_layout=False: the parity-partitioned copy `desc2` (a third of the arena) is not
        kept.  Only the ONE-direction fast sweep reads it; a store that serves batches holding
        both directions of every pair (find_matches: the symmetric sweep reads `desc3`, the exact
        stage `desc`) does without, and a batch the symmetric sweep refuses (an image of < 2 rows)
        then takes the general kernel, which reads `desc` only.  The choice holds for the store's
        life, and for every store grown from it (copy_images_from).
        reserve_rows / reserve_images: capacity beyond `counts` -- try_extend() appends images
        without re-allocating (find_matches meeting undetected images registers ~250 per round:
        rebuilding a 40 GB arena each time was a quarter of that call form's time)."""
        dev = require_gpu()
        self.has_train_layout = bool(train_layout)
        counts = [int(c) for c in counts]
        reserve_rows, reserve_images = int(reserve_rows), int(reserve_images)
        offs = self._layout_offsets(counts)
        if max(int(o[-1]) for o in offs) >= 2 ** 31:
            raise ValueError("descriptor store limited to 2^31 rows")
        for (sfx, _cap, data, scratch), o in zip(self.LAYOUTS, offs):
            total = max(int(o[-1]), reserve_rows, 1) if self._has(sfx) else 1
            if total >= 2 ** 31:
                total = max(int(o[-1]), 1)
            for name, w, dt in data + scratch:
                setattr(self, name, torch.empty((total, w) if w > 1 else total, dtype=dt, device=dev))
        # per image: the parity classes of its desc2 rows (written with them, zero without)
        self.meta = torch.zeros((max(len(counts), reserve_images, 1), 4), dtype=I32, device=dev)
        self._set_tables(counts, offs)

    def __len__(self):
        return len(self.counts)

    @property
    def rows_used(self):
        """rows of the original-order layout that belong to images (the buffers may be larger)"""
        return int(self.offsets[-1])

    def try_extend(self, new_counts):
        """Append images of new_counts rows each behind the existing ones if every layout's
        buffers (and `meta`, whichever layouts the store keeps) have room: the big buffers stay,
        the small per-image tables are rebuilt (batches made earlier keep their own references; the
        rows of old images do not move).  -> False (and nothing changed) when the capacity does
        not suffice."""
        counts = self.counts + [int(c) for c in new_counts]
        offs = self._layout_offsets(counts)
        if len(counts) > self.meta.shape[0] or max(int(o[-1]) for o in offs) >= 2 ** 31:
            return False
        for (sfx, _cap, data, _scratch), o in zip(self.LAYOUTS, offs):
            if self._has(sfx) and o[-1] > getattr(self, data[0][0]).shape[0]:
                return False
        self._set_tables(counts, offs)
        return True

    def copy_images_from(self, old):
        """Growth: this freshly built store's first len(old) images are `old`'s -- their rows in
        every layout's data buffers (and their `meta` rows with the parity-partitioned layout) are
        copied on the device, enqueued on the current stream.  Offsets depend on the counts alone,
        so the rows land where set_image() would have put them."""
        k = len(old.counts)
        if self.counts[:k] != old.counts:
            raise ValueError("copy_images_from: the older store's images must come first")
        if self.has_train_layout and not old.has_train_layout:
            raise ValueError("copy_images_from: the older store has no parity-partitioned layout")
        for sfx, _cap, data, _scratch in self.LAYOUTS:
            if self._has(sfx):
                n = int(getattr(old, 'offsets' + sfx)[-1])
                for name, _w, _dt in data:
                    getattr(self, name)[:n].copy_(getattr(old, name)[:n])
        if self.has_train_layout:
            self.meta[:k].copy_(old.meta[:k])

    def set_image(self, i, des, sync=True):
        """Pack descriptors of image i.  `des`: [n,128] float32 (cv2/reference layout, integer
        valued) or uint8, numpy or device tensor.  With sync=False the kernels are only
        enqueued and the temporaries they read are returned: keep them alive until the stream
        has been synchronised."""
        n = self.counts[i]
        if n == 0:
            return ()
        if isinstance(des, np.ndarray) and des.dtype != np.uint8 and des.dtype != np.float32:
            des = des.astype(np.float32)
        is_u8 = (des.dtype == np.uint8) if isinstance(des, np.ndarray) else (des.dtype == U8)
        src = _dev(des, U8 if is_u8 else torch.float32)
        if tuple(src.shape) != (n, 128):
            raise ValueError("image %d: expected descriptors of shape (%d,128), got %s"
                             % (i, n, tuple(src.shape)))
        o = int(self.offsets[i])
        fn = lib().iamx_desc_pack_u8 if is_u8 else lib().iamx_desc_pack_f32
        check(fn(_ptr(src), n, _ptr(self.desc[o:]), _ptr(self.norm_q[o:]), _ptr(self.norm_t[o:]),
                 stream_ptr()), 'iamx_desc_pack')
        scratch = None
        if self.has_train_layout:
            o2 = int(self.offsets2[i])
            fn2 = lib().iamx_desc2_pack_u8 if is_u8 else lib().iamx_desc2_pack_f32
            scratch = torch.empty(3 * n, dtype=I32, device=src.device)
            check(fn2(_ptr(src), n, _ptr(self.desc2[o2:]), _ptr(self.norm2[o2:]), _ptr(self.cinit[o2:]),
                      _ptr(self.perm[o2:]), _ptr(self.meta[i]), _ptr(scratch), stream_ptr()),
                  'iamx_desc2_pack')
        o3 = int(self.offsets3[i])
        fn3 = lib().iamx_desc3_pack_u8 if is_u8 else lib().iamx_desc3_pack_f32
        scratch3 = torch.empty(3 * n, dtype=I32, device=src.device)
        check(fn3(_ptr(src), n, _ptr(self.desc3[o3:]), _ptr(self.sn2[o3:]), _ptr(self.sct[o3:]),
                  _ptr(self.sperm[o3:]), _ptr(self.sinv[o3:]), _ptr(scratch3), stream_ptr()),
              'iamx_desc3_pack')
        # the source buffer must outlive the enqueued kernels
        if sync:
            torch.cuda.current_stream().synchronize()
            return ()
        return (src, scratch, scratch3)

    def set_images(self, first, arrays):
        """Pack the descriptors of the consecutive images first .. first + len(arrays) - 1: host
        arrays ([n,128] float32 or uint8) go up in GROUPS of <= STAGE_BYTES -- gathered (float32:
        converted) into one of two page-locked staging buffers by libiamx's threads, copied to the
        device asynchronously and packed by the batched kernels while the threads fill the other
        buffer.  (Until round 6 the whole list was concatenated into ONE pageable host block first:
        2.4 GB copied by a numpy loop and uploaded synchronously for 512 frames of 37 k keypoints --
        0.37 s of a 2.3 s match stage -- and 47 GB of host AND device temporaries at 10 000 frames.)
        Enqueues on the current stream and returns the temporaries the kernels read (keep them
        until the stream is synchronised)."""
        import ctypes
        k = len(arrays)
        if k == 0:
            return ()
        counts = [self.counts[first + i] for i in range(k)]
        for i, a in enumerate(arrays):
            if not isinstance(a, np.ndarray) or a.dtype not in (np.float32, np.uint8) \
                    or tuple(a.shape) != (counts[i], 128):
                raise ValueError("set_images: image %d is not a host [n,128] float32 / uint8 array" % (first + i))
        arrays = [np.ascontiguousarray(a) for a in arrays]
        if int(sum(counts)) == 0:
            return ()
        dev = self.desc.device
        L, sp = lib(), stream_ptr()
        threads = min(16, os.cpu_count() or 1)
        keep = []
        with _stage_lock:
            self._set_images_staged(first, arrays, counts, keep, L, sp, threads, dev)
        return tuple(keep)

    def _set_images_staged(self, first, arrays, counts, keep, L, sp, threads, dev):
        import ctypes
        k = len(arrays)
        stage = _upload_stage(dev, max(STAGE_BYTES, 128 * int(max(counts))))
        keep.append(stage)
        g0 = 0
        while g0 < k:
            g1, rows = g0, 0
            while g1 < k and g1 - g0 < STAGE_TAIL // 8 - 1 and \
                    (g1 == g0 or (rows + counts[g1]) * 128 <= stage['bytes']):
                rows += counts[g1]
                g1 += 1
            n = g1 - g0
            if rows == 0:
                g0 = g1
                continue
            slot = stage['next'] = (stage['next'] + 1) % 2
            pin, ev = stage['pin'][slot], stage['ev'][slot]
            if stage['used'][slot]:
                ev.synchronize()                     # the copy that read this buffer last has run
            off = np.zeros(n + 1, np.int64)
            np.cumsum(counts[g0:g1], out=off[1:])
            grp = arrays[g0:g1]
            dst = ctypes.c_void_p(pin.data_ptr())
            srcs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in grp])
            if all(a.dtype == np.float32 for a in grp):
                cnt = (ctypes.c_int64 * n)(*[a.size for a in grp])
                check(L.iamx_f32_to_u8_many(srcs, cnt, n, dst, threads), 'iamx_f32_to_u8_many')
            elif all(a.dtype == np.uint8 for a in grp):
                cnt = (ctypes.c_int64 * n)(*[a.size for a in grp])
                check(L.iamx_u8_gather_many(srcs, cnt, n, dst, threads), 'iamx_u8_gather_many')
            else:
                host = pin.numpy()[:rows * 128].reshape(rows, 128)
                for i, a in enumerate(grp):
                    host[off[i]:off[i + 1]] = a if a.dtype == np.uint8 else \
                        np.clip(np.rint(a), 0, 255).astype(np.uint8)
            tail = stage['bytes']
            pin[tail:tail + 8 * (n + 1)].view(torch.int64).copy_(torch.from_numpy(off))
            # (two copies: the rows of the group, and the offsets behind the buffer's row area)
            stage['dev'][:rows * 128].copy_(pin[:rows * 128], non_blocking=True)
            stage['dev'][tail:tail + 8 * (n + 1)].copy_(pin[tail:tail + 8 * (n + 1)], non_blocking=True)
            src = stage['dev'][:rows * 128].view(rows, 128)
            ev.record()
            stage['used'][slot] = True
            # original-order store: image by image (one launch each: images are padded to 128 rows)
            for i in range(n):
                if counts[g0 + i]:
                    o = int(self.offsets[first + g0 + i])
                    check(L.iamx_desc_pack_u8(_ptr(src[int(off[i]):]), counts[g0 + i], _ptr(self.desc[o:]),
                                              _ptr(self.norm_q[o:]), _ptr(self.norm_t[o:]), sp), 'iamx_desc_pack_u8')
            src_off = stage['dev'][tail:tail + 8 * (n + 1)].view(torch.int64)
            mx = int(max(counts[g0:g1]))
            scratch = stage['scratch'][:3 * rows]
            if self.has_train_layout:
                check(L.iamx_desc2_pack_batch_u8(_ptr(src), _ptr(src_off), _ptr(self.img_off2[first + g0:]), n, rows, mx,
                                                 _ptr(self.desc2), _ptr(self.norm2), _ptr(self.cinit),
                                                 _ptr(self.perm), _ptr(self.meta[first + g0]), _ptr(scratch), sp),
                      'iamx_desc2_pack_batch_u8')
            check(L.iamx_desc3_pack_batch_u8(_ptr(src), _ptr(src_off), _ptr(self.img_off3[first + g0:]), n, rows, mx,
                                             _ptr(self.desc3), _ptr(self.sn2), _ptr(self.sct), _ptr(self.sperm),
                                             _ptr(self.sinv), _ptr(scratch), sp), 'iamx_desc3_pack_batch_u8')
            g0 = g1

    @classmethod
    def from_arrays(cls, arrays):
        st = cls([a.shape[0] for a in arrays])
        for i, a in enumerate(arrays):
            st.set_image(i, a)
        return st


def wg_per_pair(nq):
    return (int(nq) + 255) // 256


SYM_ROWS_PER_WG = {0: 256, 1: 512, 2: 1024}       # iamx_knn2sym_rows_per_wg(form)


def sym_tables(pairs, counts, caps3):
    """Host-side launch tables of the symmetric sweep (include/iamx.h, iamx_knn2sym_sweep) for a
    batch of ORDERED pairs [P,2], or None when the batch does not hold both directions of every
    image pair exactly once.  Unordered pair u = (B image, A image): B = the query image of the
    first of its two ordered pairs; the list is sorted by A so that consecutive workgroups
    re-read the same streamed rows from L2.  osrc[p] = (u, role) with role 0 when the query image
    of ordered pair p is B (its bounds come from the lane-local column direction), 1 when it is A.

    Where the form-2 item walk takes more than one pair per workgroup (sym_item_pairs > 1: short
    images), B is instead the TRAIN image of the first ordered pair and the list is sorted by
    (B, A): in a train-major schedule consecutive pairs then share B, which the walk keeps in
    registers (sym_items).  S (1 for forms 0 and 1) is returned with the tables, so that the order
    and the item table follow one rule.  The bounds are valid whichever side is B."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    P = len(pairs)
    if P == 0 or P % 2 or (pairs[:, 0] == pairs[:, 1]).any():
        return None
    counts = np.asarray(counts, np.int64)
    caps3 = np.asarray(caps3, np.int64)
    n_img = len(counts)
    key = pairs[:, 0].astype(np.int64) * n_img + pairs[:, 1]
    mkey = pairs[:, 1].astype(np.int64) * n_img + pairs[:, 0]
    order = np.argsort(key, kind='stable')
    skey = key[order]
    if (skey[1:] == skey[:-1]).any():
        return None                                   # an ordered pair listed twice
    where = np.minimum(np.searchsorted(skey, mkey), P - 1)
    if (skey[where] != mkey).any():
        return None                                   # a pair without its mirror
    mirror = order[where]
    first = np.nonzero(np.arange(P) < mirror)[0]      # one ordered pair per unordered pair
    mn = int(counts[pairs[first]].min())
    if mn < 2:
        return None
    form = 0 if mn < 2048 else (2 if mn >= 4096 else 1)
    S = sym_item_pairs(counts[pairs[first].ravel()]) if form == 2 else 1
    items = S > 1
    if items:                                         # B = train image, sorted by (B, A)
        first = first[np.lexsort((pairs[first, 0], pairs[first, 1]))]
        up = np.ascontiguousarray(pairs[first, ::-1])
    else:                                             # B = query image, sorted by A
        first = first[np.argsort(pairs[first, 1], kind='stable')]
        up = pairs[first]
    n_u = len(up)
    nb = counts[up[:, 0]]
    rows_wg = SYM_ROWS_PER_WG[form]
    nwg = (nb + rows_wg - 1) // rows_wg
    wg = np.zeros(n_u + 1, np.int64)
    np.cumsum(nwg, out=wg[1:])
    if wg[-1] >= 2 ** 31:
        return None
    col_off = np.zeros(n_u + 1, np.int64)
    np.cumsum(caps3[up[:, 0]], out=col_off[1:])
    rowp_off = np.zeros(n_u + 1, np.int64)
    np.cumsum(nwg * caps3[up[:, 1]], out=rowp_off[1:])
    osrc = np.zeros((P, 2), np.int32)
    osrc[first, 0] = np.arange(n_u)
    osrc[mirror[first], 0] = np.arange(n_u)
    osrc[first if items else mirror[first], 1] = 1
    return dict(upairs=up, form=form, wg=wg, col_off=col_off, rowp_off=rowp_off, osrc=osrc, S=S)


def sym_item_pairs(counts_a):
    """S, the unordered pairs a form-2 workgroup walks (iamx_knn2sym_sweep_items), from the rows of
    the batch's images (either side of a pair may become A).  A workgroup pays its start-up (wave launch, table reads, B slice load)
    once per item: S > 1 only where that start-up is a sizeable share of a pair's work -- at
    4096-row A images (32 chunks) S = 4 saves about 5 % of the sweep (profiles/r8_sweep_startup.txt),
    at 16 384 rows and more (128+ chunks) S = 1.  Rule: S = 16384 // (largest A cap), within 1..4."""
    cap = (int(np.max(counts_a)) + 127) // 128 * 128
    return int(min(4, max(1, 16384 // cap)))


def sym_items(upairs, counts, S, rows_wg=1024):
    """Item table [n_items][3] int32 of iamx_knn2sym_sweep_items: (first unordered pair, pair count,
    B slice).  Items of S consecutive pairs of `upairs` ((B, A), sorted by B: sym_tables); an item
    may cross a change of B image (the kernel reloads B there), which keeps every item S pairs long
    -- the item count of a launch a multiple of the CU count where the pair count allows it -- but
    it never mixes pairs of different slice counts (nwg).  The slices of one run of pairs are the
    fastest-moving index: they get consecutive workgroup ids (one XCD, the A rows from L2)."""
    upairs = np.asarray(upairs, np.int64).reshape(-1, 2)
    counts = np.asarray(counts, np.int64)
    n_u = len(upairs)
    if n_u == 0:
        return np.zeros((0, 3), np.int32)
    nwg = (counts[upairs[:, 0]] + rows_wg - 1) // rows_wg
    # runs of pairs with equal nwg, each cut into pieces of at most S pairs
    brk = np.flatnonzero(np.diff(nwg)) + 1
    starts, ends = np.concatenate([[0], brk]), np.concatenate([brk, [n_u]])
    first = np.concatenate([np.arange(a, b, S) for a, b in zip(starts, ends)])
    cnt = np.minimum(S, ends[np.searchsorted(ends, first, side='right')] - first)
    k = nwg[first]
    it = np.zeros((int(k.sum()), 3), np.int32)
    it[:, 0] = np.repeat(first, k)
    it[:, 1] = np.repeat(cnt, k)
    it[:, 2] = np.arange(len(it)) - np.repeat(np.cumsum(k) - k, k)
    return it


def knn2_pairs(store, pairs):
    """Exact 2-NN for a batch of ordered (query image, train image) pairs.

    Returns (idx, d2, out_off): idx/d2 int32 device tensors [sum n_q, 2], out_off a numpy
    int64 [n_pairs+1] of each pair's first output row."""
    dev = require_gpu()
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    counts = np.asarray(store.counts, np.int64)
    P = len(pairs)
    nq = counts[pairs[:, 0]] if P else np.zeros(0, np.int64)
    if P and counts[pairs[:, 1]].min() < 2:
        raise ValueError("train image with fewer than 2 descriptors "
                         "(the reference returns no matches there, lib/matcher.py:205-210)")
    out_off = np.zeros(P + 1, np.int64)
    np.cumsum(nq, out=out_off[1:])
    wg = np.zeros(P + 1, np.int64)
    np.cumsum((nq + 255) // 256, out=wg[1:])
    if wg[-1] >= 2 ** 31:
        raise ValueError("batch too large: split the pair list")
    total = int(out_off[-1])
    idx = torch.empty((max(total, 1), 2), dtype=I32, device=dev)
    d2 = torch.empty((max(total, 1), 2), dtype=I32, device=dev)
    if P == 0 or total == 0:
        return idx[:0], d2[:0], out_off
    d_pairs = torch.from_numpy(pairs).to(dev)
    d_wg = torch.from_numpy(wg.astype(np.int32)).to(dev)
    d_out = torch.from_numpy(out_off[:-1].copy()).to(dev)
    check(lib().iamx_knn2_l2_pairs(_ptr(store.desc), _ptr(store.norm_q), _ptr(store.norm_t),
                                   _ptr(store.img_off), _ptr(store.img_n), _ptr(d_pairs),
                                   _ptr(d_wg), _ptr(d_out), P, int(wg[-1]), _ptr(idx), _ptr(d2),
                                   stream_ptr()), 'iamx_knn2_l2_pairs')
    torch.cuda.current_stream().synchronize()      # launch tables are temporaries
    return idx[:total], d2[:total], out_off


def knn3_pairs(store, pairs):
    """Exact 3-NN for a batch of ordered (query image, train image) pairs (csrc/match_knn3.hip): what
    the 'smart' strategy's per-row walk reads.

    Returns (idx, d2, out_off) as knn2_pairs does, with idx/d2 int32 device tensors [sum n_q, 3]
    ascending by (squared distance, train row); a train image of exactly 2 rows leaves the third
    neighbour as idx = -1, d2 = 0x7FFFFFFF."""
    dev = require_gpu()
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    counts = np.asarray(store.counts, np.int64)
    P = len(pairs)
    if P and (pairs.min() < 0 or pairs.max() >= len(counts)):
        raise ValueError("pair list names an image the store does not hold")
    nq = counts[pairs[:, 0]] if P else np.zeros(0, np.int64)
    if P and counts[pairs[:, 1]].min() < 2:
        raise ValueError("train image with fewer than 2 descriptors "
                         "(the reference returns no matches there, lib/matcher.py:205-210)")
    out_off = np.zeros(P + 1, np.int64)
    np.cumsum(nq, out=out_off[1:])
    wg = np.zeros(P + 1, np.int64)
    np.cumsum((nq + 255) // 256, out=wg[1:])
    if wg[-1] >= 2 ** 31:
        raise ValueError("batch too large: split the pair list")
    total = int(out_off[-1])
    idx = torch.empty((max(total, 1), 3), dtype=I32, device=dev)
    d2 = torch.empty((max(total, 1), 3), dtype=I32, device=dev)
    if P == 0 or total == 0:
        return idx[:0], d2[:0], out_off
    d_pairs = torch.from_numpy(pairs).to(dev)
    d_wg = torch.from_numpy(wg.astype(np.int32)).to(dev)
    d_out = torch.from_numpy(out_off[:-1].copy()).to(dev)
    check(lib().iamx_knn3_l2_pairs(_ptr(store.desc), _ptr(store.norm_q), _ptr(store.norm_t),
                                   _ptr(store.img_off), _ptr(store.img_n), _ptr(d_pairs),
                                   _ptr(d_wg), _ptr(d_out), P, int(wg[-1]), _ptr(idx), _ptr(d2),
                                   stream_ptr()), 'iamx_knn3_l2_pairs')
    torch.cuda.current_stream().synchronize()      # launch tables are temporaries
    return idx[:total], d2[:total], out_off


def knn3(des_q, des_t):
    """Single pair convenience (packs both sides): returns device (idx[nq,3], d2[nq,3])."""
    idx, d2, _off = knn3_pairs(DescriptorStore.from_arrays([des_q, des_t]), [(0, 1)])
    return idx, d2


def knn2(des_q, des_t):
    """Single pair convenience (packs both sides): returns device (idx[nq,2], d2[nq,2])."""
    dev = require_gpu()
    st = DescriptorStore.from_arrays([des_q, des_t])
    nq, nt = st.counts
    idx = torch.empty((max(nq, 1), 2), dtype=I32, device=dev)
    d2 = torch.empty((max(nq, 1), 2), dtype=I32, device=dev)
    o = int(st.offsets[1])
    check(lib().iamx_knn2_l2_u8(_ptr(st.desc), _ptr(st.norm_q), nq, _ptr(st.desc[o:]),
                                _ptr(st.norm_t[o:]), nt, _ptr(idx), _ptr(d2), stream_ptr()),
          'iamx_knn2_l2_u8')
    torch.cuda.current_stream().synchronize()
    return idx[:nq], d2[:nq]


# --------------------------------------------------------------------------------------
# metric filter + compaction
# --------------------------------------------------------------------------------------
def match_metric(d2, seg_off, thresh):
    """d2 [n,2] int32 device; seg_off numpy/tensor int64 [n_seg+1].  Returns device tensors
    (metric f64 [n], keep u8 [n], seg_count i32 [n_seg]) and the number of d1==0 rows."""
    dev = require_gpu()
    n = d2.shape[0]
    seg = _dev(seg_off, I64)
    n_seg = seg.numel() - 1
    metric = torch.empty(max(n, 1), dtype=F64, device=dev)
    keep = torch.empty(max(n, 1), dtype=U8, device=dev)
    cnt = torch.zeros(max(n_seg, 1), dtype=I32, device=dev)
    zd = torch.zeros(1, dtype=I32, device=dev)
    check(lib().iamx_match_metric(_ptr(d2), _ptr(seg), n_seg, float(thresh), _ptr(metric),
                                  _ptr(keep), _ptr(cnt), _ptr(zd), stream_ptr()),
          'iamx_match_metric')
    return metric[:n], keep[:n], cnt[:n_seg], zd


def exclusive_scan(counts):
    dev = require_gpu()
    n = counts.numel()
    out = torch.empty(n + 1, dtype=I64, device=dev)
    check(lib().iamx_exclusive_scan_i32(_ptr(counts), n, _ptr(out), stream_ptr()),
          'iamx_exclusive_scan_i32')
    return out


def match_compact(idx, metric, keep, seg_off, surv_off, total):
    dev = require_gpu()
    seg = _dev(seg_off, I64)
    n_seg = seg.numel() - 1
    sq = torch.empty(max(total, 1), dtype=I32, device=dev)
    stt = torch.empty(max(total, 1), dtype=I32, device=dev)
    sm = torch.empty(max(total, 1), dtype=F64, device=dev)
    check(lib().iamx_match_compact(_ptr(idx), 2, _ptr(metric), _ptr(keep), _ptr(seg), _ptr(surv_off),
                                   n_seg, _ptr(sq), _ptr(stt), _ptr(sm), stream_ptr()),
          'iamx_match_compact')
    return sq[:total], stt[:total], sm[:total]


# --------------------------------------------------------------------------------------
# bundle adjustment
# --------------------------------------------------------------------------------------
def ba_residual(cams, pts, cam_idx, pt_idx, uv, calib, out=None):
    """All arguments device tensors (f64 / i32).  Returns r [2*n_obs] f64."""
    dev = require_gpu()
    n_obs = cam_idx.numel()
    r = out if out is not None else torch.empty(max(2 * n_obs, 1), dtype=F64, device=dev)
    check(lib().iamx_ba_residual(_ptr(cams), cams.numel() // 7, _ptr(pts), pts.numel() // 3,
                                 _ptr(cam_idx), _ptr(pt_idx), _ptr(uv), n_obs, _ptr(calib),
                                 _ptr(r), stream_ptr()), 'iamx_ba_residual')
    return r[:2 * n_obs]


def ba_residual_jac(cams, pts, cam_idx, pt_idx, uv, calib, with_calib=False):
    dev = require_gpu()
    n_obs = cam_idx.numel()
    r = torch.empty(max(2 * n_obs, 1), dtype=F64, device=dev)
    Jc = torch.empty((max(n_obs, 1), 2, 7), dtype=F64, device=dev)
    Jp = torch.empty((max(n_obs, 1), 2, 3), dtype=F64, device=dev)
    Jk = torch.empty((max(n_obs, 1), 2, 8), dtype=F64, device=dev) if with_calib else None
    check(lib().iamx_ba_residual_jac(_ptr(cams), cams.numel() // 7, _ptr(pts), pts.numel() // 3,
                                     _ptr(cam_idx), _ptr(pt_idx), _ptr(uv), n_obs, _ptr(calib),
                                     _ptr(r), _ptr(Jc), _ptr(Jp), _ptr(Jk), stream_ptr()),
          'iamx_ba_residual_jac')
    return r[:2 * n_obs], Jc[:n_obs], Jp[:n_obs], (Jk[:n_obs] if with_calib else None)


# summary layout of iamx_ba_reproj_stats / iamx_ba_mark_outliers (include/iamx.h)
REPROJ_N, REPROJ_SUM_E, REPROJ_MRE_E, REPROJ_MEAN_ABS_R, REPROJ_STD_R, REPROJ_MAX_ABS_R, \
    REPROJ_MEAN_R, REPROJ_EMPTY_CAMS, REPROJ_STDDEV_E, REPROJ_THRESHOLD, REPROJ_COUNT = range(11)
MRE_TILE = 2048


def ba_reproj_stats(cams, pts, cam_idx, pt_idx, uv, calib, cam_ptr, with_e=True):
    """Pass 1 of the reprojection-error report: device tensors in (as ba_residual, plus cam_ptr
    int64 [C+1]); returns device tensors (cam_stats [C, 3] = mean e, max e, count; summary [16];
    e [n_obs] or None).  Enqueued on the current stream, no synchronisation."""
    dev = require_gpu()
    n_obs = cam_idx.numel()
    n_cams = cams.numel() // 7
    if cam_ptr.numel() != n_cams + 1 or cam_ptr.dtype != torch.int64:
        raise ValueError('cam_ptr must be int64 [n_cams + 1]')
    cam_stats = torch.empty((n_cams, 3), dtype=F64, device=dev)
    part = torch.empty((n_cams, 8), dtype=F64, device=dev)
    summary = torch.full((16,), float('nan'), dtype=F64, device=dev)
    e = torch.empty(max(n_obs, 1), dtype=F64, device=dev) if with_e else None
    check(lib().iamx_ba_reproj_stats(_ptr(cams), n_cams, _ptr(pts), pts.numel() // 3,
                                     _ptr(cam_idx), _ptr(pt_idx), _ptr(uv), n_obs, _ptr(calib),
                                     _ptr(cam_ptr), _ptr(cam_stats), _ptr(part), _ptr(summary),
                                     _ptr(e), stream_ptr()), 'iamx_ba_reproj_stats')
    return cam_stats, summary, (e[:n_obs] if with_e else None)


def ba_mark_outliers(e, summary, trim_stddev, max_error=None, cap=None):
    """Pass 2: flags e > mre + stddev * trim_stddev (or e > max_error when max_error is not None)
    with the device-side mre of `summary` (updated in place: stddev, threshold, count).  Returns
    device tensors (idx int64 [cap], e_sel [cap]); the first int(summary[REPROJ_COUNT]) entries
    (at most cap, default n_obs) are the flagged observations in ascending order."""
    dev = require_gpu()
    n_obs = e.numel()
    cap = n_obs if cap is None else int(cap)
    n_tiles = (n_obs + MRE_TILE - 1) // MRE_TILE
    work = torch.empty(max(1, 3 * n_tiles), dtype=F64, device=dev)
    idx = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    e_sel = torch.empty(max(cap, 1), dtype=F64, device=dev)
    check(lib().iamx_ba_mark_outliers(_ptr(e), n_obs, float(trim_stddev), int(max_error is not None),
                                      float(max_error) if max_error is not None else 0.0,
                                      _ptr(summary), _ptr(work), _ptr(idx), _ptr(e_sel), cap,
                                      stream_ptr()), 'iamx_ba_mark_outliers')
    return idx[:cap], e_sel[:cap]


# --------------------------------------------------------------------------------------
# RANSAC verification of pair matches (csrc/match_verify.hip)
# --------------------------------------------------------------------------------------
VERIFY_MODELS = {'homography': 0, 'fundamental': 1, 'essential': 2}
VERIFY_OK, VERIFY_TOO_FEW, VERIFY_NO_MODEL = 0, 1, 2


def verify_pairs(pts, m_off, model, tol, hypotheses=2048, seed=0, K=None, return_essential=False):
    """pts [total, 4] float32 (x1 y1 x2 y2, undistorted pixels), m_off [n_pairs + 1] int64, model
    'homography' | 'fundamental' | 'essential' (or the ABI's number), tol [n_pairs] float64 pixels (or
    one number for all pairs).  'essential' needs the camera matrix K [3, 3] (host) and samples five
    matches on calibrated rays; the other models refuse a K.  Returns device tensors (mask uint8
    [total], model f64 [n_pairs, 3, 3], best int32 [n_pairs, 2] = hypothesis, inlier count, status
    int32 [n_pairs]); for 'essential' model is the pixel F = K^-T E K^-1, and return_essential adds E
    on normalised rays [n_pairs, 3, 3] as a fifth entry.  Stream ordered, nothing is synchronised."""
    dev = require_gpu()
    code = VERIFY_MODELS.get(model, model)
    if code not in (0, 1, 2):
        raise ValueError("verify_pairs: model must be 'homography', 'fundamental' or 'essential', "
                         "not %r" % (model,))
    if code == 2 and K is None:
        raise ValueError("verify_pairs: model 'essential' needs the camera matrix K")
    if code != 2 and (K is not None or return_essential):
        raise ValueError("verify_pairs: K and return_essential belong to model 'essential' only")
    pts = _dev(pts, torch.float32).reshape(-1, 4)
    m_off = _dev(m_off, I64).reshape(-1)
    n_pairs, total = m_off.numel() - 1, pts.shape[0]
    if n_pairs < 0:
        raise ValueError("verify_pairs: m_off needs n_pairs + 1 entries")
    if np.ndim(tol) == 0 and not isinstance(tol, torch.Tensor):
        tol = torch.full((max(n_pairs, 1),), float(tol), dtype=F64, device=dev)
    tol = _dev(tol, F64).reshape(-1)
    if tol.numel() < n_pairs:
        raise ValueError("verify_pairs: one tolerance per pair")
    mask = torch.empty(max(total, 1), dtype=U8, device=dev)
    out_model = torch.empty((max(n_pairs, 1), 3, 3), dtype=F64, device=dev)
    best = torch.empty((max(n_pairs, 1), 2), dtype=I32, device=dev)
    status = torch.empty(max(n_pairs, 1), dtype=I32, device=dev)
    if code == 2:
        Kh = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        ess = torch.empty((max(n_pairs, 1), 3, 3), dtype=F64, device=dev) if return_essential else None
        check(lib().iamx_verify_pairs_essential(
            _ptr(pts), _ptr(m_off), n_pairs, total, _lib.c_void_p(Kh.ctypes.data), _ptr(tol),
            int(hypotheses), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(mask), _ptr(out_model),
            _ptr(ess), _ptr(best), _ptr(status), stream_ptr()),
            'iamx_verify_pairs_essential')
        out = (mask[:total], out_model[:n_pairs], best[:n_pairs], status[:n_pairs])
        return out + (ess[:n_pairs],) if return_essential else out
    check(lib().iamx_verify_pairs(_ptr(pts), _ptr(m_off), n_pairs, total, code, _ptr(tol),
                                  int(hypotheses), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(mask),
                                  _ptr(out_model), _ptr(best), _ptr(status), stream_ptr()),
          'iamx_verify_pairs')
    return mask[:total], out_model[:n_pairs], best[:n_pairs], status[:n_pairs]


def five_point(rays):
    """The five-point solver alone (iamx_five_point): rays [n, 5, 4] float64 (x1 y1 x2 y2 on
    calibrated rays).  Returns device tensors (E f64 [n, 10, 3, 3]: unit Frobenius norm, largest
    entry positive, ascending in the solver's hidden variable, NaN past the count; count int32 [n])."""
    dev = require_gpu()
    rays = _dev(rays, F64)
    if rays.dim() != 3 or tuple(rays.shape[1:]) != (5, 4):
        raise ValueError("five_point: rays must be [n, 5, 4]")
    n = rays.shape[0]
    E = torch.empty((max(n, 1), 10, 3, 3), dtype=F64, device=dev)
    count = torch.empty(max(n, 1), dtype=I32, device=dev)
    if n == 0:                      # an empty tensor has no address to pass
        return E[:0], count[:0]
    check(lib().iamx_five_point(_ptr(rays), n, _ptr(E), _ptr(count), stream_ptr()), 'iamx_five_point')
    return E[:n], count[:n]


# --------------------------------------------------------------------------------------
# what the 'bestratio', 'smart' and 'bruteforce' strategies share (csrc/bin_select.h): a search, the
# rows of every pair in bins materialised as segments, verify_pairs over the segments, the select stage
# --------------------------------------------------------------------------------------
class _StrategyResult(object):
    """keyword constructor over a result class' __slots__ (a field not given is None)"""
    __slots__ = ()

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _tab_size(stride):
    """entries of a key table of the select stage: a power of two >= max(64, 2 * stride)"""
    t = 64
    while t < 2 * stride:
        t *= 2
    return t


def _live_pairs(store, pairs):
    """-> (pairs int32 [P, 2], nq int64 [P] the rows of every query image, live: the pairs whose two
    images both have at least 2 rows -- the others end with nothing, raw_matches' guards)"""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    counts = np.asarray(store.counts, np.int64)
    nq = counts[pairs[:, 0]] if len(pairs) else np.zeros(0, np.int64)
    ok = (nq >= 2) & (counts[pairs[:, 1]] >= 2) if len(pairs) else np.zeros(0, bool)
    return pairs, nq, np.nonzero(ok)[0]


def _split_by_bytes(live, nq, bytes_of, batch_bytes):
    """`live` cut into launches of at most batch_bytes each, at least one pair (a launch's stride is
    its largest query image: bytes_of takes the launch's query rows)"""
    chunks, a = [], 0
    while a < len(live):
        b = a + 1
        while b < len(live) and bytes_of(nq[live[a:b + 1]]) <= batch_bytes:
            b += 1
        chunks.append(live[a:b])
        a = b
    return chunks


def _bin_tables(P, nb, cap, dev):
    """-> bin_cnt, seg_cnt int32 [P, nb], seg_off int64 [P * nb + 1] (zeros), pts f32 [cap, 4], rows
    int32 [cap, 2] of the segments (at least one entry: an empty tensor has no address to pass)"""
    return (torch.zeros((P, nb), dtype=I32, device=dev), torch.zeros((P, nb), dtype=I32, device=dev),
            torch.zeros(P * nb + 1, dtype=I64, device=dev),
            torch.empty((max(cap, 1), 4), dtype=torch.float32, device=dev),
            torch.empty((max(cap, 1), 2), dtype=I32, device=dev))


def _select_buffers(P, stride, total, dev):
    """-> tab_size, work int32 [P * (6 * stride + 2 * tab_size)], slots int32 [P, stride, 2], cnt int32
    [P], off int64 [P + 1] (zeros), out_rows int32 [total, 2] of a select stage"""
    tab = _tab_size(stride)
    return (tab, torch.empty(P * (6 * stride + 2 * tab), dtype=I32, device=dev),
            torch.empty((P, stride, 2), dtype=I32, device=dev), torch.zeros(P, dtype=I32, device=dev),
            torch.zeros(P + 1, dtype=I64, device=dev), torch.empty((max(total, 1), 2), dtype=I32, device=dev))


class _Launch(object):
    """the tensors of one launch chain, by name"""


def _launch_chain(cls, store, pairs, knn, nb, per_row, tol, hypotheses, seed, flag, bins, select):
    """one launch chain over pairs whose images all have at least 2 rows: the search knn(store, pairs),
    bins(b) -- at most per_row segment entries a query row over nb segments a pair --, the consensus of
    every segment (iamx_verify_pairs on its points), select(b) -> the extra fields of cls"""
    dev = require_gpu()
    b = _Launch()
    b.P, b.flag = len(pairs), flag
    b.idx, b.d2, out_off = knn(store, pairs)
    b.total = int(out_off[-1])
    b.stride = max(int(np.diff(out_off).max()), 1)
    b.cap = per_row * b.total
    b.pairs = torch.from_numpy(np.ascontiguousarray(pairs, np.int32)).to(dev)
    b.row_off = torch.from_numpy(out_off).to(dev)
    b.bin_cnt, b.seg_cnt, b.seg_off, b.pts, b.rows = _bin_tables(b.P, nb, b.cap, dev)
    bins(b)
    b.mask, _model, _best, b.vstatus = verify_pairs(b.pts[:b.cap], b.seg_off, 'homography', float(tol),
                                                    hypotheses=hypotheses, seed=seed)
    b.tab, b.work, b.slots, b.cnt, b.off, b.out_rows = _select_buffers(b.P, b.stride, b.total, dev)
    return cls(rows=b.out_rows, off=b.off, cnt=b.cnt, flag=flag, slots=b.slots, stride=b.stride, **select(b))


def _merge_launches(cls, P, chunks, parts, flag, fields):
    """several launches' results side by side over all P pairs (copies and one scan, no arithmetic of
    their own).  fields: per extra field of cls its shape behind P and what a pair without a launch
    holds, a number or one per entry of the last axis; cnt is 0 there.  No slots: they are a launch's."""
    dev = flag.device
    out = dict(cnt=torch.zeros(P, dtype=I32, device=dev))
    for k, (shape, fill) in fields.items():
        out[k] = torch.tensor(fill, dtype=I32, device=dev).expand((P,) + shape).contiguous()
    rows = []
    for c, r in zip(chunks, parts):
        where = torch.from_numpy(c).to(dev)
        for k in out:
            out[k][where] = getattr(r, k)
        rows.append(r.rows[:int(r.off[-1])])
    off = exclusive_scan(out['cnt']) if P else torch.zeros(1, dtype=I64, device=dev)
    rows = torch.cat(rows) if rows else torch.empty((0, 2), dtype=I32, device=dev)
    return cls(rows=rows, off=off, flag=flag, slots=None, stride=parts[0].stride if len(parts) == 1 else None,
               **out)


# --------------------------------------------------------------------------------------
# the 'bestratio' strategy (csrc/match_ratio.hip): ratio bins -> RANSAC homography per bin -> select
# --------------------------------------------------------------------------------------
RATIO_CUTOFFS = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85)       # matcher.py:622
RATIO_MIN_UNIQUE = 20                                              # matcher.py:603
RATIO_BATCH_BYTES = 4 << 30


class RatioResult(_StrategyResult):
    """what ratio_pairs() returns, device tensors over its n pairs: rows int32 [total, 2] (query
    row, train row) packed back to back, off int64 [n + 1], cnt int32 [n], chosen int32 [n] (-1:
    no bin taken), stats int32 [n, n_bins, 3] = members, fit, unique (-1 where a bin is not looked
    at), flag int32 [2] (rows with a zero second distance, pairs refused).  slots int32 [n, stride,
    2]: the same lists in fixed slots (iamx_similarity_pairs' layout) when the call was one launch,
    else None."""
    __slots__ = ('rows', 'off', 'cnt', 'chosen', 'stats', 'flag', 'slots', 'stride')


def ratio_bytes(nq, n_bins=len(RATIO_CUTOFFS)):
    """device bytes one launch of ratio_pairs() over query images of `nq` rows (an array) takes:
    the top-2 rows (16 B), the materialised bins (n_bins x 25 B), the packed result (8 B) per query
    row, and per pair the select stage's slices at the launch's stride (work lists 24 B, result
    slot 8 B per row of the largest query image, two key tables of tab_size x 4 B)"""
    nq = np.asarray(nq, np.int64).reshape(-1)
    if not len(nq):
        return 0
    stride = max(int(nq.max()), 1)
    return int(nq.sum()) * (24 + 25 * n_bins) + len(nq) * (32 * stride + 8 * _tab_size(stride) + 64 * n_bins)


def _ratio_launch(store, pairs, kp_off, xy, key2, tol, min_pairs, hypotheses, seed, cut, flag):
    L = lib()
    nb = len(cut)

    def bins(b):
        check(L.iamx_ratio_bins(_ptr(b.idx), _ptr(b.d2), _ptr(b.row_off), _ptr(b.pairs), _ptr(kp_off), _ptr(xy),
                                b.P, nb, _lib.c_void_p(cut.ctypes.data), float(min_pairs), b.cap,
                                _ptr(b.bin_cnt), _ptr(b.seg_cnt), _ptr(b.seg_off), _ptr(b.pts), _ptr(b.rows),
                                _ptr(flag), stream_ptr()), 'iamx_ratio_bins')

    def select(b):
        chosen = torch.zeros(b.P, dtype=I32, device=flag.device)
        stats = torch.zeros((b.P, nb, 3), dtype=I32, device=flag.device)
        check(L.iamx_ratio_select(_ptr(b.pairs), _ptr(kp_off), _ptr(key2), b.P, nb, float(min_pairs),
                                  RATIO_MIN_UNIQUE, _ptr(b.bin_cnt), _ptr(b.seg_cnt), _ptr(b.seg_off),
                                  _ptr(b.rows), _ptr(b.mask), _ptr(b.vstatus), b.cap, b.stride, b.tab,
                                  _ptr(b.work), _ptr(b.slots), _ptr(b.cnt), _ptr(b.off), _ptr(b.out_rows),
                                  b.total, _ptr(chosen), _ptr(stats), _ptr(flag), stream_ptr()),
              'iamx_ratio_select')
        return dict(chosen=chosen, stats=stats)

    return _launch_chain(RatioResult, store, pairs, knn2_pairs, nb, nb, tol, hypotheses, seed, flag, bins, select)


def ratio_pairs(store, pairs, kp_off, xy, key2, tol, min_pairs, hypotheses, seed,
                cutoffs=RATIO_CUTOFFS, batch_bytes=RATIO_BATCH_BYTES):
    """scripts/lib/matcher.py:595-694 ratio_pair_matches() for a batch of ordered (query image, train
    image) pairs of `store`: exact k=2 neighbours (knn2_pairs), Lowe-ratio bins, a RANSAC homography
    per bin at `tol` pixels (verify_pairs' rule with `hypotheses` and `seed`), the bin with the most
    unique inliers, the min_pairs gates.  kp_off / xy / key2: the keypoint arena of the store's
    slots (DeviceMatcher.keypoints()).  A pair with an image of at most 1 row ends with nothing
    (raw_matches' guards).  The work is enqueued on the current stream in launches of at most
    batch_bytes of device memory each (ratio_bytes); -> RatioResult."""
    dev = require_gpu()
    cut = np.ascontiguousarray(cutoffs, np.float64).reshape(-1)
    nb = len(cut)
    if not 1 <= nb <= 8:
        raise ValueError("ratio_pairs: 1 to 8 cutoffs")
    pairs, nq, live = _live_pairs(store, pairs)
    chunks = _split_by_bytes(live, nq, lambda q: ratio_bytes(q, nb), batch_bytes)
    flag = torch.zeros(2, dtype=I32, device=dev)            # (the launches only ever raise it)
    parts = [_ratio_launch(store, pairs[c], kp_off, xy, key2, tol, min_pairs, hypotheses, seed, cut, flag)
             for c in chunks]
    if len(parts) == 1 and len(live) == len(pairs):
        return parts[0]
    return _merge_launches(RatioResult, len(pairs), chunks, parts, flag,
                           dict(chosen=((), -1), stats=((nb, 3), (0, -1, -1))))


# --------------------------------------------------------------------------------------
# the 'smart' strategy (csrc/match_knn3.hip, csrc/match_smart.hip): per pass, candidate choice and
# distance bins -> RANSAC homography per bin -> select + least-squares refit
# --------------------------------------------------------------------------------------
SMART_CUTOFFS = (32, 64, 128, 256, 512, 1024, 2048)                # matcher.py:516
SMART_MIN_UNIQUE = 20                                              # matcher.py:468
FIT_OK, FIT_TOO_FEW, FIT_DEGENERATE = 0, 1, 2


def homography_fit(pts, seg_off, mask=None):
    """Least-squares homographies x2 ~ H x1 (iamx_homography_fit: cv2's kernel without its LM
    polish) of segments of correspondences: pts [total, 4] float32 (x1 y1 x2 y2), seg_off [n + 1]
    int64, mask [total] uint8 or None (only points with a non-zero byte count).  Returns device
    tensors (H f64 [n, 3, 3] with h22 = 1, NaN where status != FIT_OK; status int32 [n]).  Stream
    ordered, nothing is synchronised."""
    dev = require_gpu()
    pts = _dev(pts, torch.float32).reshape(-1, 4)
    seg_off = _dev(seg_off, I64).reshape(-1)
    n, total = seg_off.numel() - 1, pts.shape[0]
    if n < 0:
        raise ValueError("homography_fit: seg_off needs n + 1 entries")
    if mask is not None:
        mask = _dev(mask, U8).reshape(-1)
        if mask.numel() != total:
            raise ValueError("homography_fit: one mask byte per point")
    H = torch.empty((max(n, 1), 3, 3), dtype=F64, device=dev)
    status = torch.empty(max(n, 1), dtype=I32, device=dev)
    if n == 0:
        return H[:0], status[:0]
    if total == 0:                              # an empty tensor has no address to pass
        pts = torch.zeros((1, 4), dtype=torch.float32, device=dev)
    check(lib().iamx_homography_fit(_ptr(pts), _ptr(seg_off), _ptr(mask), n, total, _ptr(H), _ptr(status),
                                    stream_ptr()), 'iamx_homography_fit')
    return H[:n], status[:n]


class SmartResult(_StrategyResult):
    """what smart_pairs() returns over its n pairs: rows int32 [total, 2] (query row, train row)
    packed back to back, off int64 [n + 1], cnt int32 [n] (device tensors: the lists after the
    min_pairs gates and filter_duplicates); H f64 [n, 3, 3] the last prediction of every pair (device);
    passes int [n] (host) the passes every pair went through, the last one without a gain included;
    stats: one int32 [n, 7, 3] host array per pass = members, fit, unique per bin (-1, -1 where a bin
    is not looked at; a pair that did not take part in the pass: -2 throughout); taken: one int32 [n]
    host array per pass, 1 + the last bin that raised the pair's best (0: none); best int32 [n, 2]
    (host) = unique, fitted of the final lists before the gates; flag int32 [2] (host): rows with a
    zero nearest distance, pairs refused."""
    __slots__ = ('rows', 'off', 'cnt', 'H', 'passes', 'stats', 'taken', 'best', 'flag')


def smart_pairs(store, pairs, kp_off, xy, size, key2, H0, tol, min_pairs, match_ratio, hypotheses=2048,
                seed=0, knn=None, max_passes=None):
    """scripts/lib/matcher.py:465-593 -- smart_pair_matches() from its k = 3 search on -- for a batch
    of ordered (query image, train image) pairs of `store`.  kp_off / xy / key2: the keypoint arena
    of the store's slots (DeviceMatcher.keypoints()), size: kp.size beside xy (DeviceMatcher.sizes());
    H0 [n, 3, 3] float64: every pair's predicted homography (matcher.smart_prior).  Per pass, for the
    pairs whose best rose in the pass before (all in the first): iamx_smart_stats -> verify_pairs'
    consensus at `tol` pixels with `hypotheses` and `seed` over the 7 bins -> iamx_smart_select; one
    word per pair is read back.  knn: (idx, d2, out_off) of knn3_pairs(store, pairs) when the caller
    ran the search ahead.  A pair with an image of at most 1 row ends with nothing (raw_matches'
    guards).  max_passes: stop early (tests).  -> SmartResult."""
    dev = require_gpu()
    L = lib()
    NB = len(SMART_CUTOFFS)
    pairs, _nq, live = _live_pairs(store, pairs)
    P, n = len(pairs), len(live)
    H0 = np.ascontiguousarray(np.asarray(H0, np.float64).reshape(-1, 9))
    if len(H0) != P:
        raise ValueError("smart_pairs: one predicted homography per pair")
    if knn is not None and n != P:
        raise ValueError("smart_pairs: a search handed in covers pairs of images with at least 2 rows only")
    passes = np.zeros(P, np.int64)
    res = SmartResult(passes=passes, stats=[], taken=[], flag=np.zeros(2, np.int32),
                      best=np.tile(np.array([SMART_MIN_UNIQUE, 0], np.int32), (P, 1)))
    H = torch.from_numpy(H0.copy()).to(dev)
    cnt_all = torch.zeros(P, dtype=I32, device=dev)
    if n == 0:
        res.rows, res.off, res.cnt, res.H = (torch.empty((0, 2), dtype=I32, device=dev),
                                             torch.zeros(P + 1, dtype=I64, device=dev), cnt_all, H.view(P, 3, 3))
        return res
    idx, d2, out_off = knn if knn is not None else knn3_pairs(store, pairs[live])
    total = int(out_off[-1])
    stride = max(int(np.diff(out_off).max()), 1)
    cap = NB * total
    z32 = lambda *shape: torch.zeros(shape, dtype=I32, device=dev)
    d_pairs = torch.from_numpy(np.ascontiguousarray(pairs[live])).to(dev)
    row_off = torch.from_numpy(np.ascontiguousarray(out_off, np.int64)).to(dev)
    Hl = H[torch.from_numpy(live).to(dev)].contiguous() if n != P else H
    bin_cnt, seg_cnt, seg_off, pts, rows = _bin_tables(n, NB, cap, dev)
    flag = z32(2)
    tab, work, slots, cnt, off, out_rows = _select_buffers(n, stride, total, dev)
    best = torch.from_numpy(np.tile(np.array([SMART_MIN_UNIQUE, 0], np.int32), (n, 1))).to(dev)
    improved, fit_status = z32(n), z32(n)
    stats = z32(n, NB, 3)
    active = torch.ones(n, dtype=I32, device=dev)
    act_h = np.ones(n, bool)
    while act_h.any() and (max_passes is None or len(res.stats) < max_passes):
        check(L.iamx_smart_stats(_ptr(idx), _ptr(d2), _ptr(row_off), _ptr(d_pairs), _ptr(kp_off), _ptr(xy),
                                 _ptr(size), _ptr(Hl), _ptr(active), n, float(match_ratio), float(min_pairs),
                                 cap, _ptr(bin_cnt), _ptr(seg_cnt), _ptr(seg_off), _ptr(pts), _ptr(rows),
                                 _ptr(flag), stream_ptr()), 'iamx_smart_stats')
        mask, model, _best, vstatus = verify_pairs(pts[:cap], seg_off, 'homography', float(tol),
                                                   hypotheses=hypotheses, seed=seed)
        check(L.iamx_smart_select(_ptr(d_pairs), _ptr(kp_off), _ptr(key2), _ptr(active), n, float(min_pairs),
                                  _ptr(bin_cnt), _ptr(seg_cnt), _ptr(seg_off), _ptr(pts), _ptr(rows),
                                  _ptr(mask), _ptr(vstatus), _ptr(model), cap, stride, tab, _ptr(work),
                                  _ptr(best), _ptr(improved), _ptr(slots), _ptr(cnt), _ptr(off),
                                  _ptr(out_rows), total, _ptr(stats), _ptr(Hl), _ptr(fit_status), _ptr(flag),
                                  stream_ptr()), 'iamx_smart_select')
        taken = improved.cpu().numpy()                      # (the one read of the pass: it synchronises)
        passes[live[act_h]] += 1
        st_h = np.full((P, NB, 3), -2, np.int32)
        st_h[live[act_h]] = stats.cpu().numpy()[act_h]
        tk_h = np.zeros(P, np.int32)
        tk_h[live] = taken
        res.stats.append(st_h)
        res.taken.append(tk_h)
        res.flag = flag.cpu().numpy()
        if res.flag.any():
            break                                           # (the caller raises: python stops at that row)
        act_h = taken > 0
        active.copy_(torch.from_numpy(act_h.astype(np.int32)))
    res.best[live] = best.cpu().numpy()
    if n == P:
        res.rows, res.off, res.cnt, res.H = out_rows, off, cnt, Hl.view(P, 3, 3)
        return res
    where = torch.from_numpy(live).to(dev)
    cnt_all[where] = cnt
    H[where] = Hl
    res.rows, res.cnt, res.H = out_rows, cnt_all, H.view(P, 3, 3)
    res.off = exclusive_scan(cnt_all)
    return res


# --------------------------------------------------------------------------------------
# the 'bruteforce' strategy (csrc/match_knn3.hip, csrc/match_brute.hip): candidate choice and 41 x 21
# motion cells -> RANSAC homography per cell -> the walk with the early exit
# --------------------------------------------------------------------------------------
BRUTE_DIST_BINS, BRUTE_ANGLE_BINS = 41, 21                        # matcher.py:758, :779 (divs + 1)
BRUTE_CELLS = BRUTE_DIST_BINS * BRUTE_ANGLE_BINS
BRUTE_STEP_A = 2 * math.pi / (BRUTE_ANGLE_BINS - 1)               # matcher.py:780
BRUTE_BATCH_BYTES = 4 << 30


class BruteResult(_StrategyResult):
    """what brute_pairs() returns, device tensors over its n pairs: rows int32 [total, 2] (query
    row, train row) packed back to back, off int64 [n + 1], cnt int32 [n], chosen int32 [n] (the
    taken cell dbin * 21 + abin, -1: none), stats int32 [n, 4] = fitted, unique (-1: the
    de-duplication did not run), distance bins walked, cells looked at within them, fit_cnt int32
    [n, 861] the fitted inliers of every cell (-1: not looked at or not reached), bin_cnt int32
    [n, 861] the members of every cell, flag int32 [2] (rows with a zero nearest distance, pairs
    refused).  slots int32 [n, stride, 2]: the same lists in fixed slots (iamx_similarity_pairs'
    layout) when the call was one launch, else None."""
    __slots__ = ('rows', 'off', 'cnt', 'chosen', 'stats', 'fit_cnt', 'bin_cnt', 'flag', 'slots', 'stride')


def brute_bytes(nq):
    """device bytes one launch of brute_pairs() over query images of `nq` rows (an array) takes: the
    top-3 rows (24 B), nine materialised members (9 x 25 B), the packed result (8 B) per query row,
    and per pair the 861-wide tables (members, segments, offsets, status, best, model, fitted: 112 B
    a cell) and the select stage's slices at the launch's stride (work lists 24 B, result slot 8 B per
    row of the largest query image, two key tables of tab_size x 4 B)"""
    nq = np.asarray(nq, np.int64).reshape(-1)
    if not len(nq):
        return 0
    stride = max(int(nq.max()), 1)
    return int(nq.sum()) * (32 + 25 * 9) + len(nq) * (32 * stride + 8 * _tab_size(stride) + 112 * BRUTE_CELLS)


def _brute_launch(store, pairs, kp_off, xy, size, key2, tol, min_pairs, match_ratio, step_d, hypotheses,
                  seed, flag):
    L = lib()
    NC = BRUTE_CELLS

    def bins(b):
        check(L.iamx_brute_bins(_ptr(b.idx), _ptr(b.d2), _ptr(b.row_off), _ptr(b.pairs), _ptr(kp_off), _ptr(xy),
                                _ptr(size), b.P, float(match_ratio), float(min_pairs), float(step_d),
                                BRUTE_STEP_A, b.cap, _ptr(b.bin_cnt), _ptr(b.seg_cnt), _ptr(b.seg_off),
                                _ptr(b.pts), _ptr(b.rows), _ptr(flag), stream_ptr()), 'iamx_brute_bins')

    # (the consensus runs on every cell, the cells the early exit leaves unreached included: the walk
    #  alone is pruned)
    def select(b):
        z32 = lambda *shape: torch.zeros(shape, dtype=I32, device=flag.device)
        chosen, stats, fit_cnt = z32(b.P), z32(b.P, 4), z32(b.P, NC)
        check(L.iamx_brute_select(_ptr(b.pairs), _ptr(kp_off), _ptr(key2), b.P, float(min_pairs),
                                  _ptr(b.seg_cnt), _ptr(b.seg_off), _ptr(b.rows), _ptr(b.mask), _ptr(b.vstatus),
                                  b.cap, b.stride, b.tab, _ptr(b.work), _ptr(b.slots), _ptr(b.cnt), _ptr(b.off),
                                  _ptr(b.out_rows), b.total, _ptr(chosen), _ptr(stats), _ptr(fit_cnt),
                                  _ptr(flag), stream_ptr()), 'iamx_brute_select')
        return dict(chosen=chosen, stats=stats, fit_cnt=fit_cnt, bin_cnt=b.bin_cnt)

    # (a query row is in at most 3 x 3 cells)
    return _launch_chain(BruteResult, store, pairs, knn3_pairs, NC, 9, tol, hypotheses, seed, flag, bins, select)


def brute_pairs(store, pairs, kp_off, xy, size, key2, tol, min_pairs, match_ratio, step_d, hypotheses,
                seed, batch_bytes=BRUTE_BATCH_BYTES):
    """scripts/lib/matcher.py:696-850 bruteforce_pair_matches() for a batch of ordered (query image,
    train image) pairs of `store`: exact k=3 neighbours (knn3_pairs), the per-row choice and the 41 x
    21 motion cells (iamx_brute_bins; step_d = int(diag * 0.55) / 40), a RANSAC homography per cell
    at `tol` pixels (verify_pairs' rule with `hypotheses` and `seed`) over all n_pairs * 861 segments
    in one launch, the walk with the early exit and the min_pairs gates (iamx_brute_select).  kp_off
    / xy / key2: the keypoint arena of the store's slots (DeviceMatcher.keypoints()), size: kp.size
    beside xy (DeviceMatcher.sizes()).  A pair with an image of at most 1 row ends with nothing
    (raw_matches' guards).  The work is enqueued on the current stream in launches of at most
    batch_bytes of device memory each (brute_bytes); -> BruteResult."""
    dev = require_gpu()
    NC = BRUTE_CELLS
    if not (float(step_d) > 0.0 and math.isfinite(float(step_d))):
        raise ValueError("brute_pairs: step_d must be positive and finite")
    pairs, nq, live = _live_pairs(store, pairs)
    chunks = _split_by_bytes(live, nq, brute_bytes, batch_bytes)
    flag = torch.zeros(2, dtype=I32, device=dev)            # (the launches only ever raise it)
    parts = [_brute_launch(store, pairs[c], kp_off, xy, size, key2, tol, min_pairs, match_ratio, step_d,
                           hypotheses, seed, flag) for c in chunks]
    if len(parts) == 1 and len(live) == len(pairs):
        return parts[0]
    return _merge_launches(BruteResult, len(pairs), chunks, parts, flag,
                           dict(chosen=((), -1), stats=((4,), (0, -1, 0, 0)), fit_cnt=((NC,), -1),
                                bin_cnt=((NC,), 0)))


# --------------------------------------------------------------------------------------
# a reusable, allocation-free batch of ordered pairs: knn2 -> metric -> scan -> compaction
# --------------------------------------------------------------------------------------
class PairWorkspace(object):
    """Output buffers for up to `max_rows` query rows / `max_pairs` ordered pairs."""

    def __init__(self, max_rows, max_pairs):
        dev = require_gpu()
        r, p = max(int(max_rows), 1), max(int(max_pairs), 1)
        self.max_rows, self.max_pairs = r, p
        self.idx = torch.empty((r, 2), dtype=I32, device=dev)
        self.d2 = torch.empty((r, 2), dtype=I32, device=dev)
        self.metric = torch.empty(r, dtype=F64, device=dev)
        self.keep = torch.empty(max(r, 8), dtype=U8, device=dev)   # (the symmetric form's bit map: whole words)
        self.seg_count = torch.zeros(p, dtype=I32, device=dev)
        self.surv_off = torch.zeros(p + 1, dtype=I64, device=dev)
        self.surv_q = torch.empty(r, dtype=I32, device=dev)
        self.surv_t = torch.empty(r, dtype=I32, device=dev)
        self.surv_metric = torch.empty(r, dtype=F64, device=dev)
        # [0] a zero second distance was met (ZeroDivisionError of matcher.py:255), [1] rows the
        # bound form could not resolve exactly (must stay 0: find_matches refuses the batch)
        self.flags = torch.zeros(2, dtype=I32, device=dev)
        self.zero_div = self.flags[0:1]
        self.tile = torch.empty(r, dtype=I32, device=dev)
        self.unresolved = self.flags[1:2]
        self.surv_cnt = torch.zeros(p, dtype=I32, device=dev)
        # symmetric sweep: bounds per row (allocated on first use, grown when a batch needs more)
        self.col = self.rowp = self.colmask = self.nar = None
        self.cand_keep = torch.empty(r, dtype=U8, device=dev)
        # exact stage of the symmetric form: two task lists in one buffer (wave tasks from entry
        # 0, workgroup tasks from entry n_pairs) and their two counters
        self.task_total = torch.zeros(2, dtype=I32, device=dev)
        self.tasks = torch.empty((2 * p + r // 32 + 2, 2), dtype=I32, device=dev)

    def ensure_sym(self, col_rows, rowp_rows):
        dev = self.d2.device
        if self.col is None or self.col.shape[0] < col_rows:
            self.col = torch.empty((max(col_rows, 1), 2), dtype=I32, device=dev)
            # which of its eight train-row groups can hold a query's best / second (narrow exact stage)
            self.colmask = torch.empty(max(col_rows, 1), dtype=U8, device=dev)
        if self.nar is None:
            # items / tasks / partial results of the narrow exact stage, sized for the workspace's
            # row and pair capacity (its control words start at 0; the stage leaves them 0)
            self.nar = torch.zeros(max(int(lib().iamx_knn2sym_narrow_bytes(self.max_rows, self.max_pairs)),
                                       256), dtype=U8, device=dev)
        if self.rowp is None or self.rowp.shape[0] < rowp_rows:
            self.rowp = torch.empty((max(rowp_rows, 1), 2), dtype=I32, device=dev)

    def survivor_counts(self, n_pairs):
        """host copies of (first, count) per pair only"""
        first = self.surv_off[:n_pairs].cpu().numpy()
        count = self.surv_cnt[:n_pairs].cpu().numpy().astype(np.int64)
        return first, count

    def survivors(self, n_pairs):
        """host copies: (first, count) per pair and the survivor arrays they index
        (pair p owns [first[p], first[p] + count[p]); query rows ascending)."""
        first, count = self.survivor_counts(n_pairs)
        total = int(self.surv_off[n_pairs].item())
        return (first, count, self.surv_q[:total].cpu().numpy(),
                self.surv_t[:total].cpu().numpy(), self.surv_metric[:total].cpu().numpy())


class UploadArena(object):
    """Small host tables -> device without stalling the stream.  A pageable `tensor.to(device)`
    blocks the host until everything already enqueued has run -- in find_matches' software
    pipeline that is the previous round's 4 ms of kernels, per table, a dozen tables per round.
    The arena packs all tables of a round into ONE page-locked buffer and issues ONE asynchronous
    copy into a device buffer of a small ring (a slot is reused after the event behind its copy);
    the tensors it hands out are views of that device buffer, valid in stream order."""

    def __init__(self, nbytes=8 << 20, slots=4):
        dev = require_gpu()
        self.dev = dev
        self.slots = [dict(pin=torch.empty(nbytes, dtype=U8).pin_memory(),
                           dev=torch.empty(nbytes, dtype=U8, device=dev),
                           ev=torch.cuda.Event(), used=False) for _ in range(slots)]
        self.cur, self.off, self.k = None, 0, 0

    def begin(self):
        if self.cur is not None:
            self.commit()
        self.k = (self.k + 1) % len(self.slots)
        self.cur = self.slots[self.k]
        if self.cur['used']:
            self.cur['ev'].synchronize()
        self.off = 0

    def put(self, a):
        """numpy array -> device tensor (same dtype / shape) behind the arena's next commit()"""
        a = np.ascontiguousarray(a)
        nb = a.nbytes
        off = (self.off + 15) & ~15
        if self.cur is None or off + nb > self.cur['pin'].numel():
            return torch.from_numpy(a).to(self.dev)            # (does not fit: the plain way)
        if nb:
            self.cur['pin'].numpy()[off:off + nb] = a.reshape(-1).view(np.uint8)
        self.off = off + nb
        t = self.cur['dev'][off:off + nb].view(_TORCH_OF[a.dtype.str]) if nb else \
            torch.empty(0, dtype=_TORCH_OF[a.dtype.str], device=self.dev)
        return t.view(a.shape) if a.ndim != 1 else t

    def commit(self):
        c = self.cur
        if c is None:
            return
        if self.off:
            c['dev'][:self.off].copy_(c['pin'][:self.off], non_blocking=True)
        c['ev'].record()
        c['used'] = True
        self.cur = None


_TORCH_OF = {'<i4': torch.int32, '<i8': torch.int64, '<f4': torch.float32, '<f8': torch.float64,
             '|u1': torch.uint8, '|i1': torch.int8}


class PairBatch(object):
    """Device-side launch tables of one batch of ordered (query image, train image) pairs.
    `run()` only enqueues kernels on the current stream (no host sync, no allocation)."""

    def __init__(self, store, pairs, sym=None, arena=None):
        """sym: None = use the symmetric sweep (one MFMA pass for both directions of an image
        pair) when the batch holds both directions of every pair, False = never (one sweep per
        ordered pair), True = require it.  arena: an UploadArena between begin() and commit() --
        the launch tables go up with its one asynchronous copy."""
        dev = require_gpu()
        up = arena.put if arena is not None else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        self._up = up
        self.store = store
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        counts = np.asarray(store.counts, np.int64)
        self.pairs = pairs
        self.n_pairs = P = len(pairs)
        nq = counts[pairs[:, 0]] if P else np.zeros(0, np.int64)
        if P and counts[pairs[:, 1]].min() < 2:
            raise ValueError("train image with fewer than 2 descriptors")
        self.out_off = np.zeros(P + 1, np.int64)
        np.cumsum(nq, out=self.out_off[1:])
        wg = np.zeros(P + 1, np.int64)
        np.cumsum((nq + 255) // 256, out=wg[1:])
        if wg[-1] >= 2 ** 31:
            raise ValueError("batch too large: split the pair list")
        self.rows = int(self.out_off[-1])
        self.max_query_rows = int(nq.max()) if P else 0
        self.total_wg = int(wg[-1])
        self.d_pairs = up(pairs)
        self.d_wg = up(wg.astype(np.int32))
        self.d_out = up(self.out_off.copy())                           # also the metric seg_off
        # query rows per workgroup of the fast sweep (256 / 512 / 1024 by image size): bigger =
        # fewer LDS reads and barriers per MFMA
        self.fast_rows = 256 if not (P and nq.min() >= 2048) else (1024 if nq.min() >= 4096 else 512)
        wgf = np.zeros(P + 1, np.int64)
        np.cumsum((nq + self.fast_rows - 1) // self.fast_rows, out=wgf[1:])
        self.total_wg_fast = int(wgf[-1])
        self.d_wg_fast = up(wgf.astype(np.int32))
        self.sym = False
        if sym is not False:
            self._setup_sym(dev)
            if sym and not self.sym:
                raise ValueError("symmetric sweep needs both directions of every pair (i != j) "
                                 "in the batch")

    def _setup_sym(self, dev):
        t = sym_tables(self.pairs, self.store.counts, self.store.caps3)
        if t is None:
            return
        assert SYM_ROWS_PER_WG[t['form']] == int(lib().iamx_knn2sym_rows_per_wg(t['form']))
        self.sym = True
        self.sym_form = t['form']
        self.n_u, self.sym_total_wg = len(t['upairs']), int(t['wg'][-1])
        self.sym_col_rows, self.sym_rowp_rows = int(t['col_off'][-1]), int(t['rowp_off'][-1])
        up = self._up
        self.d_upairs = up(np.ascontiguousarray(t['upairs']))
        self.d_sym_wg = up(t['wg'].astype(np.int32))
        self.d_col_off = up(t['col_off'][:-1].copy())
        self.d_rowp_off = up(t['rowp_off'][:-1].copy())
        self.d_osrc = up(t['osrc'])
        self.sym_items_s = t['S']
        self.sym_items_entry = 'iamx_knn2sym_sweep_items16'
        # form 2 with S > 1 walks items of S pairs that share their B image; at S = 1 (long images) the
        # one-pair kernel runs: the item kernel with one pair per item measured 0.6-0.9 % slower there
        # (profiles/r8_sweep_time.txt)
        if self.sym_items_s > 1:
            items = sym_items(t['upairs'], self.store.counts, self.sym_items_s)
            self.n_sym_items = len(items)
            self.d_sym_items = up(items)

    def run_sym_sweep(self, ws):
        st = self.store
        ws.ensure_sym(self.sym_col_rows, self.sym_rowp_rows)
        if self.sym_items_s > 1:
            # the item walk on v_mfma_i32_16x16x64_i8: iamx_knn2sym_sweep_items' outputs, bit for bit
            # (`sym_items_entry`: tests run the 32x32x32 item kernel through the same batch)
            entry = self.sym_items_entry
            check(getattr(lib(), entry)(_ptr(st.desc3), _ptr(st.sn2), _ptr(st.sct), _ptr(st.img_off3),
                                        _ptr(st.img_n), _ptr(self.d_upairs), _ptr(self.d_sym_items),
                                        _ptr(self.d_col_off), _ptr(self.d_rowp_off), self.n_u,
                                        self.n_sym_items, _ptr(ws.col), _ptr(ws.rowp),
                                        _ptr(ws.colmask), stream_ptr()), entry)
            return
        check(lib().iamx_knn2sym_sweep(_ptr(st.desc3), _ptr(st.sn2), _ptr(st.sct), _ptr(st.img_off3),
                                       _ptr(st.img_n), _ptr(self.d_upairs), _ptr(self.d_sym_wg),
                                       _ptr(self.d_col_off), _ptr(self.d_rowp_off), self.n_u,
                                       self.sym_total_wg, self.sym_form, _ptr(ws.col), _ptr(ws.rowp),
                                       _ptr(ws.colmask), stream_ptr()), 'iamx_knn2sym_sweep')

    def run_sym_filter(self, ws, thresh):
        """candidate rows from the sweep's bounds, exact top-2 + metric test for those rows,
        survivors compacted in place (pair p: surv_*[surv_off[p] .. + surv_cnt[p]))"""
        L, s, st = lib(), stream_ptr(), self.store
        check(L.iamx_knn2sym_candidates(_ptr(st.sn2), _ptr(st.sperm), _ptr(st.img_off3), _ptr(st.img_n),
                                        _ptr(self.d_pairs), _ptr(self.d_osrc), _ptr(self.d_sym_wg),
                                        _ptr(self.d_col_off), _ptr(self.d_rowp_off), _ptr(self.d_out),
                                        _ptr(ws.col), _ptr(ws.rowp), self.n_pairs, float(thresh),
                                        _ptr(ws.keep), _ptr(ws.seg_count), _ptr(ws.surv_q),
                                        _ptr(ws.task_total), _ptr(ws.tasks), _ptr(ws.d2),
                                        _ptr(ws.colmask), _ptr(ws.nar), ws.max_rows, self.max_query_rows,
                                        self.sym_form, s),
              'iamx_knn2sym_candidates')
        check(L.iamx_knn2sym_exact(_ptr(st.desc), _ptr(st.norm_q), _ptr(st.norm_t), _ptr(st.key_t),
                                   st.rows_used, _ptr(st.img_off),
                                   _ptr(st.img_n), _ptr(self.d_pairs), _ptr(self.d_out),
                                   _ptr(ws.seg_count), _ptr(ws.task_total), _ptr(ws.tasks),
                                   _ptr(ws.surv_q), self.n_pairs, float(thresh), _ptr(ws.d2),
                                   _ptr(ws.surv_t), _ptr(ws.surv_metric), _ptr(ws.cand_keep),
                                   _ptr(ws.surv_cnt), _ptr(ws.zero_div), _ptr(st.desc3), _ptr(st.sn2),
                                   _ptr(st.sct), _ptr(st.sperm), _ptr(st.img_off3), _ptr(self.d_osrc),
                                   _ptr(ws.nar), ws.max_rows, self.sym_form, s), 'iamx_knn2sym_exact')
        # pair p's survivors sit at the start of its own row range
        ws.surv_off[:self.n_pairs + 1].copy_(self.d_out, non_blocking=True)

    def run_knn2(self, ws):
        st = self.store
        check(lib().iamx_knn2_l2_pairs(_ptr(st.desc), _ptr(st.norm_q), _ptr(st.norm_t),
                                       _ptr(st.img_off), _ptr(st.img_n), _ptr(self.d_pairs),
                                       _ptr(self.d_wg), _ptr(self.d_out), self.n_pairs,
                                       self.total_wg, _ptr(ws.idx), _ptr(ws.d2), stream_ptr()),
              'iamx_knn2_l2_pairs')

    def _threshold_compact(self, ws, thresh, index, stride, final):
        """metric threshold -> scan of the per-pair counts -> compaction of the kept rows with their
        train entry index[row * stride].  final: the kept rows ARE the survivors (no finish stage
        follows that writes surv_cnt)."""
        L, s = lib(), stream_ptr()
        check(L.iamx_match_metric(_ptr(ws.d2), _ptr(self.d_out), self.n_pairs, float(thresh),
                                  _ptr(ws.metric), _ptr(ws.keep), _ptr(ws.seg_count),
                                  _ptr(ws.zero_div), s), 'iamx_match_metric')
        check(L.iamx_exclusive_scan_i32(_ptr(ws.seg_count), self.n_pairs, _ptr(ws.surv_off), s),
              'iamx_exclusive_scan_i32')
        check(L.iamx_match_compact(_ptr(index), stride, _ptr(ws.metric), _ptr(ws.keep),
                                   _ptr(self.d_out), _ptr(ws.surv_off), self.n_pairs,
                                   _ptr(ws.surv_q), _ptr(ws.surv_t), _ptr(ws.surv_metric), s),
              'iamx_match_compact')
        if final:
            ws.surv_cnt[:self.n_pairs].copy_(ws.seg_count[:self.n_pairs])

    def run_filter(self, ws, thresh):
        self._threshold_compact(ws, thresh, ws.idx, 2, True)

    # ---- fast form: distances + tile in the sweep, train index only for the survivors
    def _route(self, exact_second):
        """the one decision run_knn2_fast and run_filter_fast share: 'sym' = the symmetric sweep,
        'general' = the kernel that tracks indices (a store without the parity-partitioned copy),
        'exact' / 'bound' = the one-direction forms"""
        if self.sym and not exact_second:
            return 'sym'
        if not self.store.has_train_layout:
            return 'general'
        return 'exact' if exact_second else 'bound'

    def run_knn2_fast(self, ws, exact_second=False):
        route = self._route(exact_second)
        if route == 'sym':
            return self.run_sym_sweep(ws)
        if route == 'general':
            return self.run_knn2(ws)
        if route == 'exact' and self.fast_rows == 1024:      # the exact-second form stops at 512
            self._use_rows(512)
        st = self.store
        check(lib().iamx_knn2v2_pairs(_ptr(st.desc), _ptr(st.norm_q), _ptr(st.img_off),
                                      _ptr(st.img_n), _ptr(st.desc2), _ptr(st.cinit),
                                      _ptr(st.img_off2), _ptr(st.meta), _ptr(self.d_pairs),
                                      _ptr(self.d_wg_fast), _ptr(self.d_out), self.n_pairs,
                                      self.total_wg_fast, self.fast_rows, 1 if route == 'exact' else 0,
                                      _ptr(ws.d2), _ptr(ws.tile), stream_ptr()),
              'iamx_knn2v2_pairs')

    def _use_rows(self, rows):
        nq = np.asarray(self.store.counts, np.int64)[self.pairs[:, 0]]
        wgf = np.zeros(self.n_pairs + 1, np.int64)
        np.cumsum((nq + rows - 1) // rows, out=wgf[1:])
        self.fast_rows, self.total_wg_fast = rows, int(wgf[-1])
        self.d_wg_fast = torch.from_numpy(wgf.astype(np.int32)).to(self.d_pairs.device)

    def run_filter_fast(self, ws, thresh, exact_second=False):
        """threshold + compaction + train rows; every route leaves pair p's survivors at
        surv_*[surv_off[p] .. + surv_cnt[p]).  With the bound form of the sweep the first
        threshold keeps a superset; iamx_knn2v2_finish makes it exact (include/iamx.h)."""
        route = self._route(exact_second)
        if route == 'sym':
            return self.run_sym_filter(ws, thresh)
        if route == 'general':
            return self.run_filter(ws, thresh)
        L, s, st = lib(), stream_ptr(), self.store
        self._threshold_compact(ws, thresh, ws.tile, 1, route == 'exact')
        if route == 'exact':
            check(L.iamx_knn2v2_resolve(_ptr(st.desc), _ptr(st.norm_q), _ptr(st.img_off),
                                        _ptr(st.desc2), _ptr(st.norm2), _ptr(st.perm),
                                        _ptr(st.img_off2), _ptr(self.d_pairs), _ptr(self.d_out),
                                        _ptr(ws.d2), _ptr(ws.surv_off), _ptr(ws.surv_q),
                                        _ptr(ws.surv_t), self.n_pairs, _ptr(ws.unresolved), s),
                  'iamx_knn2v2_resolve')
        else:
            check(L.iamx_knn2v2_finish(_ptr(st.desc), _ptr(st.norm_q), _ptr(st.img_off),
                                       _ptr(st.desc2), _ptr(st.norm2), _ptr(st.perm),
                                       _ptr(st.img_off2), _ptr(self.d_pairs), _ptr(self.d_out),
                                       _ptr(ws.d2), float(thresh), _ptr(ws.surv_off),
                                       _ptr(ws.surv_q), _ptr(ws.surv_t), _ptr(ws.surv_metric),
                                       _ptr(ws.surv_cnt), self.n_pairs, _ptr(ws.zero_div),
                                       _ptr(ws.unresolved), s), 'iamx_knn2v2_finish')

    def run(self, ws, thresh, fast=True):
        """enqueue top-2 + metric threshold + survivor compaction (+ index resolve).
        fast: True = the shipped form (symmetric sweep when the batch holds both directions of
        every pair, else the one-direction bound form), 'exact' = exact-second fast sweep,
        False = the general kernel that tracks indices in the sweep."""
        if self.rows > ws.max_rows or self.n_pairs > ws.max_pairs:
            raise ValueError("workspace too small for this batch")
        if self.n_pairs == 0 or self.rows == 0:
            return
        if fast:
            exact = fast == 'exact'
            self.run_knn2_fast(ws, exact_second=exact)
            self.run_filter_fast(ws, thresh, exact_second=exact)
        else:
            self.run_knn2(ws)
            self.run_filter(ws, thresh)


# --------------------------------------------------------------------------------------
# SIFT
# --------------------------------------------------------------------------------------
_sift_ws = {}
_sift_out = {}
_prep_ws = {}

# Detector slots: the workspace / output / staging caches above are keyed by (device, slot).  Slot 0
# belongs to whoever calls without asking (one thread at a time, as before); worker threads that
# detect concurrently take one of DETECT_SLOTS numbered slots each (image.py runs whole detections
# on its prefetch workers): a slot is ~1 GB of workspace for a 3 MP detect image (8 of them keep the GPU fed), so the number of
# detections in flight is bounded by the slots, not by the number of threads.
DETECT_SLOTS = 8
_slot_tls = threading.local()
_slot_free = None
_slot_lock = threading.Lock()


def _slot_key(dev):
    return (dev.index, getattr(_slot_tls, 'slot', 0))


def wait_stream(polite=None):
    """Wait for the current stream.  The HIP runtime spins on the host while it waits
    (hipDeviceScheduleAuto: one core at 100 % per waiting thread, measured with
    torch.cuda.Event(blocking=True) as well); a thread that holds a detector slot -- or says
    polite=True -- polls an event with short sleeps instead: +0.2 ms of latency, no core burnt.
    (Two dozen prefetch workers waiting for uploads and detections cost more CPU than the JPEG
    Huffman decoding and the cache compression together on a host with a 16-core quota.)"""
    if polite is None:
        polite = getattr(_slot_tls, 'slot', 0) != 0 or getattr(_slot_tls, 'polite', False)
    if not polite:
        torch.cuda.current_stream().synchronize()
        return
    import time
    ev = torch.cuda.Event()
    ev.record()
    pause = 0.0001
    while not ev.query():
        time.sleep(pause)
        pause = min(pause * 1.5, 0.001)


class polite_waits(object):
    """with polite_waits(): waits of this thread inside the package's calls sleep instead of spin"""

    def __enter__(self):
        self.prev = getattr(_slot_tls, 'polite', False)
        _slot_tls.polite = True
        return self

    def __exit__(self, *exc):
        _slot_tls.polite = self.prev
        return False


class detector_slot(object):
    """with detector_slot(): ... -- this thread's sift_detect / equalize_resize calls use a
    private set of device buffers (blocks while all DETECT_SLOTS are taken)"""

    def __enter__(self):
        global _slot_free
        with _slot_lock:
            if _slot_free is None:
                import queue
                _slot_free = queue.Queue()
                for k in range(1, DETECT_SLOTS + 1):
                    _slot_free.put(k)
        self.slot = _slot_free.get()
        self.prev = getattr(_slot_tls, 'slot', 0)
        _slot_tls.slot = self.slot
        return self

    def __exit__(self, *exc):
        _slot_tls.slot = self.prev
        _slot_free.put(self.slot)
        return False


class OverlappedSweeps(object):
    """Runs a sequence of PairBatch launches with the small threshold / compaction / finish
    kernels of launch k on a second stream, beside the sweep of launch k+1 (two workspaces,
    events both ways).  The sweep is ~95 % of a launch and fills the machine; the filter kernels
    are latency bound and fit into its tail -- 6 % more pairs/s at BASELINE configs[1]."""

    def __init__(self, max_rows, max_pairs, first_workspace=None):
        self.ws = [first_workspace or PairWorkspace(max_rows, max_pairs),
                   PairWorkspace(max_rows, max_pairs)]
        self.side = torch.cuda.Stream()
        self.swept = [torch.cuda.Event(), torch.cuda.Event()]
        self.filtered = [torch.cuda.Event(), torch.cuda.Event()]

    def run(self, batches, thresh, after_filter=None, sweep_events=None):
        """after_filter(batch, workspace) is called with the side stream current (enqueue only);
        sweep_events: optional [(start, stop)] timing events, one pair per batch.  On return
        the current stream has waited for everything."""
        main = torch.cuda.current_stream()
        for k, b in enumerate(batches):
            w = self.ws[k & 1]
            if k >= 2:
                main.wait_event(self.filtered[k & 1])        # that workspace is free again
            if sweep_events is not None:
                sweep_events[k][0].record()
            b.run_knn2_fast(w)
            if sweep_events is not None:
                sweep_events[k][1].record()
            self.swept[k & 1].record(main)
            self.side.wait_event(self.swept[k & 1])
            with torch.cuda.stream(self.side):
                b.run_filter_fast(w, thresh)
                if after_filter is not None:
                    after_filter(b, w)
                self.filtered[k & 1].record(self.side)
        main.wait_stream(self.side)


def sift_detect(image, cap=200000, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6,
                order='opencv'):
    """cv2.SIFT_create().detectAndCompute(image, None): image [h,w,3] BGR or [h,w] gray uint8
    (numpy or device tensor).  Returns numpy (kp [N,5] float32: x, y, size, angle, response;
    octave [N] int32 (cv2 packing); desc [N,128] uint8), duplicates removed, in OpenCV's output
    order (KeyPointsFilter::removeDuplicatedSorted) -- or, order='canonical', in the pyramid-local
    (octave, layer, y, x, angle) order."""
    dev = require_gpu()
    img = _dev(image, U8)
    if img.dim() == 2:
        h, w, ch = img.shape[0], img.shape[1], 1
    else:
        h, w, ch = img.shape
    need = int(lib().iamx_sift_workspace_bytes(h, w))
    ws = _sift_ws.get(_slot_key(dev))
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=U8, device=dev)
        _sift_ws[_slot_key(dev)] = ws
    ob = _sift_out.get(_slot_key(dev))                  # (allocations cost ~0.3 ms each per frame)
    if ob is None or ob[0].shape[0] < cap:
        ob = (torch.empty((cap, 8), dtype=torch.float32, device=dev),
              torch.empty((cap, 128), dtype=U8, device=dev), torch.zeros(1, dtype=I32, device=dev))
        _sift_out[_slot_key(dev)] = ob
    kp, desc, n = ob[0][:cap], ob[1][:cap], ob[2]
    check(lib().iamx_sift_detect(_ptr(img), h, w, ch, contrast_threshold, edge_threshold, sigma,
                                 _ptr(ws), need, _ptr(kp), _ptr(desc), cap, _ptr(n), stream_ptr()),
          'iamx_sift_detect')
    # removeDuplicatedSorted on the device (the kernels append in a nondeterministic order, with
    # duplicates): iamx_sift_sort, then one pinned download
    sw = _sift_sort_ws.get(_slot_key(dev))
    need_s = int(lib().iamx_sift_sort_workspace_bytes(cap))
    if sw is None or sw[0].numel() < need_s or sw[1].shape[0] < cap:
        sw = (torch.empty(need_s, dtype=U8, device=dev),
              torch.empty((cap, 8), dtype=torch.float32, device=dev),
              torch.empty((cap, 128), dtype=U8, device=dev),
              torch.zeros(2, dtype=I32, device=dev))
        _sift_sort_ws[_slot_key(dev)] = sw
    if order not in ('opencv', 'canonical'):
        raise ValueError("sift_detect: order must be 'opencv' or 'canonical'")
    check(lib().iamx_sift_sort(_ptr(kp), _ptr(desc), _ptr(n), cap, 1 if order == 'opencv' else 0,
                               w, h, _ptr(sw[0]), need_s, _ptr(sw[1]), _ptr(sw[2]), _ptr(sw[3]),
                               stream_ptr()), 'iamx_sift_sort')
    sw[3][1:2].copy_(n, non_blocking=True)                # [kept, appended]
    hn = _sift_pinned_count(dev)
    hn.copy_(sw[3], non_blocking=True)
    wait_stream()
    cnt, found = int(hn[0]), int(hn[1])
    if found > cap:
        raise _lib.IamxError("sift_detect: %d keypoints exceed the capacity %d" % (found, cap))
    sift_detect.last_removed = found - cnt               # duplicates dropped (diagnosis / tests)
    hk, hd = _sift_pinned(dev, cnt)
    hk[:cnt].copy_(sw[1][:cnt], non_blocking=True)
    hd[:cnt].copy_(sw[2][:cnt], non_blocking=True)
    wait_stream()
    k = hk[:cnt].numpy()
    return k[:, :5].copy(), k[:, 5].copy().view(np.int32), hd[:cnt].numpy().copy()


_sift_sort_ws = {}
_sift_pin = {}


def _sift_pinned_count(dev):
    cur = _sift_pin.get((_slot_key(dev), 'n'))
    if cur is None:
        cur = _sift_pin[(_slot_key(dev), 'n')] = torch.zeros(2, dtype=I32).pin_memory()
    return cur


def _sift_pinned(dev, n):
    """page-locked staging for the keypoint / descriptor download (grown geometrically)"""
    cur = _sift_pin.get(_slot_key(dev))
    if cur is None or cur[0].shape[0] < n:
        m = max(1 << 16, 1 << int(n - 1).bit_length())
        cur = (torch.empty((m, 8), dtype=torch.float32).pin_memory(),
               torch.empty((m, 128), dtype=U8).pin_memory())
        _sift_pin[_slot_key(dev)] = cur
    return cur


# ---- split JPEG decoder (csrc/jpeg.hip): Huffman decode on the host, the rest on the device --------
class JpegCoefficients(object):
    """A JPEG after the host half of the decoder: info (int32 [16], iamx_jpeg_info), the
    quantised coefficients in a page-locked buffer (int16 [blocks, 64]) and the quantisation
    tables (uint16 [3, 64]).  release() hands the buffer back to the pool.  After
    jpeg_device_decode the coefficients are a device tensor and there is no buffer to hand back."""
    __slots__ = ('info', 'coef', 'quant', '_slot')

    def release(self):
        if self._slot is not None:
            with _jpeg_lock:
                _jpeg_pool.append(self._slot)
            self._slot = None
            self.coef = None


_jpeg_pool = []          # free page-locked coefficient buffers (torch int16, flat)
_jpeg_lock = __import__('threading').Lock()


def _jpeg_buffer(n_values):
    with _jpeg_lock:
        for k, b in enumerate(_jpeg_pool):
            if b.numel() >= n_values:
                return _jpeg_pool.pop(k)
        if len(_jpeg_pool) >= 8:             # (a survey's frames are all the same size)
            _jpeg_pool.pop(0)
    return torch.empty(int(n_values), dtype=torch.int16).pin_memory()


def jpeg_host_decode(source):
    """The host half: file name or bytes -> JpegCoefficients, or None for a file the split
    decoder does not handle (progressive, arithmetic, CMYK, ... -- the caller reads those the
    host way).  No device involved; the C call releases the GIL (worker threads decode in
    parallel).  Raises IamxError for a broken file."""
    import ctypes
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source)
    else:
        with open(source, 'rb') as fp:
            data = fp.read()
    raw = np.frombuffer(data, np.uint8)
    L = lib()
    jc = JpegCoefficients()
    jc.info = np.zeros(16, np.int32)
    jc._slot = None
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = L.iamx_jpeg_info(p(raw), len(raw), p(jc.info))
    if rc == -4:
        return None
    check(rc, 'iamx_jpeg_info')
    blocks = int(jc.info[11])
    jc._slot = _jpeg_buffer(blocks * 64)
    jc.coef = jc._slot[:blocks * 64].view(blocks, 64)
    jc.quant = np.zeros((3, 64), np.uint16)
    rc = L.iamx_jpeg_decode_coefficients(p(raw), len(raw), ctypes.c_void_p(jc.coef.data_ptr()), blocks,
                                         p(jc.quant))
    if rc != 0:
        jc.release()
        if rc == -4:
            return None
        check(rc, 'iamx_jpeg_decode_coefficients')
    return jc


def jpeg_reconstruct(jc, release=True):
    """The device half: JpegCoefficients -> BGR uint8 [h, w, 3] in HBM, bit-identical to
    libjpeg-turbo's output (dequantisation, islow IDCT, fancy upsampling, YCbCr -> BGR)."""
    import ctypes
    dev = require_gpu()
    L = lib()
    info = jc.info
    w, h = int(info[0]), int(info[1])
    # (the 384-byte table first: a pageable copy waits for what is in front of it on the stream)
    d_quant = torch.from_numpy(jc.quant.astype(np.int16)).to(dev)        # (bit pattern; read as uint16)
    if jc.coef.is_cuda:                                  # jpeg_device_decode: already in HBM
        d_coef = jc.coef
    else:
        d_coef = torch.empty(jc.coef.shape, dtype=torch.int16, device=dev)
        d_coef.copy_(jc.coef, non_blocking=True)
    need = int(L.iamx_jpeg_workspace_bytes(info.ctypes.data_as(ctypes.c_void_p)))
    ws = torch.empty(need, dtype=U8, device=dev)
    out = torch.empty((h, w, 3), dtype=U8, device=dev)
    check(L.iamx_jpeg_reconstruct(_ptr(d_coef), _ptr(d_quant), info.ctypes.data_as(ctypes.c_void_p),
                                  _ptr(ws), need, _ptr(out), stream_ptr()), 'iamx_jpeg_reconstruct')
    if release:
        wait_stream()                                    # the page-locked buffer has been read
        jc.release()
    return out


# what became of the files given to jpeg_device_decode: decoded on the device / not a file of the
# split decoder's kind / refused because the sub-sequences did not synchronise inside the pass
# bound / damaged (data ended early, marker out of place) -- the last three return None
jpeg_device_stats = {'device': 0, 'unsupported': 0, 'refused': 0, 'damaged': 0, 'passes': 0}
_jpeg_status = []                # page-locked landing places of the status words and the free ones' numbers


def jpeg_device_decode(source):
    """The host half's work done on the device (csrc/jpeg_entropy.hip): file name or bytes ->
    JpegCoefficients whose coefficients are already in HBM (no page-locked slot; jpeg_reconstruct
    takes it as it takes the host half's), or None for "go the host way": a file the split decoder
    does not handle, one whose sub-sequences did not synchronise (flat images), a damaged one
    (data that ends before the last block, a stray marker in the scan).
    jpeg_device_stats says which.  Only the file's bytes cross PCIe.  Runs on the current stream
    and waits for it once, to read the status word.  Raises IamxError for a broken file."""
    import ctypes
    dev = require_gpu()
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source)
    else:
        with open(source, 'rb') as fp:
            data = fp.read()
    L = lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = len(data)
    raw = np.zeros((n + 15) // 16 * 16, np.uint8)        # (the kernels load whole 16-byte pieces)
    raw[:n] = np.frombuffer(data, np.uint8)
    jc = JpegCoefficients()
    jc.info = np.zeros(16, np.int32)
    jc.quant = np.zeros((3, 64), np.uint16)
    jc._slot = None
    header = np.zeros(int(L.iamx_jpeg_entropy_header_bytes()), np.uint8)
    rc = L.iamx_jpeg_entropy_prepare(p(raw), n, p(jc.info), p(jc.quant), p(header), len(header))
    if rc == -4:
        with _jpeg_lock:
            jpeg_device_stats['unsupported'] += 1
        return None
    check(rc, 'iamx_jpeg_entropy_prepare')
    blocks = int(jc.info[11])
    need = int(L.iamx_jpeg_entropy_workspace_bytes(p(header)))
    d_header = torch.from_numpy(header).to(dev)
    d_raw = torch.from_numpy(raw).to(dev)
    ws = torch.empty(need, dtype=U8, device=dev)
    coef = torch.empty((blocks, 64), dtype=torch.int16, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    check(L.iamx_jpeg_entropy_decode(_ptr(d_raw), raw.size, p(header), _ptr(d_header), _ptr(ws), need,
                                     _ptr(coef), blocks, _ptr(status), stream_ptr()),
          'iamx_jpeg_entropy_decode')
    with _jpeg_lock:
        if not _jpeg_status:                             # one page-locked allocation for every thread
            _jpeg_status.append(torch.zeros((64, 4), dtype=torch.int32).pin_memory())
            _jpeg_status.append(list(range(64)))
        slot = _jpeg_status[1].pop() if _jpeg_status[1] else None
    host = _jpeg_status[0][slot] if slot is not None else torch.zeros(4, dtype=torch.int32).pin_memory()
    try:
        host.copy_(status, non_blocking=True)
        wait_stream()                                    # (this stream only; politely on a worker)
        st, passes = int(host[0]), int(host[1])
    finally:
        if slot is not None:
            with _jpeg_lock:
                _jpeg_status[1].append(slot)
    key = {1: 'device', 2: 'refused', 3: 'damaged'}.get(st)
    if key is None:
        raise _lib.IamxError('iamx_jpeg_entropy_decode left status %d' % st)
    with _jpeg_lock:
        jpeg_device_stats[key] += 1
        jpeg_device_stats['passes'] = max(jpeg_device_stats['passes'], passes)
    if st != 1:
        return None
    jc.coef = coef
    return jc


def jpeg_decode(source, entropy='host'):
    """file name or bytes -> BGR uint8 [h, w, 3] on the device, or None for an unsupported file.
    entropy='device': the Huffman decode runs on the device too (jpeg_device_decode), with the host
    half as the fallback for the files it refuses."""
    if entropy not in ('host', 'device'):
        raise ValueError("entropy must be 'host' or 'device'")
    jc = jpeg_device_decode(source) if entropy == 'device' else None
    if jc is None:
        jc = jpeg_host_decode(source)
    return None if jc is None else jpeg_reconstruct(jc)


def equalize_resize(bgr, scale, equalize=True, clip_limit=3.0):
    """Image.load_rgb(equalize=True) + cv2.resize(fx=fy=scale) on the device.
    bgr [h,w,3] uint8 (numpy or device) -> device tensor [round(h*s), round(w*s), 3] uint8."""
    dev = require_gpu()
    img = _dev(bgr, U8)
    h, w, ch = img.shape
    if ch != 3:
        raise ValueError("expected a BGR image")
    import ctypes
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().iamx_image_resized_dims(h, w, float(scale), ctypes.byref(oh), ctypes.byref(ow)),
          'iamx_image_resized_dims')
    need = int(lib().iamx_image_prep_workspace_bytes(h, w))
    ws = _prep_ws.get(_slot_key(dev))
    if ws is None or ws.numel() < need:
        ws = _prep_ws[_slot_key(dev)] = torch.empty(need, dtype=U8, device=dev)
    out = torch.empty((oh.value, ow.value, 3), dtype=U8, device=dev)
    check(lib().iamx_image_equalize_resize(_ptr(img), h, w, 1 if equalize else 0, float(clip_limit),
                                           float(scale), _ptr(ws), need, _ptr(out), stream_ptr()),
          'iamx_image_equalize_resize')
    if not isinstance(bgr, torch.Tensor):
        torch.cuda.current_stream().synchronize()      # (the upload's staging copy has been read)
    return out


def image_prep_stages(h, w):
    """What the last equalize_resize(equalize=True) of an [h, w, 3] image left in the current slot's
    workspace (tests / diagnosis): views 'hsv' and 'equalised' uint8 [h,w,3], 'hist' int32 [64,256]
    and 'lut' uint8 [64,256], laid out as iamx_image_prep_stage says."""
    dev = require_gpu()
    ws = _prep_ws.get(_slot_key(dev))
    if ws is None or ws.numel() < int(lib().iamx_image_prep_workspace_bytes(h, w)):
        raise _lib.IamxError("no equalize_resize of a %dx%d image has run in this slot" % (h, w))
    import ctypes
    views = {}
    for stage, (name, dtype, shape) in enumerate((('hsv', U8, (h, w, 3)), ('equalised', U8, (h, w, 3)),
                                                  ('hist', I32, (64, 256)), ('lut', U8, (64, 256)))):
        off, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib().iamx_image_prep_stage(h, w, stage, ctypes.byref(off), ctypes.byref(nbytes)),
              'iamx_image_prep_stage')
        views[name] = ws[off.value:off.value + nbytes.value].view(dtype).view(shape)
    return views


def resize_area_shape(h, w, fx, fy):
    """(rows, columns) of resize_area's result for an h x w image (host arithmetic, no device)"""
    import ctypes
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().iamx_image_area_dims(int(h), int(w), float(fx), float(fy), ctypes.byref(oh), ctypes.byref(ow)),
          'iamx_image_area_dims')
    return max(oh.value, 0), max(ow.value, 0)


def resize_area(img, fx, fy):
    """cv2.resize(img, (0, 0), fx=fx, fy=fy, interpolation=cv2.INTER_AREA) on the device
    (csrc/image_area.hip; downscale only).  img uint8 [h,w,3] or [h,w] (numpy or device) ->
    device tensor [round(h*fy), round(w*fx)(, 3)] uint8."""
    dev = require_gpu()
    src = _dev(img, U8)
    if src.dim() == 2:
        h, w, ch = src.shape[0], src.shape[1], 1
    elif src.dim() == 3 and src.shape[2] in (1, 3):
        h, w, ch = src.shape
    else:
        raise ValueError("expected a uint8 [h,w,3] or [h,w] image")
    # (argument errors -- an upscale, an empty result -- are reported by the call before it launches)
    shape = resize_area_shape(h, w, fx, fy) + ((ch,) if src.dim() == 3 else ())
    out = torch.empty(shape, dtype=U8, device=dev)
    check(lib().iamx_image_resize_area(_ptr(src), h, w, ch, float(fx), float(fy), _ptr(out), stream_ptr()),
          'iamx_image_resize_area')
    if not isinstance(img, torch.Tensor):
        torch.cuda.current_stream().synchronize()      # (the upload's staging copy has been read)
    return out


# --------------------------------------------------------------------------------------
# Step 5 surface grids (csrc/surface_grid.hip)
# --------------------------------------------------------------------------------------
SURFACE_SKY, SURFACE_HIGH_ANGLE, SURFACE_FALLBACK = 1, 2, 4
SURFACE_RECORD_BYTES = 128
SURFACE_MAX_SEED_GRID = 4096


def surface_seed_grid(tri, G):
    """The G x G table of start triangles over the points' bounding box (host): find_simplex of the
    cell centres; a centre outside the hull takes vertex_to_simplex of the nearest point.
    -> (seed int32 [G, G] (row = y), bbox float64 [xmin, ymin, xmax, ymax])"""
    from scipy.spatial import cKDTree
    G = int(G)
    if not 1 <= G <= SURFACE_MAX_SEED_GRID:
        raise ValueError("seed grid of %d cells a side" % G)
    pts = np.asarray(tri.points, np.float64)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    cx = lo[0] + (np.arange(G) + 0.5) * ((hi[0] - lo[0]) / G)
    cy = lo[1] + (np.arange(G) + 0.5) * ((hi[1] - lo[1]) / G)
    centres = np.stack(np.meshgrid(cx, cy), axis=-1).reshape(-1, 2)
    seed = np.asarray(tri.find_simplex(centres), np.int32)
    out = np.nonzero(seed < 0)[0]
    if len(out):
        _d, near = cKDTree(pts).query(centres[out])
        seed[out] = np.asarray(tri.vertex_to_simplex, np.int32)[near]
    return seed.reshape(G, G), np.array([lo[0], lo[1], hi[0], hi[1]], np.float64)


class Surface(object):
    """A scipy.spatial.Delaunay triangulation and its vertex values on the device: 128-byte records
    (iamx_surface_pack), the values, the seed grid.  upload_s is the host's time in the uploads."""

    def __init__(self, tri, values, seed_g=None):
        import time
        dev = require_gpu()
        simplices = np.ascontiguousarray(tri.simplices, np.int32)
        self.T, self.P = int(simplices.shape[0]), int(np.asarray(tri.points).shape[0])
        values = np.ascontiguousarray(values, np.float64).reshape(-1)
        if simplices.shape[1] != 3 or values.shape[0] != self.P:
            raise ValueError("expected a 2-d triangulation and one value per point")
        if seed_g is None:
            seed_g = min(1024, max(1, int(np.ceil(np.sqrt(self.T / 4.0)))))
        seed, bbox = surface_seed_grid(tri, seed_g)
        self.G, self.bbox = int(seed_g), bbox
        t0 = time.perf_counter()
        simp = _dev(simplices, I32)
        nbr = _dev(np.ascontiguousarray(tri.neighbors, np.int32), I32)
        trans = _dev(np.ascontiguousarray(tri.transform, np.float64), F64)
        self.values = _dev(values, F64)
        self.seed = _dev(seed, I32)
        self.records = torch.empty(self.T * SURFACE_RECORD_BYTES, dtype=U8, device=dev)
        check(lib().iamx_surface_pack(_ptr(simp), _ptr(nbr), _ptr(trans), self.T, _ptr(self.records),
                                      stream_ptr()), 'iamx_surface_pack')
        torch.cuda.current_stream().synchronize()         # (the scipy-shaped arrays are dropped here)
        self.upload_s = time.perf_counter() - t0

    def _bbox_ptr(self):
        return self.bbox.ctypes.data_as(_lib.c_void_p)


def surface_interp(surface, xy, max_steps=0, with_steps=False):
    """LinearNDInterpolator(tri, values)(xy) by a walk per query (csrc/surface_grid.hip).
    xy [N, 2] (numpy or device) -> z float64 [N] (NaN outside the hull), flags uint8 [N] (1: the
    query was NOT answered -- step bound, degenerate simplex, NaN query -- and scipy has to be asked)
    and, with_steps, the records each walk read (int32 [N]).  Device tensors."""
    dev = require_gpu()
    q = _dev(xy, F64).reshape(-1, 2)
    n = int(q.shape[0])
    out = torch.empty(n, dtype=F64, device=dev)
    flags = torch.empty(n, dtype=U8, device=dev)
    steps = torch.empty(n, dtype=I32, device=dev) if with_steps else None
    check(lib().iamx_surface_interp(_ptr(surface.records), surface.T, _ptr(surface.values), surface.P,
                                    _ptr(surface.seed), surface.G, surface._bbox_ptr(), _ptr(q), n,
                                    int(max_steps), _ptr(out), _ptr(flags), _ptr(steps), stream_ptr()),
          'iamx_surface_interp')
    if not isinstance(xy, torch.Tensor):
        torch.cuda.current_stream().synchronize()          # (the upload's staging copy has been read)
    return (out, flags, steps) if with_steps else (out, flags)


def surface_grid(surface, M, ned, avg_ground, uv, no_extrapolate=False, ground_m=None, max_steps=0,
                 with_steps=False):
    """projectVectors + intersect2d of render_panda3d.build_map for a batch of images, one thread per
    (image, grid vertex).  M [I, 3, 3] = body2ned . cam2body . IK, ned [I, 3], avg_ground [I] = -z_avg,
    uv [n, 2] the shared pixel grid; surface a Surface, or None with ground_m (the ground-plane mode,
    intersectVectorsWithGroundPlane).  -> pts float64 [I, n, 3] NED, rounds int32 [I, n], flags uint8
    [I, n] (SURFACE_SKY | SURFACE_HIGH_ANGLE | SURFACE_FALLBACK) and, with_steps, records read per ray."""
    dev = require_gpu()
    ground = ground_m is not None
    if surface is None and not ground:
        raise ValueError("a Surface, or ground_m for the ground-plane mode")
    Md = _dev(M, F64).reshape(-1, 9)
    nd = _dev(ned, F64).reshape(-1, 3)
    I = int(Md.shape[0])
    ag = _dev(avg_ground if avg_ground is not None else np.zeros(I), F64).reshape(-1)
    uvd = _dev(uv, F64).reshape(-1, 2)
    n = int(uvd.shape[0])
    if nd.shape[0] != I or ag.shape[0] != I:
        raise ValueError("M, ned and avg_ground must have one entry per image")
    pts = torch.empty((I, n, 3), dtype=F64, device=dev)
    rounds = torch.empty((I, n), dtype=I32, device=dev)
    flags = torch.empty((I, n), dtype=U8, device=dev)
    steps = torch.empty((I, n), dtype=I32, device=dev) if with_steps else None
    s = None if ground else surface
    check(lib().iamx_surface_grid(_ptr(s.records) if s else None, s.T if s else 0,
                                  _ptr(s.values) if s else None, s.P if s else 0,
                                  _ptr(s.seed) if s else None, s.G if s else 0,
                                  s._bbox_ptr() if s else None, _ptr(Md), _ptr(nd), _ptr(ag), I, _ptr(uvd), n,
                                  1 if no_extrapolate else 0, 1 if ground else 0,
                                  float(ground_m) if ground else 0.0, int(max_steps), _ptr(pts),
                                  _ptr(rounds), _ptr(flags), _ptr(steps), stream_ptr()),
          'iamx_surface_grid')
    torch.cuda.current_stream().synchronize()              # (the uploads' staging copies have been read)
    return (pts, rounds, flags, steps) if with_steps else (pts, rounds, flags)


# --------------------------------------------------------------------------------------
# terrain under the survey (csrc/terrain.hip)
# --------------------------------------------------------------------------------------
TERRAIN_SKY, TERRAIN_CAPPED, TERRAIN_LEFT_GRID = 1, 2, 4
TERRAIN_MAX_AXIS = 32768
TERRAIN_FILL = -32768.0


class Terrain(object):
    """The axes and the grid of a RegularGridInterpolator((axis_n, axis_e), grid) on the device."""

    def __init__(self, axis_n, axis_e, grid):
        axis_n = np.ascontiguousarray(axis_n, np.float64).reshape(-1)
        axis_e = np.ascontiguousarray(axis_e, np.float64).reshape(-1)
        grid = np.ascontiguousarray(grid, np.float64)
        self.rows, self.cols = int(axis_n.shape[0]), int(axis_e.shape[0])
        if grid.shape != (self.rows, self.cols):
            raise ValueError("a grid of %r over axes of %d and %d nodes" % (grid.shape, self.rows, self.cols))
        for a in (axis_n, axis_e):
            if not 2 <= a.shape[0] <= TERRAIN_MAX_AXIS or not np.all(np.diff(a) > 0):
                raise ValueError("a terrain axis is strictly ascending with 2 to %d nodes" % TERRAIN_MAX_AXIS)
        self.axis_n, self.axis_e, self.grid = _dev(axis_n, F64), _dev(axis_e, F64), _dev(grid, F64)
        torch.cuda.current_stream().synchronize()          # (the uploads' staging copies have been read)

    def _args(self):
        return _ptr(self.axis_n), self.rows, _ptr(self.axis_e), self.cols, _ptr(self.grid)


def terrain_heights(terrain, points):
    """RegularGridInterpolator(..., bounds_error=False, fill_value=-32768)(points) on the device:
    points [N, 2] (n, e), numpy or device -> z float64 [N] device (NaN for a NaN coordinate,
    TERRAIN_FILL outside the axes)."""
    dev = require_gpu()
    q = _dev(points, F64).reshape(-1, 2)
    n = int(q.shape[0])
    z = torch.empty(n, dtype=F64, device=dev)
    check(lib().iamx_terrain_heights(*terrain._args(), _ptr(q), n, _ptr(z), stream_ptr()), 'iamx_terrain_heights')
    if not isinstance(points, torch.Tensor):
        torch.cuda.current_stream().synchronize()          # (the upload's staging copy has been read)
    return z


def terrain_rays(terrain, M, ned, uv=None, v=None):
    """lib/srtm.py's interpolate_vector for a batch of images, one thread per ray.  ned [I, 3] and
    either M [I, 3, 3] with the shared pixel grid uv [n, 2] (rays = unit(M . [u, v, 1]), the arguments
    of surface_grid) or ready vectors v [I, n, 3] with M None.  -> pts float64 [I, n, 3] NED, iters
    uint8 [I, n], flags uint8 [I, n] (TERRAIN_SKY | TERRAIN_CAPPED | TERRAIN_LEFT_GRID)."""
    dev = require_gpu()
    if (M is None) == (v is None) or (M is None) != (uv is None):
        raise ValueError("M with uv, or v")
    nd = _dev(ned, F64).reshape(-1, 3)
    I = int(nd.shape[0])
    if v is None:
        Md = _dev(M, F64).reshape(-1, 9)
        uvd = _dev(uv, F64).reshape(-1, 2)
        n = int(uvd.shape[0])
        if Md.shape[0] != I:
            raise ValueError("M and ned must have one entry per image")
    else:
        vd = _dev(v, F64).reshape(I, -1, 3) if I else _dev(v, F64).reshape(0, 1, 3)
        n = int(vd.shape[1])
    if n < 1:
        raise ValueError("no rays")
    pts = torch.empty((I, n, 3), dtype=F64, device=dev)
    iters = torch.empty((I, n), dtype=U8, device=dev)
    flags = torch.empty((I, n), dtype=U8, device=dev)
    if v is None:
        check(lib().iamx_terrain_rays(*terrain._args(), _ptr(Md), _ptr(nd), I, _ptr(uvd), n, _ptr(pts),
                                      _ptr(iters), _ptr(flags), stream_ptr()), 'iamx_terrain_rays')
    else:
        check(lib().iamx_terrain_rays_vec(*terrain._args(), _ptr(vd), _ptr(nd), I, n, _ptr(pts),
                                          _ptr(iters), _ptr(flags), stream_ptr()), 'iamx_terrain_rays_vec')
    torch.cuda.current_stream().synchronize()              # (the uploads' staging copies have been read)
    return pts, iters, flags


# --------------------------------------------------------------------------------------
# the explorer's colour tables (csrc/image_colour.hip)
# --------------------------------------------------------------------------------------
def _frame3(img):
    """numpy / tensor -> contiguous device uint8 [h, w, 3]"""
    t = _dev(img, U8)
    if t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0:
        raise ValueError("expected a uint8 [h,w,3] image")
    return t


def colour_histogram(img, hist=None):
    """The three channel histograms of a uint8 [h,w,3] image (numpy or device): int32 device tensor
    [3, 256] holding unsigned 32-bit counts.  With `hist` the counts are ADDED onto it (zero it once)."""
    dev = require_gpu()
    src = _frame3(img)
    if hist is None:
        hist = torch.zeros((3, 256), dtype=I32, device=dev)
    elif hist.dtype != I32 or tuple(hist.shape) != (3, 256) or not hist.is_cuda or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous int32 device tensor [3, 256]")
    check(lib().iamx_colour_histogram(_ptr(src), src.shape[0] * src.shape[1], _ptr(hist), stream_ptr()),
          'iamx_colour_histogram')
    if not isinstance(img, torch.Tensor):
        torch.cuda.current_stream().synchronize()      # (the upload's staging copy has been read)
    return hist


def colour_accumulate(total, frames):
    """total (int32 device tensor of the frames' shape, unsigned 32-bit sums) += every frame of
    `frames` (device uint8 tensors of one shape), 8 frames per launch: the sum is read and written
    once per launch."""
    import ctypes
    require_gpu()
    frames = list(frames)
    for f in frames:
        if not (isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == U8 and f.is_contiguous()
                and f.shape == total.shape):
            raise ValueError("frames must be contiguous uint8 device tensors of the sum's shape")
    if total.dtype != I32 or not total.is_cuda or not total.is_contiguous():
        raise ValueError("the sum must be a contiguous int32 device tensor")
    L = lib()
    per = int(L.iamx_colour_accumulate_max_frames())
    for k in range(0, len(frames), per):
        part = frames[k:k + per]
        ptrs = (ctypes.c_void_p * len(part))(*[f.data_ptr() for f in part])
        check(L.iamx_colour_accumulate(ptrs, len(part), total.numel(), _ptr(total), stream_ptr()),
              'iamx_colour_accumulate')
    return total


def colour_mean(total, count):
    """uint8(trunc(float32(total) / float32(count))): the reference's (sum / count).astype('uint8');
    count above 65 793 is refused (255 * count < 2^24: the reference's float32 sum is exact)"""
    dev = require_gpu()
    count = int(count)
    if total.dtype != I32 or not total.is_cuda or not total.is_contiguous():
        raise ValueError("the sum must be a contiguous int32 device tensor")
    out = torch.empty(total.shape, dtype=U8, device=dev)
    check(lib().iamx_colour_mean(_ptr(total), total.numel(), count, _ptr(out), stream_ptr()), 'iamx_colour_mean')
    return out


def colour_moments(img, cu, cv):
    """The sums of the radial fit v ~ a' s^4 + b' s^2 + c about (cu, cv), s = r / R: (out, R) with
    out a float64 device tensor [3, 8] = per channel sum s^8, s^6, s^4, s^2, n, s^4 v, s^2 v, v and
    R the image's largest (float32-rounded) radius.  Reproducible bit for bit."""
    import ctypes
    dev = require_gpu()
    src = _frame3(img)
    L = lib()
    ws = torch.empty(int(L.iamx_colour_moments_workspace_doubles()), dtype=F64, device=dev)
    out = torch.empty((3, 8), dtype=F64, device=dev)
    R = ctypes.c_double(0.0)
    check(L.iamx_colour_moments(_ptr(src), src.shape[0], src.shape[1], float(cu), float(cv), ctypes.byref(R),
                                _ptr(ws), _ptr(out), stream_ptr()), 'iamx_colour_moments')
    torch.cuda.current_stream().synchronize()          # (the workspace, and an upload's staging copy)
    return out, R.value


def colour_fit_mask(height, width, cu, cv, coef, seed=0):
    """dither(a r^4 + b r^2 + c) per channel, coef [3][3] = (a, b, c) per channel -> device uint8
    [height, width, 3].  Raises IamxError when a polynomial leaves [0, 255] inside the image."""
    dev = require_gpu()
    coef = np.ascontiguousarray(coef, np.float64).reshape(9)
    out = torch.empty((int(height), int(width), 3), dtype=U8, device=dev)
    check(lib().iamx_colour_fit_mask(int(height), int(width), float(cu), float(cv),
                                     coef.ctypes.data_as(_lib.c_void_p), int(seed) & (2 ** 64 - 1), _ptr(out),
                                     stream_ptr()), 'iamx_colour_fit_mask')
    return out


def colour_mask_finish(img):
    """per channel m = 255 - v, m -= min(m) -> device uint8 [h, w, 3]"""
    dev = require_gpu()
    src = _frame3(img)
    scratch = torch.empty(3, dtype=I32, device=dev)
    out = torch.empty(src.shape, dtype=U8, device=dev)
    check(lib().iamx_colour_mask_finish(_ptr(src), src.shape[0] * src.shape[1], _ptr(scratch), _ptr(out),
                                        stream_ptr()), 'iamx_colour_mask_finish')
    torch.cuda.current_stream().synchronize()          # (the scratch words, and an upload's staging copy)
    return out


def colour_lut(img, lut, mask=None):
    """out[y][x][c] = lut[c][img[y][x][c]], plus mask (uint8, img's shape) with saturation at 255.
    A numpy image is uploaded and a numpy array comes back; a device tensor gives a device tensor
    (like resize_area's input)."""
    dev = require_gpu()
    src = _frame3(img)
    table = _dev(np.asarray(lut) if not isinstance(lut, torch.Tensor) else lut, U8)
    if tuple(table.shape) != (3, 256):
        raise ValueError("lut must be uint8 [3, 256]")
    m = None
    if mask is not None:
        m = _frame3(mask)
        if m.shape != src.shape:
            raise ValueError("the mask must have the image's shape")
    out = torch.empty(src.shape, dtype=U8, device=dev)
    check(lib().iamx_colour_lut(_ptr(src), src.shape[0] * src.shape[1], _ptr(table), _ptr(m), _ptr(out),
                                stream_ptr()), 'iamx_colour_lut')
    if isinstance(img, torch.Tensor):
        if not (isinstance(lut, torch.Tensor) and (mask is None or isinstance(mask, torch.Tensor))):
            torch.cuda.current_stream().synchronize()  # (the uploads' staging copies have been read)
        return out
    return out.cpu().numpy()


# --------------------------------------------------------------------------------------
# surface-consistency and depth culls of chains (csrc/chain_surface.hip)
# --------------------------------------------------------------------------------------
SURFACE_MAX_K = 32                                                 # IAMX_SURFACE_MAX_K
SURFACE_FITTED, SURFACE_SKIPPED_SMALL, SURFACE_SKIPPED_FLAT = 1, 2, 3
SURFACE_N_SMALL, SURFACE_N_FLAT, SURFACE_N_UNCOUNTED, SURFACE_N_LOOKED = range(4)
CHAIN_STATS_TILE = 256                                             # IAMX_CHAIN_STATS_TILE
STATS_AVERAGE, STATS_STDDEV, STATS_N, STATS_BAND = range(4)


def surface_knn_fit(img_ptr, uv, ned, chain, k=30, n_pos=10):
    """The observation table (device tensors: img_ptr i64 [n_images + 1], uv f64 [n_obs, 2], ned f64
    [n_obs, 3], chain i32 [n_obs]) -> device (tgt i32 [n_obs, k], val f64 [n_obs, k], used i32,
    fit f64 [n_obs, 2], status i32).  Enqueued on the current stream, no synchronisation."""
    dev = require_gpu()
    n_obs, n_images = chain.numel(), img_ptr.numel() - 1
    m = max(n_obs, 1)
    tgt = torch.empty((m, k), dtype=I32, device=dev)
    val = torch.empty((m, k), dtype=F64, device=dev)
    used = torch.empty(m, dtype=I32, device=dev)
    fit = torch.empty((m, 2), dtype=F64, device=dev)
    status = torch.empty(m, dtype=I32, device=dev)
    check(lib().iamx_surface_knn_fit(_ptr(img_ptr), _ptr(uv), _ptr(ned), _ptr(chain), n_images, n_obs,
                                     int(k), int(n_pos), _ptr(tgt), _ptr(val), _ptr(used), _ptr(fit),
                                     _ptr(status), stream_ptr()), 'iamx_surface_knn_fit')
    return tgt[:n_obs], val[:n_obs], used[:n_obs], fit[:n_obs], status[:n_obs]


def surface_chain_metric(tgt, val, status, looked, n_chains):
    """-> device (sum f64 [n_chains], count i32, metric f64, counters i64 [4]: SURFACE_N_*)."""
    dev = require_gpu()
    n_obs, k = tgt.shape
    m = max(n_chains, 1)
    total = torch.empty(m, dtype=F64, device=dev)
    count = torch.empty(m, dtype=I32, device=dev)
    metric = torch.empty(m, dtype=F64, device=dev)
    counters = torch.zeros(4, dtype=I64, device=dev)
    off = torch.empty(m + 1, dtype=I64, device=dev)
    order = torch.empty(max(n_obs * k, 1), dtype=I32, device=dev)
    check(lib().iamx_surface_chain_metric(_ptr(tgt), _ptr(val), _ptr(status), n_obs, k, _ptr(looked),
                                          n_chains, _ptr(total), _ptr(count), _ptr(metric), _ptr(counters),
                                          _ptr(off), _ptr(order), stream_ptr()), 'iamx_surface_chain_metric')
    return total[:n_chains], count[:n_chains], metric[:n_chains], counters


def chain_outlier_stats(metric, looked, factor, two_sided):
    """-> device (stats f64 [4]: STATS_*, flag u8 [n], idx i32 [n], metric of idx f64 [n], n_flagged
    i64 [1]); the first n_flagged entries of idx are the flagged chains in ascending order."""
    dev = require_gpu()
    n = metric.numel()
    m = max(n, 1)
    tiles = (m + CHAIN_STATS_TILE - 1) // CHAIN_STATS_TILE
    stats = torch.zeros(4, dtype=F64, device=dev)
    flag = torch.zeros(m, dtype=U8, device=dev)
    idx = torch.empty(m, dtype=I32, device=dev)
    sel = torch.empty(m, dtype=F64, device=dev)
    n_flagged = torch.zeros(1, dtype=I64, device=dev)
    part = torch.empty(tiles, dtype=F64, device=dev)
    cnt = torch.empty(tiles, dtype=I32, device=dev)
    off = torch.empty(tiles + 1, dtype=I64, device=dev)
    check(lib().iamx_chain_outlier_stats(_ptr(metric), _ptr(looked), n, float(factor), int(bool(two_sided)),
                                         _ptr(stats), _ptr(flag), _ptr(idx), _ptr(sel), _ptr(n_flagged),
                                         _ptr(part), _ptr(cnt), _ptr(off), stream_ptr()),
          'iamx_chain_outlier_stats')
    return stats, flag[:n], idx[:n], sel[:n], n_flagged


def chain_depths(img_ptr, ned, pos, chain_ptr, chain_obs):
    """-> device (depth f64 [n_obs], z f64 [n_images, 3] = mean, deviation, count, metric f64
    [n_chains], looked u8 [n_chains])."""
    dev = require_gpu()
    n_obs, n_images, n_chains = ned.shape[0], img_ptr.numel() - 1, chain_ptr.numel() - 1
    depth = torch.empty(max(n_obs, 1), dtype=F64, device=dev)
    z = torch.zeros((max(n_images, 1), 3), dtype=F64, device=dev)
    metric = torch.zeros(max(n_chains, 1), dtype=F64, device=dev)
    looked = torch.zeros(max(n_chains, 1), dtype=U8, device=dev)
    check(lib().iamx_chain_depths(_ptr(img_ptr), _ptr(ned), n_images, n_obs, _ptr(pos), _ptr(chain_ptr),
                                  _ptr(chain_obs), n_chains, _ptr(depth), _ptr(z), _ptr(metric),
                                  _ptr(looked), stream_ptr()), 'iamx_chain_depths')
    return depth[:n_obs], z[:n_images], metric[:n_chains], looked[:n_chains]


# --------------------------------------------------------------------------------------
# dense surface (csrc/dense_sweep.hip; the rules: dense.py)
# --------------------------------------------------------------------------------------
DENSE_TILE = (32, 16)                    # a workgroup's reference pixels, (width, height)
DENSE_MAX_RADIUS, DENSE_MAX_PLANES, DENSE_MAX_NEIGHBOURS, DENSE_MAX_SIDE = 7, 4096, 16, 16384
DENSE_SGM_MAX_PLANES = 64                # semi-global mode: one plane per lane of a wave
DENSE_GUIDED_MAX_PLANES = 65536          # the guided sweep's whole plane set (a tile walks a window of it)
DENSE_SGM_DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))   # (dx, dy)


def dense_camera(view):
    """the 21 doubles of a view: R (row-major), C, fx, fy, cx, cy, k1, k2, p1, p2, k3"""
    R = np.asarray(view.R, np.float64).reshape(9)
    C = np.asarray(view.C, np.float64).reshape(3)
    K = np.asarray(view.K, np.float64).reshape(4)
    d = np.asarray(view.dist, np.float64).reshape(5)
    return np.concatenate([R, C, K, d])


def _dense_size(views):
    shapes = [tuple(v.G.shape) for v in views]
    if any(len(s) != 2 or s[0] < 1 or s[1] < 1 for s in shapes):
        raise ValueError("a view's grey plane is [h, w]")
    if any(s != shapes[0] for s in shapes):
        raise ValueError("the views of a call have one size, got %s" % sorted(set(shapes)))
    h, w = shapes[0]
    if h > DENSE_MAX_SIDE or w > DENSE_MAX_SIDE:
        raise ValueError("a view side above %d pixels" % DENSE_MAX_SIDE)
    return h, w


def _dense_out(out, specs, dev):
    """the outputs: fresh, or the caller's (checked: shape, dtype, device, contiguous)"""
    if out is None:
        return [torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in specs]
    out = list(out)
    if len(out) != len(specs):
        raise ValueError("%d output tensors wanted" % len(specs))
    for t, (shape, dtype) in zip(out, specs):
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
            raise ValueError("an output tensor is a contiguous device %s of shape %r" % (dtype, tuple(shape)))
    return out


def _dense_sweep_check(ref, neighbours, w_far, w_near, radius):
    """the arguments that every form of the sweep shares, on the host -> (h, w, w_far, w_near, radius)"""
    radius = int(radius)
    if not 1 <= radius <= DENSE_MAX_RADIUS:
        raise ValueError("radius is 1 to %d, got %d" % (DENSE_MAX_RADIUS, radius))
    if not 1 <= len(neighbours) <= DENSE_MAX_NEIGHBOURS:
        raise ValueError("1 to %d neighbours, got %d" % (DENSE_MAX_NEIGHBOURS, len(neighbours)))
    h, w = _dense_size([ref] + neighbours)
    w_far, w_near = float(w_far), float(w_near)
    if not (w_far > 0.0 and w_near > w_far and math.isfinite(w_near)):
        raise ValueError("inverse depths with 0 < w_far < w_near wanted, got %r and %r" % (w_far, w_near))
    if ref.rays is None or tuple(ref.rays.shape) != (h, w, 2):
        raise ValueError("the reference view carries rays [h, w, 2]")
    return h, w, w_far, w_near, radius


def _dense_sweep_upload(ref, neighbours, h, w):
    """-> the reference's grey plane and rays, the neighbours' planes [n, h, w], its pose, their cameras"""
    G = _dev(ref.G, torch.float32)
    rays = _dev(ref.rays, F64)
    planes_n = [_dev(v.G, torch.float32) for v in neighbours]
    if all(p.data_ptr() == planes_n[0].data_ptr() + 4 * h * w * k for k, p in enumerate(planes_n)):
        N = planes_n[0]                                    # (consecutive in one buffer already: read in place)
    else:
        N = torch.stack(planes_n).contiguous()
    pose = _dev(dense_camera(ref)[:12], F64)
    cams = _dev(np.stack([dense_camera(v) for v in neighbours]), F64)
    return G, rays, N, pose, cams


def dense_sweep(ref, neighbours, w_far, w_near, planes, radius=3, min_var=4.0, min_score=0.6, out=None, volume=None):
    """The plane sweep of one reference view (dense.py, THE RULES), one launch.  ref and the
    neighbours are views (G [h, w] float32, K, dist, R, C; the reference also rays [h, w, 2]), numpy
    or device.  -> device plane int32 [h, w], score float32 [h, w], depth float32 [h, w] (NaN where
    not kept), around float32 [h, w, 3].  out: those four, allocated by the caller.  volume: a
    contiguous device uint8 [h, w, planes] that receives the costs of SEMI-GLOBAL RULES beside them
    (2 to 64 planes then)."""
    neighbours = list(neighbours)
    planes = int(planes)
    if not 1 <= planes <= DENSE_MAX_PLANES:
        raise ValueError("planes is 1 to %d, got %d" % (DENSE_MAX_PLANES, planes))
    if volume is not None:
        _dense_sgm_planes(planes)
    h, w, w_far, w_near, radius = _dense_sweep_check(ref, neighbours, w_far, w_near, radius)
    dev = require_gpu()
    G, rays, N, pose, cams = _dense_sweep_upload(ref, neighbours, h, w)
    plane, score, depth, around = _dense_out(out, [((h, w), I32), ((h, w), torch.float32), ((h, w), torch.float32),
                                                   ((h, w, 3), torch.float32)], dev)
    args = (_ptr(G), _ptr(rays), _ptr(N), _ptr(pose), _ptr(cams), w, h, len(neighbours), planes, w_far, w_near, radius,
            float(min_var), float(min_score), _ptr(plane), _ptr(score), _ptr(depth), _ptr(around))
    if volume is None:
        check(lib().iamx_dense_sweep(*(args + (stream_ptr(),))), 'iamx_dense_sweep')
    else:
        volume, = _dense_out([volume], [((h, w, planes), U8)], dev)
        check(lib().iamx_dense_sweep_volume(*(args + (_ptr(volume), stream_ptr()))), 'iamx_dense_sweep_volume')
    torch.cuda.current_stream().synchronize()              # (the uploads' staging copies have been read)
    return plane, score, depth, around


def _dense_total(total):
    total = int(total)
    if not 2 <= total <= DENSE_GUIDED_MAX_PLANES:
        raise ValueError("the fine plane set has 2 to %d planes, got %d" % (DENSE_GUIDED_MAX_PLANES, total))
    return total


def dense_tiles(h, w):
    """(tiles_y, tiles_x) of the sweep's tiles over an h x w image"""
    return (int(h) + DENSE_TILE[1] - 1) // DENSE_TILE[1], (int(w) + DENSE_TILE[0] - 1) // DENSE_TILE[0]


def dense_windows_check(windows, h, w, total):
    """A window table of an h x w image (dense.py, REFINEMENT RULES): int32 [tiles_y, tiles_x, 2] =
    (first, count), numpy or a tensor, every entry inside the `total` planes; anything else is a
    ValueError.  A device table is read back for it.  -> the table as it came"""
    shape = dense_tiles(h, w) + (2,)
    if isinstance(windows, torch.Tensor):
        if windows.dtype != I32 or tuple(windows.shape) != shape:
            raise ValueError("the window table is int32 of shape %r" % (shape,))
        tab = windows.cpu().numpy()
    else:
        tab = np.asarray(windows)
        if tab.dtype != np.int32 or tab.shape != shape:
            raise ValueError("the window table is int32 of shape %r" % (shape,))
    first, count = tab[..., 0].astype(np.int64), tab[..., 1].astype(np.int64)
    if (first < 0).any() or (count < 0).any() or (first + count > total).any():
        raise ValueError("a window has 0 <= first, 0 <= count and first + count <= %d" % total)
    return windows


def dense_guide(coarse_depth, fine_hw, w_far, w_near, total, radius=3, pad=0, out=None):
    """The window table of a fine level from a coarse depth map (dense.py, REFINEMENT RULES: Guide), one
    launch.  coarse_depth float32 [hc, wc], NaN where there is none, numpy or device; fine_hw = (h, w) of
    the fine views; total the size of the fine plane set.  -> device int32 [tiles_y, tiles_x, 2] =
    (first, count).  out: that tensor, allocated by the caller."""
    total, radius, pad = _dense_total(total), int(radius), int(pad)
    h, w = int(fine_hw[0]), int(fine_hw[1])
    shape = tuple(coarse_depth.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("a coarse depth map is [hc, wc]")
    if not (1 <= h <= DENSE_MAX_SIDE and 1 <= w <= DENSE_MAX_SIDE and max(shape) <= DENSE_MAX_SIDE):
        raise ValueError("a side of 1 to %d pixels wanted" % DENSE_MAX_SIDE)
    if not 1 <= radius <= DENSE_MAX_RADIUS:
        raise ValueError("radius is 1 to %d, got %d" % (DENSE_MAX_RADIUS, radius))
    if not 0 <= pad <= DENSE_GUIDED_MAX_PLANES:
        raise ValueError("pad is 0 to %d planes, got %d" % (DENSE_GUIDED_MAX_PLANES, pad))
    w_far, w_near = float(w_far), float(w_near)
    if not (w_far > 0.0 and w_near > w_far and math.isfinite(w_near)):
        raise ValueError("inverse depths with 0 < w_far < w_near wanted, got %r and %r" % (w_far, w_near))
    dev = require_gpu()
    D = _dev(coarse_depth, torch.float32)
    windows, = _dense_out(None if out is None else [out], [(dense_tiles(h, w) + (2,), I32)], dev)
    check(lib().iamx_dense_guide(_ptr(D), shape[1], shape[0], w, h, w_far, w_near, total, radius, pad, _ptr(windows),
                                 stream_ptr()), 'iamx_dense_guide')
    torch.cuda.current_stream().synchronize()
    return windows


def dense_sweep_guided(ref, neighbours, w_far, w_near, total, windows, radius=3, min_var=4.0, min_score=0.6, out=None):
    """The plane sweep of one reference view over per-tile windows of `total` planes (dense.py,
    REFINEMENT RULES: Guided sweep), one launch.  The views as in dense_sweep; windows int32
    [tiles_y, tiles_x, 2] = (first, count), numpy or device.  -> device plane int32 [h, w] (the index in
    the whole set), score, depth float32 [h, w], around float32 [h, w, 3].  out: those four."""
    neighbours = list(neighbours)
    total = _dense_total(total)
    h, w, w_far, w_near, radius = _dense_sweep_check(ref, neighbours, w_far, w_near, radius)
    dense_windows_check(windows, h, w, total)
    dev = require_gpu()
    G, rays, N, pose, cams = _dense_sweep_upload(ref, neighbours, h, w)
    tab = _dev(windows, I32)
    plane, score, depth, around = _dense_out(out, [((h, w), I32), ((h, w), torch.float32), ((h, w), torch.float32),
                                                   ((h, w, 3), torch.float32)], dev)
    check(lib().iamx_dense_sweep_guided(_ptr(G), _ptr(rays), _ptr(N), _ptr(pose), _ptr(cams), w, h, len(neighbours), total,
                                        w_far, w_near, radius, float(min_var), float(min_score), _ptr(tab), _ptr(plane),
                                        _ptr(score), _ptr(depth), _ptr(around), stream_ptr()), 'iamx_dense_sweep_guided')
    torch.cuda.current_stream().synchronize()              # (the uploads' staging copies have been read)
    return plane, score, depth, around


def _dense_sgm_planes(planes):
    if not 2 <= planes <= DENSE_SGM_MAX_PLANES:
        raise ValueError("semi-global mode takes 2 to %d planes, got %d" % (DENSE_SGM_MAX_PLANES, planes))


def dense_sgm_check(planes, paths, p1, p2, c_invalid):
    """the parameters of SEMI-GLOBAL RULES, checked on the host -> them as ints"""
    planes, paths, p1, p2, c_invalid = int(planes), int(paths), int(p1), int(p2), int(c_invalid)
    _dense_sgm_planes(planes)
    if paths not in (4, 8):
        raise ValueError("paths is 4 or 8, got %d" % paths)
    if not 0 <= p1 <= p2 <= 255:
        raise ValueError("0 <= P1 <= P2 <= 255 wanted, got %d and %d" % (p1, p2))
    if not 0 <= c_invalid <= 254:
        raise ValueError("c_invalid is 0 to 254, got %d" % c_invalid)
    return planes, paths, p1, p2, c_invalid


def _dense_volume(volume):
    """a cost volume (numpy or device) -> device uint8 [h, w, planes], its sizes"""
    if len(volume.shape) != 3 or min(volume.shape) < 1:
        raise ValueError("a cost volume is [h, w, planes]")
    h, w, planes = (int(x) for x in volume.shape)
    _dense_sgm_planes(planes)
    if h > DENSE_MAX_SIDE or w > DENSE_MAX_SIDE:
        raise ValueError("a view side above %d pixels" % DENSE_MAX_SIDE)
    return h, w, planes


def dense_sgm_paths(volume, paths=8, p1=16, p2=128, c_invalid=127, out=None, direction=None):
    """The path costs of SEMI-GLOBAL RULES summed over the first `paths` directions, one launch per
    direction: volume uint8 [h, w, planes] (numpy or device).  -> device total [h, w, planes], the uint16 sums as
    torch.int16 (they are at most 4072).
    out: (total,), allocated by the caller; whatever it holds is overwritten.  direction = 0 .. 7: that
    direction's L_r alone, one launch."""
    h, w, planes = _dense_volume(volume)
    planes, paths, p1, p2, c_invalid = dense_sgm_check(planes, paths, p1, p2, c_invalid)
    if direction is not None and not 0 <= int(direction) < 8:
        raise ValueError("direction is 0 to 7")
    dev = require_gpu()
    vol = _dev(volume, U8)
    total, = _dense_out(out, [((h, w, planes), I16)], dev)
    if direction is None:
        check(lib().iamx_dense_sgm_paths(_ptr(vol), w, h, planes, paths, p1, p2, c_invalid, _ptr(total), stream_ptr()),
              'iamx_dense_sgm_paths')
    else:
        check(lib().iamx_dense_sgm_direction(_ptr(vol), w, h, planes, int(direction), 0, p1, p2, c_invalid, _ptr(total),
                                             stream_ptr()), 'iamx_dense_sgm_direction')
    torch.cuda.current_stream().synchronize()
    return total


def dense_sgm_select(total, volume, w_far, w_near, max_cost, out=None):
    """The select of SEMI-GLOBAL RULES: total (int16 bits of the uint16 sums) and volume uint8 [h, w, planes] (numpy or device),
    the planes uniform in inverse depth from w_far to w_near, max_cost = q(min_score).  -> device plane
    int32, cost uint8, total at the winner int16, depth float32 (NaN where not kept), all [h, w].
    out: those four."""
    h, w, planes = _dense_volume(volume)
    if tuple(total.shape) != (h, w, planes):
        raise ValueError("total has the volume's shape %r" % ((h, w, planes),))
    w_far, w_near, max_cost = float(w_far), float(w_near), int(max_cost)
    if not (w_far > 0.0 and w_near > w_far and math.isfinite(w_near)):
        raise ValueError("inverse depths with 0 < w_far < w_near wanted, got %r and %r" % (w_far, w_near))
    if not 0 <= max_cost <= 254:
        raise ValueError("max_cost is 0 to 254, got %d" % max_cost)
    dev = require_gpu()
    vol = _dev(volume, U8)
    tot = _dev(total, I16)
    plane, cost, tot0, depth = _dense_out(out, [((h, w), I32), ((h, w), U8), ((h, w), I16),
                                                ((h, w), torch.float32)], dev)
    step = (w_near - w_far) / (planes - 1)
    check(lib().iamx_dense_sgm_select(_ptr(tot), _ptr(vol), w, h, planes, w_far, step, max_cost, _ptr(plane), _ptr(cost),
                                      _ptr(tot0), _ptr(depth), stream_ptr()), 'iamx_dense_sgm_select')
    torch.cuda.current_stream().synchronize()
    return plane, cost, tot0, depth


def dense_neighbour_table(neighbours, n_views):
    """lists of view numbers -> int32 [V, M], -1 padded (host)"""
    if len(neighbours) != n_views:
        raise ValueError("one neighbour list per view")
    M = max([len(n) for n in neighbours] + [1])
    if M > DENSE_MAX_NEIGHBOURS:
        raise ValueError("at most %d neighbours per view" % DENSE_MAX_NEIGHBOURS)
    tab = -np.ones((n_views, M), np.int32)
    for i, n in enumerate(neighbours):
        n = [int(j) for j in n]
        if any(not 0 <= j < n_views or j == i for j in n):
            raise ValueError("view %d: a neighbour is another view of the call" % i)
        tab[i, :len(n)] = n
    return tab


def dense_check(depths, views, neighbours, eps=0.01, min_agree=2, out=None):
    """The consistency rule over stacked depth maps: depths float32 [V, h, w] (NaN: not kept), the V
    views (each with rays), neighbours a list of view numbers per view.  -> device keep uint8
    [V, h, w], ned float64 [V, h, w, 3]."""
    views = list(views)
    V = len(views)
    tab = dense_neighbour_table(neighbours, V)
    if not (float(eps) >= 0.0 and int(min_agree) >= 1):
        raise ValueError("eps >= 0 and min_agree >= 1 wanted")
    if V == 0:
        raise ValueError("no views")
    h, w = _dense_size(views)
    if tuple(depths.shape) != (V, h, w):
        raise ValueError("depths is [V, h, w] = %r" % ((V, h, w),))
    for v in views:
        if v.rays is None or tuple(v.rays.shape) != (h, w, 2):
            raise ValueError("every view carries rays [h, w, 2]")
    dev = require_gpu()
    D = _dev(depths, torch.float32)
    rays = torch.stack([_dev(v.rays, F64) for v in views]).contiguous()
    cams = _dev(np.stack([dense_camera(v) for v in views]), F64)
    nb = _dev(tab, I32)
    keep, ned = _dense_out(out, [((V, h, w), U8), ((V, h, w, 3), F64)], dev)
    check(lib().iamx_dense_check(_ptr(D), _ptr(rays), _ptr(cams), _ptr(nb), V, int(tab.shape[1]), w, h, float(eps),
                                 int(min_agree), _ptr(keep), _ptr(ned), stream_ptr()), 'iamx_dense_check')
    torch.cuda.current_stream().synchronize()
    return keep, ned


def dense_splat(ned, keep, x0, y1, gsd, W, H, out=None):
    """The fusion rule: NED points [..., 3] (numpy or device) with keep [...] (or None: all) into the
    raster frame.  -> device count int32 [H, W], sum int64 [H, W] of rint(up 1024), dsm float32
    [H, W].  out: those three; count and sum are zeroed here."""
    W, H, gsd = int(W), int(H), float(gsd)
    if not (W >= 1 and H >= 1 and gsd > 0.0 and math.isfinite(gsd) and math.isfinite(x0) and math.isfinite(y1)):
        raise ValueError("a raster frame of at least one cell at a positive gsd wanted")
    dev = require_gpu()
    P = _dev(ned, F64).reshape(-1, 3)
    n = int(P.shape[0])
    Kp = None
    if keep is not None:
        Kp = _dev(keep, U8).reshape(-1)
        if int(Kp.shape[0]) != n:
            raise ValueError("one keep flag per point")
    count, total, dsm = _dense_out(out, [((H, W), I32), ((H, W), I64), ((H, W), torch.float32)], dev)
    count.zero_()
    total.zero_()
    check(lib().iamx_dense_splat(_ptr(P), _ptr(Kp), n, float(x0), float(y1), gsd, W, H, _ptr(count), _ptr(total),
                                 stream_ptr()), 'iamx_dense_splat')
    check(lib().iamx_dense_resolve(_ptr(count), _ptr(total), W, H, _ptr(dsm), stream_ptr()), 'iamx_dense_resolve')
    torch.cuda.current_stream().synchronize()
    return count, total, dsm


DENSE_FUSE_MIN_BINS, DENSE_FUSE_MAX_BINS, DENSE_FUSE_MAX_LEVELS = 4, 64, 4
DENSE_FUSE_MAX_WIDTH = 1 << 40           # of wmin, the least bin width in units of q = rint(up 1024)


def dense_fuse_check(bins=32, levels=2, band=None, share=256, gsd=None):
    """the parameters of ROBUST FUSION RULES (dense.py), checked on the host -> (bins, levels, wmin, share)
    with wmin = max(1, rint(band 1024)); band None: 0.5 gsd"""
    if any(isinstance(v, float) and not float(v).is_integer() for v in (bins, levels, share)):
        raise ValueError("bins, levels and share are integers, got %r, %r and %r" % (bins, levels, share))
    bins, levels, share = int(bins), int(levels), int(share)
    if not DENSE_FUSE_MIN_BINS <= bins <= DENSE_FUSE_MAX_BINS:
        raise ValueError("bins is %d to %d, got %d" % (DENSE_FUSE_MIN_BINS, DENSE_FUSE_MAX_BINS, bins))
    if not 1 <= levels <= DENSE_FUSE_MAX_LEVELS:
        raise ValueError("levels is 1 to %d, got %d" % (DENSE_FUSE_MAX_LEVELS, levels))
    if not 1 <= share <= 256:
        raise ValueError("share is 1 to 256 (256ths of the strongest bin), got %d" % share)
    if band is None:
        if gsd is None:
            raise ValueError("band defaults to half the gsd: one of them is wanted")
        band = 0.5 * float(gsd)
    band = float(band)
    if not (band > 0.0 and math.isfinite(band)):
        raise ValueError("band is a positive number of metres, got %r" % band)
    wmin = max(1, int(np.rint(band * 1024.0)))
    if wmin > DENSE_FUSE_MAX_WIDTH:
        raise ValueError("band %g m is %d units of 1/1024 m, above 2^40" % (band, wmin))
    return bins, levels, wmin, share


def dense_fuse_bytes(W, H, bins):
    """what dense_fuse holds per call: 4 bins (hist) + 16 (window) + 4 (count) + 4 (support) + 8 (sum) + 4 (dsm)
    bytes per cell"""
    return int(W) * int(H) * (4 * int(bins) + 16 + 4 + 4 + 8 + 4)


def dense_fuse(ned, keep, x0, y1, gsd, W, H, bins=32, levels=2, band=None, share=256, out=None):
    """The robust fusion rule (dense.py, ROBUST FUSION RULES): NED points [..., 3] (numpy or device) with keep
    [...] (or None: all) into the raster frame; band None: 0.5 gsd.  2 + levels passes over the points, `levels`
    over the cells and the resolve, stream ordered.  -> device count int32 [H, W], support int32 [H, W], sum
    int64 [H, W] of the supporting rint(up 1024), window int64 [H, W, 2] = the final (lo, hi), dsm float32
    [H, W].  out: those five; they are initialised here.  The call holds 4 bins + 40 bytes per cell
    (dense_fuse_bytes), the histograms among them; more than the device has free is a ValueError before a launch."""
    W, H, gsd = int(W), int(H), float(gsd)
    if not (W >= 1 and H >= 1 and gsd > 0.0 and math.isfinite(gsd) and math.isfinite(x0) and math.isfinite(y1)):
        raise ValueError("a raster frame of at least one cell at a positive gsd wanted")
    bins, levels, wmin, share = dense_fuse_check(bins, levels, band, share, gsd)
    dev = require_gpu()
    need = dense_fuse_bytes(W, H, bins) if out is None else W * H * 4 * bins
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if need > free:                                        # (free on the device, or free in torch's own pool)
        raise ValueError("a %d x %d cell raster with %d bins takes %d bytes (4 bins + 40 per cell), %d are free"
                         % (W, H, bins, need, free))
    P = _dev(ned, F64).reshape(-1, 3)
    n = int(P.shape[0])
    Kp = None
    if keep is not None:
        Kp = _dev(keep, U8).reshape(-1)
        if int(Kp.shape[0]) != n:
            raise ValueError("one keep flag per point")
    count, support, total, window, dsm = _dense_out(out, [((H, W), I32), ((H, W), I32), ((H, W), I64), ((H, W, 2), I64),
                                                          ((H, W), torch.float32)], dev)
    hist = torch.zeros((H, W, bins), dtype=I32, device=dev)          # (the bits of uint32 counters)
    count.zero_()
    support.zero_()
    total.zero_()
    window[..., 0] = torch.iinfo(I64).max
    window[..., 1] = torch.iinfo(I64).min
    L, s = lib(), stream_ptr()
    frame = (_ptr(P), _ptr(Kp), n, float(x0), float(y1), gsd, W, H)
    check(L.iamx_dense_fuse_range(*(frame + (_ptr(count), _ptr(window), s))), 'iamx_dense_fuse_range')
    for level in range(levels):
        check(L.iamx_dense_fuse_hist(*(frame + (_ptr(window), bins, wmin, _ptr(hist), s))), 'iamx_dense_fuse_hist')
        check(L.iamx_dense_fuse_select(_ptr(count), W, H, bins, wmin, share if level == 0 else 256, _ptr(hist), _ptr(window),
                                       s), 'iamx_dense_fuse_select')
    check(L.iamx_dense_fuse_sum(*(frame + (_ptr(window), _ptr(support), _ptr(total), s))), 'iamx_dense_fuse_sum')
    check(L.iamx_dense_resolve(_ptr(support), _ptr(total), W, H, _ptr(dsm), s), 'iamx_dense_resolve')
    torch.cuda.current_stream().synchronize()
    return count, support, total, window, dsm


def dense_fill(dsm, rounds=8):
    """The DSM hole fill (dense.py, THE RULES: fill), one launch per round and one to sort the cells:
    dsm float32 [H, W] (numpy or device), NaN: empty.  -> device (filled float32 [H, W], round_of uint8
    [H, W]: 0 measured, k filled in round k, 255 still empty)."""
    rounds = int(rounds)
    if not 0 <= rounds <= 254:
        raise ValueError("rounds is 0 to 254, got %d" % rounds)
    if len(dsm.shape) != 2 or dsm.shape[0] < 1 or dsm.shape[1] < 1:
        raise ValueError("a DSM is [H, W]")
    dev = require_gpu()
    src = _dev(dsm, torch.float32)
    H, W = int(src.shape[0]), int(src.shape[1])
    z = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(2)]
    r = [torch.empty((H, W), dtype=U8, device=dev) for _ in range(2)]
    check(lib().iamx_dense_fill(_ptr(src), None, W, H, 0, _ptr(z[0]), _ptr(r[0]), stream_ptr()), 'iamx_dense_fill')
    for k in range(1, rounds + 1):
        a, b = (k - 1) & 1, k & 1
        check(lib().iamx_dense_fill(_ptr(z[a]), _ptr(r[a]), W, H, k, _ptr(z[b]), _ptr(r[b]), stream_ptr()),
              'iamx_dense_fill')
    torch.cuda.current_stream().synchronize()              # (src may be a staging copy: it has been read)
    return z[rounds & 1], r[rounds & 1]


# --------------------------------------------------------------------------------------
# true orthophoto (csrc/ortho_dsm.hip; the rules: ortho.py)
# --------------------------------------------------------------------------------------
ORTHO_DSM_PARAMS, ORTHO_DSM_MAX_UPSAMPLE = 26, 8


def ortho_dsm_params(x0, y1, gsd, bias, zmax, K, dist, R, C):
    """the 26 host doubles of iamx_ortho_dsm_image: the DSM's frame, bias, zmax, then a dense camera
    (R row-major, C, fx, fy, cx, cy at the frame's size, k1, k2, p1, p2, k3)"""
    return np.concatenate([[float(x0), float(y1), float(gsd), float(bias), float(zmax)],
                           np.asarray(R, np.float64).reshape(9), np.asarray(C, np.float64).reshape(3),
                           np.asarray(K, np.float64).reshape(4), np.asarray(dist, np.float64).reshape(5)])


def ortho_dsm_image(mode, dsm, ss, params, frame, image_index, box, acc, index, count, bgr):
    """One image of a true orthophoto into the accumulators (ortho.py, THE TRUE-ORTHO RULES), one
    launch: mode 0 best / 1 feather, dsm device float32 [H, W], ss the upsample, params
    ortho_dsm_params(), frame device uint8 [h, w, 3], box (c0, r0, c1, r1) in mosaic pixels; acc,
    index (None in mode feather), count, bgr as iamx_ortho_clear left them or earlier images did."""
    params = np.ascontiguousarray(params, np.float64)
    if params.shape != (ORTHO_DSM_PARAMS,):
        raise ValueError("%d parameters wanted" % ORTHO_DSM_PARAMS)
    c0, r0, c1, r1 = (int(v) for v in box)
    check(lib().iamx_ortho_dsm_image(int(mode), _ptr(dsm), int(dsm.shape[0]), int(dsm.shape[1]), int(ss),
                                     params.ctypes.data_as(_lib.c_void_p), _ptr(frame), int(frame.shape[0]),
                                     int(frame.shape[1]), int(image_index), c0, r0, c1, r1, _ptr(acc), _ptr(index),
                                     _ptr(count), _ptr(bgr), stream_ptr()), 'iamx_ortho_dsm_image')


def _ortho_dsm_args(params, box):
    params = np.ascontiguousarray(params, np.float64)
    if params.shape != (ORTHO_DSM_PARAMS,):
        raise ValueError("%d parameters wanted" % ORTHO_DSM_PARAMS)
    return params, tuple(int(v) for v in box)


def ortho_dsm_owner(dsm, ss, params, frame_hw, image_index, box, metric, index, count):
    """The owner pass of one image (ortho.py, THE TRUE-ORTHO RULES, mode multiband): mode best's count,
    metric and index from the geometry alone; frame_hw = (h, w) of the frame that will follow, the
    rest as ortho_dsm_image."""
    params, (c0, r0, c1, r1) = _ortho_dsm_args(params, box)
    check(lib().iamx_ortho_dsm_owner(_ptr(dsm), int(dsm.shape[0]), int(dsm.shape[1]), int(ss),
                                     params.ctypes.data_as(_lib.c_void_p), int(frame_hw[0]), int(frame_hw[1]),
                                     int(image_index), c0, r0, c1, r1, _ptr(metric), _ptr(index), _ptr(count),
                                     stream_ptr()), 'iamx_ortho_dsm_owner')


def ortho_dsm_layer(dsm, ss, params, frame, image_index, box, index, layer):
    """The layer of one image over its work box: layer device float32 [box pixels][4] = (C_b, C_g,
    C_r, A), iamx_ortho_mb_layer's layout; every pixel of the box is written."""
    params, (c0, r0, c1, r1) = _ortho_dsm_args(params, box)
    check(lib().iamx_ortho_dsm_layer(_ptr(dsm), int(dsm.shape[0]), int(dsm.shape[1]), int(ss),
                                     params.ctypes.data_as(_lib.c_void_p), _ptr(frame), int(frame.shape[0]),
                                     int(frame.shape[1]), int(image_index), c0, r0, c1, r1, _ptr(index), _ptr(layer),
                                     stream_ptr()), 'iamx_ortho_dsm_layer')
