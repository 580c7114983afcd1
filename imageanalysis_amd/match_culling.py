"""MI355X-native counterpart of the reference's scripts/lib/match_culling.py, plus the device-backed
report that scripts/4b-mre-by-image.py builds from it.

Same names and semantics as the reference:

    mark_feature(matches, match_index, feat_index, error)      match_culling.py:133-137
    mark_using_list(mark_list, matches)                        :139-141
    delete_marked_features(matches, min_chain_len, strong=False)   :144-161
    show_outliers(result_list, matches, image_list) / draw_match(...)   (interactive, cv2)

New, for the 4b-mre-by-image.py twin (imageanalysis_amd/scripts/4b-mre-by-image.py):

    mre_by_image(opt, matches, x=None, proj=None) -> MreReport
        per-observation e = |observed - projected|, per-camera mean / max, the summary scalars of
        the signed residual vector: one pass of iamx_ba_reproj_stats over the camera-major
        observations Optimizer.setup() uploaded; only C rows and a few scalars reach the host
    mark_outliers(matches, report, trim_stddev, max_error=None) -> mark count
        the reference's mark_outliers(): iamx_ba_mark_outliers thresholds on the device, the
        flagged observations (ascending) come back, are ordered by descending e on the host (ties
        in observation order: the reference's stable sort) and marked

New, for the 4b-colocated-feats.py twin (imageanalysis_amd/scripts/4b-colocated-feats.py):

    colocated_features(proj, matches, group_list, group_index, min_angle) -> mark list
        [chain, member] once per member pair of the group that sees the chain's position under less
        than min_angle degrees, in the reference's order: one pass of iamx_chain_pair_angles, the
        per-member counts come back and are unrolled on the host

New, for the 4c-surface-outliers.py and 4c-by-depth.py twins (the rules: include/iamx.h):

    surface_consistency(proj, matches, group_list, group_index, k=30, positives=10, alive=None)
        -> SurfaceReport: per chain the mean misfit of its members against the line of 3-D over
        pixel distance that each of their image neighbours fits (iamx_surface_knn_fit,
        iamx_surface_chain_metric); the arrays stay on the device
    surface_outliers(report, stddev=5) -> (chains by descending |metric|, average, deviation)
    cull_surface(proj, matches, group_list, group_index, stddev=5, max_rounds=None) -> rounds
        the reference's `while result > 0` loop on an alive mask; every member of a culled chain
        is marked at the end
    depth_outliers(proj, matches, group_list, group_index, stddev=3) -> (mark list, image rows)
    weak_images(matches, n_images, min_features=25) -> mark list (host)

`matches` is the reference's list of `[ned, group, [image, [u, v]], ...]` chains, or the
array-backed match_cleanup.Chains: marks on an untouched Chains are kept in a member mask
(`chains.marked`) and delete_marked_features() rebuilds its arrays with numpy.
"""
import numpy as np

from .match_cleanup import Chains

MARK = [-1, -1]


# ---------------------------------------------------------------------------------------------
# marking
# ---------------------------------------------------------------------------------------------
def _marks(chains):
    m = getattr(chains, 'marked', None)
    if m is None or len(m) != len(chains.img):
        m = np.zeros(len(chains.img), bool)
        chains.marked = m
    return m


def _arrays(matches):
    return isinstance(matches, Chains) and matches.untouched()


def mark_feature(matches, match_index, feat_index, error, quiet=False):
    if not quiet:
        print('  outlier - match index:', match_index, 'feature index:', feat_index, 'error:', error)
    if _arrays(matches):
        lo, hi = int(matches.ptr[match_index]), int(matches.ptr[match_index + 1])
        if not 0 <= feat_index < hi - lo:
            raise IndexError('feature index %d out of range of match %d' % (feat_index, match_index))
        _marks(matches)[lo + feat_index] = True
        return
    match = matches[match_index]
    match[feat_index + 2] = [-1, -1]


def mark_using_list(mark_list, matches):
    for mark in mark_list:
        mark_feature(matches, mark[0], mark[1], "-")


# ---------------------------------------------------------------------------------------------
# deletion
# ---------------------------------------------------------------------------------------------
def delete_marked_features(matches, min_chain_len, strong=False):
    """Remove the marked members; a chain that had a marked member goes entirely with `strong`,
    otherwise when fewer than min_chain_len members are left.  Chains without marks stay, however
    short.  The reference's messages in the reference's order (last chain first)."""
    print(" deleting marked items...")
    if _arrays(matches):
        _delete_arrays(matches, min_chain_len, strong)
    else:
        keep = np.ones(len(matches), bool)
        for i in reversed(range(len(matches))):
            match = matches[i]
            members = [p for p in match[2:] if p != MARK]
            if len(members) == len(match) - 2:
                continue
            match[2:] = members
            if strong:
                print("deleting entire match that contains a bad element", i)
                keep[i] = False
            elif len(members) < min_chain_len:
                print("deleting match that is now in less than %d images:" % min_chain_len, match)
                keep[i] = False
        if not keep.all():
            # one pass instead of a list.pop(i) per chain (quadratic when many chains go)
            matches[:] = [m for m, k in zip(matches, keep.tolist()) if k]
    print("final matches size:", len(matches))


def _delete_arrays(ch, min_chain_len, strong):
    marked = getattr(ch, 'marked', None)
    n = len(ch.ptr) - 1
    if marked is None or len(marked) != len(ch.img) or not marked.any():
        return
    chain_of = np.repeat(np.arange(n), np.diff(ch.ptr))
    has_bad = np.bincount(chain_of[marked], minlength=n) > 0
    new_len = np.bincount(chain_of[~marked], minlength=n)
    drop = has_bad & (True if strong else (new_len < min_chain_len))
    for i in np.nonzero(drop)[0][::-1].tolist():
        if strong:
            print("deleting entire match that contains a bad element", i)
        else:
            sel = np.arange(ch.ptr[i], ch.ptr[i + 1])
            sel = sel[~marked[sel]]
            row = [ch.ned[i].tolist() if ch.has_ned[i] else None, int(ch.group[i])] + \
                [[a, b] for a, b in zip(ch.img[sel].tolist(), ch.uv[sel].tolist())]
            print("deleting match that is now in less than %d images:" % min_chain_len, row)
    keep_chain = ~drop
    keep_mem = ~marked & keep_chain[chain_of]
    ptr = np.zeros(int(keep_chain.sum()) + 1, np.int64)
    np.cumsum(new_len[keep_chain], out=ptr[1:])
    ch.img = ch.img[keep_mem]
    ch.uv = ch.uv[keep_mem]
    ch.ptr = ptr
    ch.ned = ch.ned[keep_chain]
    ch.has_ned = ch.has_ned[keep_chain]
    ch.group = ch.group[keep_chain]
    ch.marked = np.zeros(len(ch.img), bool)


# ---------------------------------------------------------------------------------------------
# observation -> (match index, feature index)
# ---------------------------------------------------------------------------------------------
def observation_features(matches, match_index, image_index):
    """For every observation (its chain `match_index[i]`, its camera's image `image_index[i]`):
    the index in match[2:] of the LAST member of the chain from that image (4b-mre-by-image.py:80-85
    overwrites its match_index in the loop), 0 when there is none."""
    match_index = np.asarray(match_index, np.int64)
    image_index = np.asarray(image_index, np.int64)
    out = np.zeros(len(match_index), np.int64)
    if _arrays(matches):
        ptr, img = matches.ptr, matches.img
        lo = ptr[match_index]
        ln = ptr[match_index + 1] - lo
        rep = np.repeat(np.arange(len(match_index)), ln)
        start = np.cumsum(ln) - ln
        pos = np.arange(int(ln.sum())) - np.repeat(start, ln)
        hit = img[lo[rep] + pos] == image_index[rep]
        np.maximum.at(out, rep[hit], pos[hit])
        return out
    for i, (m, im) in enumerate(zip(match_index.tolist(), image_index.tolist())):
        k = 0
        for j, p in enumerate(matches[m][2:]):
            if p[0] == im:
                k = j
        out[i] = k
    return out


# ---------------------------------------------------------------------------------------------
# the report (4b-mre-by-image.py:55-110) and the marking (:112-150)
# ---------------------------------------------------------------------------------------------
class MreReport(object):
    """n_error (= len(error) of the reference: 2 per observation), mre / std / max of the signed
    residual vector (np.mean(np.abs(r)), np.std(r), np.amax(np.abs(r))), `by_cam`: per camera
    [mean e, max e, name] in the reference's results_by_cam order (stable, descending mean;
    9999.0 for a camera without observations), `e`: the per-observation errors (device tensor,
    camera-major), `summary`: the device summary (kernels.REPROJ_*)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def mre_by_image(opt, matches, x=None, proj=None):
    import torch
    from . import kernels
    C = opt.n_cameras
    d = opt._device(opt.by_camera_point_indices, opt.by_camera_points_2d)
    x = opt._x0() if x is None else np.asarray(x, np.float64)
    cams, pts, calib = opt._upload(x, C, opt.n_points)
    if pts.numel() == 0:
        pts = torch.zeros(3, dtype=torch.float64, device=cams.device)
    counts = np.bincount(d['cam_idx_host'], minlength=C).astype(np.int64)
    cam_ptr = np.zeros(C + 1, np.int64)
    np.cumsum(counts, out=cam_ptr[1:])
    cam_stats, summary, e = kernels.ba_reproj_stats(
        cams, pts, d['cam_idx'], d['pt_idx'], d['uv'], calib,
        torch.from_numpy(cam_ptr).to(cams.device))
    host = torch.cat([cam_stats.reshape(-1), summary]).cpu().numpy()     # the one synchronisation
    rows_np, s = host[:3 * C].reshape(C, 3), host[3 * C:]
    rows = []
    for i in range(C):
        name = proj.image_list[opt.camera_map_fwd[i]].name if proj is not None \
            else opt.camera_map_fwd[i]
        if rows_np[i, 2] > 0:
            rows.append([float(rows_np[i, 0]), float(rows_np[i, 1]), name])
        else:
            rows.append([9999.0, 9999.0, name])
    by_cam = sorted(rows, key=lambda fields: fields[0], reverse=True)
    return MreReport(n_obs=d['n_obs'], n_error=2 * d['n_obs'],
                     mre=float(s[kernels.REPROJ_MEAN_ABS_R]), std=float(s[kernels.REPROJ_STD_R]),
                     max=float(s[kernels.REPROJ_MAX_ABS_R]), by_cam=by_cam, e=e, summary=summary,
                     cam_idx=d['cam_idx_host'], pt_idx=d['pt_idx_host'],
                     camera_map_fwd=np.array([opt.camera_map_fwd[i] for i in range(C)], np.int64),
                     feat_map_rev=opt.feat_map_rev, matches=matches)


def flagged(report, trim_stddev, max_error=None):
    """Device pass 2: (observation indices in the reference's marking order, their e, mre of e,
    stddev of e).  max_error follows the reference's `args.max and e > args.max` (0 / None: off)."""
    from . import kernels
    idx, e_sel = kernels.ba_mark_outliers(report.e, report.summary, trim_stddev,
                                          max_error=max_error if max_error else None)
    s = report.summary.cpu().numpy()                                       # the one synchronisation
    n = int(s[kernels.REPROJ_COUNT])
    idx = idx[:n].cpu().numpy()
    e_sel = e_sel[:n].cpu().numpy()
    order = np.argsort(-e_sel, kind='stable')          # descending e; ties stay ascending
    return idx[order], e_sel[order], float(s[kernels.REPROJ_MRE_E]), float(s[kernels.REPROJ_STDDEV_E])


def mark_outliers(matches, report, trim_stddev, max_error=None):
    print("Marking outliers...")
    print(" computing stats...")
    obs, err, mre, stddev = flagged(report, trim_stddev, max_error)
    print("mre = %.4f stddev = %.4f" % (mre, stddev))
    print(" marking outliers...")
    fmap = report.feat_map_rev
    match_index = np.fromiter((fmap[j] for j in report.pt_idx[obs].tolist()), np.int64, len(obs))
    image_index = report.camera_map_fwd[report.cam_idx[obs]]
    feat_index = observation_features(matches, match_index, image_index)
    for m, f, e in zip(match_index.tolist(), feat_index.tolist(), err.tolist()):
        mark_feature(matches, m, f, e)
    return len(obs)


# ---------------------------------------------------------------------------------------------
# co-located cameras (4b-colocated-feats.py:47-91)
# ---------------------------------------------------------------------------------------------
def marks_from_counts(ptr, count):
    """per-member pair counts -> the reference's mark_list: [chain, member] repeated count times,
    chains ascending, members ascending (its loops append [k, i] for every j > i that is close)"""
    count = np.asarray(count, np.int64)
    hit = np.nonzero(count)[0]
    if len(hit) == 0:
        return []
    ptr = np.asarray(ptr, np.int64)
    chain = np.searchsorted(ptr, hit, side='right') - 1
    member = hit - ptr[chain]
    rep = count[hit]
    return np.stack([np.repeat(chain, rep), np.repeat(member, rep)], 1).tolist()


def colocated_features(proj, matches, group_list, group_index, min_angle):
    """The mark list of scripts/4b-colocated-feats.py: for every chain of group `group_index`, every
    pair of members i < j whose images are both in the group and whose two cameras (camera_pose_opt
    positions) see the chain's position under less than `min_angle` degrees contributes [chain, i].
    The angle is the one the reference's compute_angle() means: its script never imports math, so as
    written every pair comes back as 0 and is marked.  Duplicates are kept (a member close to two
    others is listed twice), as the reference prints and counts them."""
    import torch
    from . import kernels, match_cleanup
    from .kernels import _ptr, check, lib, stream_ptr
    if not 0 <= group_index < len(group_list):
        raise IndexError("group %d of %d" % (group_index, len(group_list)))
    min_angle = float(min_angle)
    if np.isnan(min_angle):
        raise ValueError("min_angle is NaN")
    n_img = len(proj.image_list)
    n = len(matches)
    if n == 0:
        check(lib().iamx_chain_pair_angles(None, None, None, None, 0, group_index, None, None, n_img,
                                           min_angle, None, None, None, None), 'iamx_chain_pair_angles')
        return []
    ptr, img, _uv, group, ned, has_ned = match_cleanup.chain_arrays(matches)
    missing = np.nonzero((group == group_index) & ~has_ned)[0]
    if len(missing):
        raise ValueError("chain %d of group %d has no position (match[0] is None): triangulate the "
                         "chains before looking for co-located cameras" % (int(missing[0]), group_index))
    pos = np.zeros((n_img, 3))
    for i, image in enumerate(proj.image_list):
        pos[i] = image.get_camera_pose(opt=True)[0]
    in_group = match_cleanup.group_membership(proj, group_list, group_index)
    dev = kernels.require_gpu()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_ptr, d_img, d_group, d_ned, d_pos, d_in = (t(a) for a in (ptr, img, group, ned, pos, in_group))
    d_count = torch.empty(max(len(img), 1), dtype=torch.int32, device=dev)
    d_total = torch.empty(1, dtype=torch.int64, device=dev)
    d_status = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib().iamx_chain_pair_angles(_ptr(d_ptr), _ptr(d_img), _ptr(d_group), _ptr(d_ned), n, group_index,
                                       _ptr(d_pos), _ptr(d_in), n_img, min_angle, _ptr(d_count),
                                       _ptr(d_total), _ptr(d_status), stream_ptr()),
          'iamx_chain_pair_angles')
    match_cleanup.raise_bad_image(d_status.cpu().numpy(), img, ptr, n_img, 'colocated_features')
    if int(d_total.item()) == 0:
        return []
    mark_list = marks_from_counts(ptr, d_count[:len(img)].cpu().numpy())
    assert len(mark_list) == int(d_total.item())
    return mark_list


# ---------------------------------------------------------------------------------------------
# surface consistency and depth (the reference's 4c-surface-outliers3.py and 4c-by-depth.py; the
# rules are stated in include/iamx.h and DESIGN.md section 4, restated by tests/surface_cull_restatement.py)
# ---------------------------------------------------------------------------------------------
class ObservationTable(object):
    """host arrays: img_ptr i64 [n_images + 1], uv [n_obs, 2], ned [n_obs, 3], chain i32 [n_obs]
    (image-major: a stable sort of the looked-at chains' in-group members by image), chain_ptr i64
    [n_chains + 1] / chain_obs i32 [n_obs] (each chain's observations in member order), looked bool
    [n_chains]; after upload() the same names with a d_ prefix are device tensors."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def upload(self):
        import torch
        from . import kernels
        dev = kernels.require_gpu()
        for name in ('img_ptr', 'uv', 'ned', 'chain', 'chain_ptr', 'chain_obs'):
            setattr(self, 'd_' + name, torch.from_numpy(np.ascontiguousarray(getattr(self, name))).to(dev))
        self.d_looked = torch.from_numpy(self.looked.astype(np.uint8)).to(dev)
        return self


def observation_table(proj, matches, group_list, group_index, alive=None, min_members=1):
    """The members of the looked-at chains (group tag == group_index, alive, and at least
    `min_members` members in the group) whose image is in the group.  A looked-at chain without a
    position raises ValueError, an image index outside the project IndexError."""
    from . import match_cleanup
    if not 0 <= group_index < len(group_list):
        raise IndexError("group %d of %d" % (group_index, len(group_list)))
    n_img = len(proj.image_list)
    ptr, img, uv, group, ned, has_ned = match_cleanup.chain_arrays(matches)
    n = len(ptr) - 1
    looked = group == group_index
    if alive is not None:
        looked = looked & np.asarray(alive, bool)
    missing = np.nonzero(looked & ~has_ned)[0]
    if len(missing):
        raise ValueError("chain %d of group %d has no position (match[0] is None): triangulate the "
                         "chains before culling them by surface or depth" % (int(missing[0]), group_index))
    chain_of = np.repeat(np.arange(n), np.diff(ptr))
    sel = looked[chain_of]
    bad = np.nonzero(sel & ((img < 0) | (img >= n_img)))[0]
    if len(bad):
        raise IndexError("observation_table: chain %d refers to image %d, the project has %d images"
                         % (int(chain_of[bad[0]]), int(img[bad[0]]), n_img))
    in_group = match_cleanup.group_membership(proj, group_list, group_index).astype(bool)
    sel = sel & in_group[np.where(sel, img, 0)] if n_img else np.zeros(len(img), bool)
    if min_members > 1:
        looked = looked & (np.bincount(chain_of[sel], minlength=n) >= min_members)
        sel = sel & looked[chain_of]
    members = np.nonzero(sel)[0]
    order = np.argsort(img[members], kind='stable')
    obs = members[order]
    img_ptr = np.zeros(n_img + 1, np.int64)
    np.cumsum(np.bincount(img[members], minlength=n_img), out=img_ptr[1:])
    chain_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(chain_of[members], minlength=n), out=chain_ptr[1:])
    chain_obs = np.zeros(len(members), np.int32)
    chain_obs[order] = np.arange(len(members), dtype=np.int32)
    chain = chain_of[obs].astype(np.int32)
    return ObservationTable(img_ptr=img_ptr, uv=np.ascontiguousarray(uv[obs]), ned=np.ascontiguousarray(ned[chain]),
                            chain=chain, chain_ptr=chain_ptr, chain_obs=chain_obs, looked=looked,
                            n_chains=n, n_images=n_img)


class SurfaceReport(object):
    """metric f64 / count i32 / looked u8 [n_chains] (device tensors), n_small and n_flat (queries
    skipped because their image has fewer than 3 observations / no neighbour at a distance),
    n_uncounted (looked-at chains nobody addressed: the reference's "count is zero"), n_looked,
    table (the ObservationTable)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def surface_consistency(proj, matches, group_list, group_index, k=30, positives=10, alive=None):
    """One pass of the reference's compute_surface_outliers() up to its metric: every observation's
    nearest neighbours in its image, the line of 3-D over pixel distance through them, and per chain
    the mean misfit of the neighbours that are its members (iamx_surface_knn_fit,
    iamx_surface_chain_metric).  One synchronisation, for the four counts."""
    from . import kernels
    if not (1 <= k <= kernels.SURFACE_MAX_K and 1 <= positives <= kernels.SURFACE_MAX_K):
        raise ValueError("k and positives must be within 1..%d" % kernels.SURFACE_MAX_K)
    table = observation_table(proj, matches, group_list, group_index, alive).upload()
    tgt, val, _used, _fit, status = kernels.surface_knn_fit(table.d_img_ptr, table.d_uv, table.d_ned,
                                                            table.d_chain, k, positives)
    _sum, count, metric, counters = kernels.surface_chain_metric(tgt, val, status, table.d_looked,
                                                                 table.n_chains)
    c = counters.cpu().numpy()                                             # the one synchronisation
    return SurfaceReport(metric=metric, count=count, looked=table.d_looked, table=table,
                         n_small=int(c[kernels.SURFACE_N_SMALL]), n_flat=int(c[kernels.SURFACE_N_FLAT]),
                         n_uncounted=int(c[kernels.SURFACE_N_UNCOUNTED]),
                         n_looked=int(c[kernels.SURFACE_N_LOOKED]))


def outlier_stats(metric, looked, factor, two_sided):
    """iamx_chain_outlier_stats -> host (flagged chains ascending, their metric, average, stddev)"""
    from . import kernels
    stats, _flag, idx, sel, n_flagged = kernels.chain_outlier_stats(metric, looked, factor, two_sided)
    s = stats.cpu().numpy()
    n = int(n_flagged.item())
    return (idx[:n].cpu().numpy().astype(np.int64), sel[:n].cpu().numpy(),
            float(s[kernels.STATS_AVERAGE]), float(s[kernels.STATS_STDDEV]))


def surface_outliers(report, stddev=5):
    """-> (chains with |average - metric| >= stddev * deviation by descending |metric|, ties in chain
    order: the reference's sorted report; average; deviation)"""
    idx, sel, average, dev = outlier_stats(report.metric, report.looked, stddev, True)
    order = np.argsort(-np.abs(sel), kind='stable')
    return idx[order], average, dev


def cull_surface(proj, matches, group_list, group_index, stddev=5, max_rounds=None, k=30, positives=10):
    """The reference's `while result > 0` loop: rounds of surface_consistency / surface_outliers on
    an alive mask (a culled chain leaves the observation table; `matches` is not edited between
    rounds), then every member of every culled chain is marked, so that
    delete_marked_features(matches, min_chain_len) removes the chain.  -> the chains culled per
    round (a last empty list when the loop ended by itself)."""
    alive = np.ones(len(matches), bool)
    rounds = []
    while max_rounds is None or len(rounds) < max_rounds:
        report = surface_consistency(proj, matches, group_list, group_index, k, positives, alive)
        idx, average, dev = surface_outliers(report, stddev)
        print("average value = %.2f" % average)
        print("standard deviation = %.2f" % dev)
        print("round %d: culled %d chains (skipped: %d observations in images with < 3, %d without a "
              "distant neighbour; %d chains never a neighbour)"
              % (len(rounds) + 1, len(idx), report.n_small, report.n_flat, report.n_uncounted))
        rounds.append([int(c) for c in idx])
        if len(idx) == 0:
            break
        alive[idx] = False
    for c in sorted(c for r in rounds for c in r):
        if _arrays(matches):                       # (indexing a Chains would turn it into lists)
            members = int(matches.ptr[c + 1] - matches.ptr[c])
        else:
            members = len(matches[c]) - 2
        for j in range(members):
            mark_feature(matches, c, j, "-", quiet=True)
    return rounds


class DepthReport(object):
    """metric f64 / looked u8 [n_chains] (device tensors), z: host [n_images, 3] = mean, population
    deviation and count of each image's depths, table (the ObservationTable)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def chain_depths(proj, matches, group_list, group_index):
    """scripts/4c-by-depth.py's compute_feature_depths(): chains of the group with at least two
    members in it; per member the distance from its camera (camera_pose_opt) to the chain's position,
    per image their mean and deviation, per chain the mean |depth - image mean| (iamx_chain_depths)."""
    import torch
    from . import kernels
    table = observation_table(proj, matches, group_list, group_index, min_members=2).upload()
    pos = np.zeros((table.n_images, 3))
    for i, image in enumerate(proj.image_list):
        pos[i] = image.get_camera_pose(opt=True)[0]
    d_pos = torch.from_numpy(pos).to(table.d_ned.device)
    _depth, z, metric, looked = kernels.chain_depths(table.d_img_ptr, table.d_ned, d_pos, table.d_chain_ptr,
                                                     table.d_chain_obs)
    return DepthReport(metric=metric, looked=looked, z=z.cpu().numpy(), table=table)


def depth_outliers(proj, matches, group_list, group_index, stddev=3):
    """-> (mark list [[chain, 0], ...] of the chains whose metric > mean + stddev * deviation, by
    descending metric, ties in chain order; per-image rows (name, count, avg, std), avg and std None
    for an image without depths).  Member 0 is what the reference marks: its rows are
    [metric_avg, i, 0]."""
    report = chain_depths(proj, matches, group_list, group_index)
    rows = [(image.name, int(z[2]), float(z[0]) if z[2] else None, float(z[1]) if z[2] else None)
            for image, z in zip(proj.image_list, report.z)]
    print("Marking outliers...")
    print(" computing stats...")
    idx, sel, mean, dev = outlier_stats(report.metric, report.looked, stddev, False)
    print("mean = %.4f stddev = %.4f" % (mean, dev))
    order = np.argsort(-sel, kind='stable')
    return [[int(c), 0] for c in idx[order]], rows


def weak_images(matches, n_images, min_features=25):
    """scripts/4c-by-depth.py's weak-image rule: [chain, member] of every unmarked member that lies
    in an image holding between 1 and min_features - 1 unmarked members."""
    if _arrays(matches):
        img = matches.img
        if len(img) and (img.min() < 0 or img.max() >= n_images):
            raise IndexError("weak_images: an image index outside the project's %d images" % n_images)
        live = ~_marks(matches)
        count = np.bincount(img[live], minlength=n_images)
        weak = (count > 0) & (count < min_features)
        hit = np.nonzero(live & weak[img])[0]
        chain = np.searchsorted(matches.ptr, hit, side='right') - 1
        return np.stack([chain, hit - matches.ptr[chain]], 1).tolist() if len(hit) else []
    count = [0] * n_images
    for match in matches:
        for p in match[2:]:
            if p != MARK:
                if not 0 <= p[0] < n_images:
                    raise IndexError("weak_images: an image index outside the project's %d images" % n_images)
                count[p[0]] += 1
    weak = set(i for i, n in enumerate(count) if 0 < n < min_features)
    return [[c, j] for c, match in enumerate(matches) for j, p in enumerate(match[2:])
            if p != MARK and p[0] in weak]


# ---------------------------------------------------------------------------------------------
# interactive review (cv2 windows; no device path)
# ---------------------------------------------------------------------------------------------
def _cv2():
    try:
        import cv2
    except ImportError:
        raise RuntimeError("interactive outlier review needs OpenCV (cv2), which is not installed; "
                           "run without --interactive to mark outliers by the stddev / max rule")
    return cv2


def draw_match(i, index, matches, image_list):
    """Show a crop of every image of chain i (at most 21) around its member; member `index` (or
    both members of a pair) in red, the others green.  Returns the key pressed."""
    cv2 = _cv2()
    half = 300
    match = matches[i]
    print('match:', match, 'index:', index)
    for j, m in enumerate(match[2:22]):
        img = image_list[m[0]]
        print(' ', m, img)
        rgb = img.load_rgb()
        h, w = rgb.shape[:2]
        cx = min(max(int(round(m[1][0])), half), w - half)
        cy = min(max(int(round(m[1][1])), half), h - half)
        crop = rgb[cy - half:cy + half, cx - half:cx + half]
        color = (0, 0, 255) if (j == index or len(match) == 3) else (0, 255, 0)
        mark = (int(round(m[1][0])) - cx + half, int(round(m[1][1])) - cy + half)
        cv2.circle(crop, mark, 2, color, thickness=2)
        cv2.imshow(img.name + ' (%d)' % m[0], crop)
    print('waiting for keyboard input...')
    key = cv2.waitKey() & 0xff
    cv2.destroyAllWindows()
    return key


def show_outliers(result_list, matches, image_list):
    """result_list: [e, match index, feature index] rows, worst first.  'd' marks the shown
    member for deletion, 'q' / Esc ends the review.  Returns the [match, feature] list."""
    _cv2()
    print("Show outliers...")
    e = np.array([r[0] for r in result_list], np.float64)
    print(" computing stats...")
    mre = float(np.sum(e[::-1])) / len(e) if len(e) else float('nan')
    stddev = float(np.sqrt(np.sum((mre - e) ** 2) / len(e))) if len(e) else float('nan')
    print("avg error = %.4f stddev = %.4f" % (mre, stddev))
    mark_list = []
    for line in result_list:
        print("  outlier index %d-%d err=%.2f" % (line[1], line[2], line[0]))
        key = draw_match(line[1], line[2], matches, image_list)
        if key == ord('d'):
            mark_list.append([line[1], line[2]])
        elif key in (27, ord('q')):
            break
    return mark_list
