"""MI355X-path counterpart of the reference's keypoint undistortion (scripts/lib/project.py:257-296):

    undistort_points(uv, K, dist)                            cv2.undistortPoints(src, K, dist, P=K)
    undistort_uvlist(proj, image, uv_orig)                   ProjectMgr.undistort_uvlist
    undistort_image_keypoints(proj, image, optimized=False)  ProjectMgr.undistort_image_keypoints
    undistort_keypoints(proj, optimized=False)               ProjectMgr.undistort_keypoints
    install(project.ProjectMgr)                              the three methods onto the reference's class

The reference makes one cv2 call per image and a Python loop per keypoint before and after it; here
the points of an image go through iamx_undistort_points (csrc/chain_geom.hip) in one launch, and
undistort_keypoints sends every image's keypoints through ONE launch.  `image.uv_list` becomes an
(N, 2) float32 array: uv_list[i] is the float32 pair the reference's list holds at i, len() and
iteration work the same.

The kernel restates OpenCV's published iteration (five rounds, the default criteria) and is pinned
bit for bit to tests/undistort_restatement.py.  Parity with cv2 itself is UNPINNED: cv2 is not
available to the tests, as for CLAHE and the resizes.  There is no host path:
without a GPU these raise."""
import ctypes

import numpy as np

from . import _deps


def _k4(K):
    K = np.asarray(K, np.float64)
    if K.shape == (3, 3):
        k4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
    elif K.size == 4:
        k4 = np.ascontiguousarray(K.ravel(), np.float64)
    else:
        raise ValueError("K must be a 3x3 camera matrix or (fx, fy, cx, cy)")
    if not (np.isfinite(k4).all() and k4[0] != 0 and k4[1] != 0):
        raise ValueError("K needs finite entries and non-zero focal lengths")
    return k4


def _dist5(dist):
    d = np.asarray(dist, np.float64).ravel()
    if d.size != 5:
        raise ValueError("dist must be (k1, k2, p1, p2, k3)")
    return np.ascontiguousarray(d)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def undistort_points(uv, K, dist):
    """uv: (n, 2) (or (n, 1, 2)) pixel coordinates, read as float32 -> float32 array of the same
    shape, undistorted and re-projected through K."""
    from ._lib import check, lib, require_gpu, stream_ptr
    k4, d5 = _k4(K), _dist5(dist)
    src = np.ascontiguousarray(uv, np.float32)
    if src.size % 2 or (src.ndim and src.shape[-1] != 2):
        raise ValueError("uv must be (n, 2)")
    n = src.size // 2
    if n == 0:
        check(lib().iamx_undistort_points(None, 0, _hp(k4), _hp(d5), None, None), 'iamx_undistort_points')
        return np.zeros(src.shape, np.float32)
    import torch
    dev = require_gpu()
    d_src = torch.from_numpy(src.reshape(-1, 2)).to(dev)
    d_dst = torch.empty_like(d_src)
    check(lib().iamx_undistort_points(ctypes.c_void_p(d_src.data_ptr()), n, _hp(k4), _hp(d5),
                                      ctypes.c_void_p(d_dst.data_ptr()), stream_ptr()),
          'iamx_undistort_points')
    return d_dst.cpu().numpy().reshape(src.shape)


def _kp_pts(image):
    from .matcher import _kp_xy
    return np.ascontiguousarray(_kp_xy(image), np.float32).reshape(-1, 2)


def undistort_uvlist(proj, image, uv_orig):
    """project.py:257-275: the initial calibration, a list in, [] for an empty one"""
    if len(uv_orig) == 0:
        return []
    cam = _deps.camera()
    uv = np.array([(kp[0], kp[1]) for kp in uv_orig], np.float32).reshape(-1, 2)
    return undistort_points(uv, cam.get_K(), cam.get_dist_coeffs())


def undistort_image_keypoints(proj, image, optimized=False):
    """project.py:279-290: image.uv_list from image.kp_list (untouched when there are none)"""
    if len(image.kp_list) == 0:
        return
    cam = _deps.camera()
    image.uv_list = undistort_points(_kp_pts(image), cam.get_K(optimized), cam.get_dist_coeffs(optimized))


def undistort_keypoints(proj, optimized=False):
    """project.py:293-296, every image's keypoints in one launch"""
    _deps.logger().log("Undistorting keypoints:")
    cam = _deps.camera()
    have = [im for im in proj.image_list if len(im.kp_list)]
    if not have:
        return
    pts = [_kp_pts(im) for im in have]
    out = undistort_points(np.concatenate(pts), cam.get_K(optimized), cam.get_dist_coeffs(optimized))
    at = 0
    for im, p in zip(have, pts):
        im.uv_list = out[at:at + len(p)].copy()
        at += len(p)


def install(project_mgr_class):
    """Give the reference's lib.project.ProjectMgr the device undistortion (drop-in): the three
    methods keep their names and signatures."""
    project_mgr_class.undistort_uvlist = undistort_uvlist
    project_mgr_class.undistort_image_keypoints = undistort_image_keypoints
    project_mgr_class.undistort_keypoints = undistort_keypoints
