"""FPFH descriptors on the device (``eyoc_fpfh_batched``, ``csrc/fpfh.hip``) and the descriptor's route into matching and registration.

The reference's SC2-PCR programs take two descriptor kinds, ``fcgf`` and ``fpfh`` (``scripts/SC2_PCR/dataset.py:20,66-74``,
``config.py:63,71``); the ``fpfh`` branch L2-normalises Open3D's 33-D rows and hands them to the same ``Matcher``.  This module is that
branch without Open3D: ``compute_fpfh_batched`` restates ``compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn))`` for a
batch of clouds (the contract is in ``include/eyoc_hip.h``), ``fpfh_descriptors`` gives the rows in the form the matcher takes and
``register_fpfh_batched`` chains descriptor, nearest neighbour and pose for a batch of pairs (``downsample=True``: from raw scans,
through ``eyoc_amd.downsample`` first).  Opt-in: nothing else calls it, and
``RegistrationPipeline`` has no FPFH route.

Two differences from Open3D are by construction.  The normals of ``icp.estimate_normals_batched`` point to the origin, Open3D's are
unoriented unless the caller orients them, and FPFH depends on the orientation.  And the row's own entry is removed from its
neighbour list by index, where Open3D drops the first entry whichever row that is."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import icp as _icp
from . import registration as _reg
from .eval import _cuda_f32, knn1_segmented, mutual_correspondences

BINS = 33
PADDED = 64          # a width eyoc_knn1 takes; the 31 extra columns are zeros and change no distance


def compute_fpfh_batched(pts, seg, radius, max_nn=100, normals=None, normal_radius=None, normal_max_nn=30, normalize=False, pad=False,
                         return_hist=False):
    """FPFH rows of a batch of clouds: ``pts f32 [N, 3]`` holds the clouds back to back, cloud ``b`` = rows ``seg[b]:seg[b+1]``.
    Returns ``(feat f32 [N, 33], status int32 [B])`` on the device - ``[N, 64]`` with ``pad`` (columns 33.. are zeros), the rows divided by
    ``norm + 1e-6`` with ``normalize``; with ``return_hist`` ``(feat, hist uint8 [N, 33], count int32 [N], status)``: the SPFH counts and
    the number of neighbours of every row.  ``normals f32 [N, 3]``: the caller's; ``None`` estimates them first with
    ``icp.estimate_normals_batched(pts, seg, normal_radius, normal_max_nn)`` (``normal_radius`` is then required) and ors that call's
    status in.  A cloud whose status is ``icp.RANGE`` (a non-finite point or normal, a point beyond 2^17 cells) has zero rows.
    ``2 <= max_nn <= 128``."""
    p = _cuda_f32(pts).reshape(-1, 3)
    sc, seg_l = _icp._segs(seg)
    B = len(seg_l) - 1
    if B < 1 or seg_l[-1] != p.shape[0]:
        raise ValueError("compute_fpfh_batched: the segments do not describe the clouds")
    status_n = None
    if normals is None:
        if normal_radius is None:
            raise ValueError("compute_fpfh_batched: without normals, normal_radius is required")
        nr, status_n = _icp.estimate_normals_batched(p, seg_l, normal_radius, normal_max_nn)
    else:
        nr = _cuda_f32(normals, p.device).reshape(-1, 3)
        if nr.shape[0] != p.shape[0]:
            raise ValueError("compute_fpfh_batched: points and normals disagree in length")
    stride = PADDED if pad else BINS
    feat = torch.empty((p.shape[0], stride), dtype=torch.float32, device=p.device)
    hist = torch.empty((p.shape[0], BINS), dtype=torch.uint8, device=p.device) if return_hist else None
    count = torch.empty(p.shape[0], dtype=torch.int32, device=p.device) if return_hist else None
    status = torch.empty(B, dtype=torch.int32, device=p.device)
    lib = _lib.load()
    with _lib.on_device(p.device):
        ws = _lib.workspace(lib.eyoc_fpfh_workspace_bytes(B, p.shape[0], int(max_nn)), p.device)
        _lib.check(lib.eyoc_fpfh_batched(_lib.ctx(p.device.index), _lib.ptr(p), _lib.ptr(nr), sc, B, float(radius), int(max_nn),
                                         int(bool(normalize)), stride, _lib.ptr(feat), _lib.ptr(hist), _lib.ptr(count), _lib.ptr(status),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "eyoc_fpfh_batched")
        if status_n is not None:
            status |= status_n
    return (feat, hist, count, status) if return_hist else (feat, status)


def compute_fpfh_feature(points, radius, max_nn=100, normals=None, normal_radius=None, normal_max_nn=30, normalize=False, pad=False):
    """One cloud: ``[n, 3]`` points (numpy, torch, or anything with a ``points`` attribute) -> ``f32 [n, 33]`` (or ``[n, 64]``) on the
    device.  Raises for a cloud the grid cannot hold, like ``icp.estimate_normals``."""
    if not torch.cuda.is_available():
        raise _lib.EyocError("no GPU visible: FPFH runs on MI355X only (no CPU fallback)")
    if normals is None:
        normals = getattr(points, "normals", None)
        if normals is not None and len(normals) == 0:
            normals = None
    p = _icp._points(points)
    feat, status = compute_fpfh_batched(p, [0, p.shape[0]], radius, max_nn, None if normals is None else _icp._points(normals),
                                        normal_radius, normal_max_nn, normalize, pad)
    if int(status[0]) != 0:
        raise _lib.EyocError("compute_fpfh_feature: a point or normal is not finite or a point lies outside the grid's range", _lib.ERR_RANGE)
    return feat


def fpfh_descriptors(pts, seg, voxel_size, normal_radius=None, normal_max_nn=30, radius=None, max_nn=100, normals=None):
    """The ``fpfh`` input of the reference's SC2-PCR programs for a batch of clouds: L2-normalised rows (``feature / (norm + 1e-6)``,
    ``scripts/SC2_PCR/dataset.py``), padded to 64 columns for ``eyoc_knn1``.  Radii: the customary Open3D choices for a cloud that was
    voxelised at ``voxel_size`` - normals from ``2 * voxel_size`` / 30 neighbours, FPFH from ``5 * voxel_size`` / 100 neighbours - each
    overridable.  -> ``(feat f32 [N, 64], status int32 [B])``."""
    return compute_fpfh_batched(pts, seg, 5.0 * voxel_size if radius is None else radius, max_nn, normals,
                                2.0 * voxel_size if normal_radius is None else normal_radius, normal_max_nn, normalize=True, pad=True)


def register_fpfh_batched(src, tgt, seg_src, seg_tgt, voxel_size, distance_threshold, backend="ransac", mutual=False, seed=0,
                          max_iteration=4000000, matcher=None, confidence=1.0, first_check=_reg.RANSAC_FIRST_CHECK, downsample=False,
                          **descriptor_args):
    """Raw points to poses for a batch of pairs, without a network: ``fpfh_descriptors`` on both sides, the feature-space nearest
    neighbour of every source row (``eval.knn1_segmented``; ``mutual``: only the reciprocal matches, ``eval.mutual_correspondences``),
    then ``backend``:

    ``"ransac"``  ``registration.ransac_batched_from_correspondences`` with ``distance_threshold`` and ``max_iteration``; pair ``b`` draws
                  with ``seed + b``.  With ``mutual`` a pair with fewer than 4 reciprocal matches keeps all its matches, like Open3D.
                  ``confidence`` below 1 (and ``first_check``) switch that call's convergence criterion on; the results then carry ``iterations``.
    ``"sc2pcr"``  ``registration.Matcher.SC2_PCR_packed`` on the matched points (the first ``max_points`` of a pair); ``matcher``: the
                  ``Matcher`` to use, default ``Matcher(inlier_threshold=distance_threshold, num_node='all', nms_radius=distance_threshold,
                  num_iterations=20)``.  ``fitness`` is the share of matches within ``inlier_threshold`` under the pose.

    ``downsample=True``: ``src`` and ``tgt`` are raw scans; both sides go through ``downsample.voxel_down_sample_batched`` at
    ``voxel_size`` first (Open3D's ``voxel_down_sample``, the first step of its global-registration recipe) and everything below runs on
    the centroids.  The poses stay in the scans' frames; a cloud that call refuses is empty afterwards and its pair carries ``icp.RANGE``.
    ``False`` (the default): the clouds are taken as voxelised at ``voxel_size`` already.

    ``descriptor_args`` go to ``fpfh_descriptors``.  -> a list of ``RegistrationResult``, one per pair; a pair whose cloud could not be
    described (``icp.RANGE``) or that has no match carries ``status = icp.RANGE`` / ``icp.FEW`` and the identity."""
    if backend not in ("ransac", "sc2pcr"):
        raise ValueError("backend must be 'ransac' or 'sc2pcr'")
    s = _cuda_f32(src).reshape(-1, 3)
    t = _cuda_f32(tgt, s.device).reshape(-1, 3)
    seg_s, seg_t = [int(v) for v in seg_src], [int(v) for v in seg_tgt]
    P = len(seg_s) - 1
    if len(seg_t) != P + 1 or seg_s[-1] != s.shape[0] or seg_t[-1] != t.shape[0]:
        raise ValueError("register_fpfh_batched: the segments do not describe the clouds")
    st_d = None
    if downsample:
        from .downsample import voxel_down_sample_batched
        s, seg_s, st_ds = voxel_down_sample_batched(s, seg_s, voxel_size)
        t, seg_t, st_dt = voxel_down_sample_batched(t, seg_t, voxel_size)
        st_d = st_ds | st_dt
    Fs, st_s = fpfh_descriptors(s, seg_s, voxel_size, **descriptor_args)
    Ft, st_t = fpfh_descriptors(t, seg_t, voxel_size, **descriptor_args)
    bad = ((st_s | st_t) if st_d is None else (st_s | st_t | st_d)).cpu().numpy()
    if mutual:
        rows, corr, seg_m = mutual_correspondences(Fs, Ft, seg_s, seg_t, "SquareL2", min_keep=4 if backend == "ransac" else 0)
        seg_m = [int(v) for v in seg_m]
        pair = torch.repeat_interleave(torch.arange(P, device=s.device), torch.as_tensor(np.diff(seg_m), device=s.device))
        base_s = torch.as_tensor(seg_s[:-1], device=s.device, dtype=torch.int64)
        ms = s[rows + base_s[pair]].contiguous()
    else:
        corr = knn1_segmented(Fs, Ft, seg_s, seg_t, "SquareL2", return_distance=False)
        seg_m, ms = seg_s, s
        pair = torch.repeat_interleave(torch.arange(P, device=s.device), torch.as_tensor(np.diff(seg_m), device=s.device))
    ns = np.diff(seg_m)
    out = [None] * P
    for b in range(P):
        if bad[b] or ns[b] == 0 or seg_t[b + 1] == seg_t[b]:
            out[b] = _reg.RegistrationResult(np.eye(4), 0.0, 0.0, status=int(_icp.RANGE if bad[b] else _icp.FEW))
    live = [b for b in range(P) if out[b] is None]
    if not live:
        return out
    if backend == "ransac":
        # pair b draws with seed + b whatever its neighbours are: one call for every run of live pairs
        runs, b = [], 0
        while b < P:
            if out[b] is not None:
                b += 1
                continue
            e = b
            while e < P and out[e] is None:
                e += 1
            runs.append((b, e))
            b = e
        for b0, b1 in runs:
            sl = slice(seg_m[b0], seg_m[b1])
            res = _reg.ransac_batched_from_correspondences(ms[sl], t[seg_t[b0]:seg_t[b1]], corr[sl], [v - seg_m[b0] for v in seg_m[b0:b1 + 1]],
                                                           [v - seg_t[b0] for v in seg_t[b0:b1 + 1]], float(distance_threshold),
                                                           int(max_iteration), int(seed) + b0, confidence=confidence,
                                                           first_check=first_check, return_iterations=float(confidence) < 1.0)
            its = None
            if float(confidence) < 1.0:
                res, its = res[0], res[1].cpu().numpy()
            for b in range(b0, b1):
                out[b] = _reg.decode_ransac_result(res[b - b0], int(ns[b]))
                if its is not None:
                    out[b].iterations = int(its[b - b0])
        return out
    m = matcher if matcher is not None else _reg.Matcher(inlier_threshold=float(distance_threshold), num_node='all',
                                                         nms_radius=float(distance_threshold), num_iterations=20)
    base_t = torch.as_tensor(seg_t[:-1], device=s.device, dtype=torch.int64)
    sel = [torch.arange(seg_m[b], seg_m[b] + min(int(ns[b]), int(m.max_points)), device=s.device) for b in live]
    seg_l = np.concatenate([[0], np.cumsum([len(v) for v in sel])])
    sel = torch.cat(sel)
    ps, pt = ms[sel].contiguous(), t[corr[sel] + base_t[pair[sel]]].contiguous()     # live pairs only: a dead pair's matches mean nothing
    T, _, _ = m.SC2_PCR_packed(ps, pt, seg_l)
    Th = T.to(torch.float64).cpu().numpy()
    hs, ht = ps.cpu().numpy().astype(np.float64), pt.cpu().numpy().astype(np.float64)
    for i, b in enumerate(live):       # per pair and on the host: a pair's figures do not depend on its batch
        sl = slice(seg_l[i], seg_l[i + 1])
        d = np.linalg.norm(hs[sl] @ Th[i, :3, :3].T + Th[i, :3, 3] - ht[sl], axis=1)
        inl = d < float(m.inlier_threshold)
        n_in = int(inl.sum())
        out[b] = _reg.RegistrationResult(Th[i], n_in / max(len(d), 1), float(np.sqrt((d[inl] ** 2).sum() / n_in)) if n_in else 0.0, inliers=n_in)
    return out
