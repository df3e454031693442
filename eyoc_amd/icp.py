"""ICP refinement on the GPU - point-to-point (``eyoc_icp_batched``, csrc/icp.hip) with the reference's call surfaces, and point-to-plane.

* ``registration_icp`` stands in for ``o3d.pipelines.registration.registration_icp(pcd0, pcd1, r, init,
  TransformationEstimationPointToPoint(), ICPConvergenceCriteria(max_iteration=200))`` at ``lib/data_loaders.py:485-515`` (through
  ``eyoc_amd.o3d`` those lines run unchanged);
* ``icp_refine`` mirrors ``scripts/SC2_PCR/benchmark_utils.py:40-56``;
* ``icp_batched`` refines a batch of pairs in one call and leaves the records on the device; ``correspondences`` is one
  evaluation of the contract (nearest target row under a gate, fp64) on the same cell grid;
* ``estimate_normals`` / ``estimate_normals_batched`` (``eyoc_normals_batched``) and ``registration_icp_point_to_plane`` /
  ``icp_plane_batched`` (``eyoc_icp_plane_batched``) are Open3D's ``estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))`` and
  ``registration_icp`` with ``TransformationEstimationPointToPlane``, restated the same way; the reference has no call site for them.

The algorithm is restated from Open3D's published source - parity unpinned, see DESIGN.md 4 - and documented in
``include/eyoc_hip.h``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .eval import _cuda_f32
from .registration import RegistrationResult

CONVERGED, BAD_INIT, FEW, RANGE = 1, 2, 4, 8      # eyoc_icp_result.status
SINGULAR = 16                                     # ... of the point-to-plane runs only: the step's 6 x 6 system had a negligible pivot
RECORD_BYTES = C.sizeof(_lib.IcpResult)           # 160


def _segs(seg):
    seg = [int(v) for v in seg]
    return (C.c_int32 * len(seg))(*seg), seg


def _clouds(who, src, tgt, seg_src, seg_tgt, one_pair=False):
    """What both entry points start from: the clouds as f32 ``[n, 3]`` on one device, their segments as C arrays (``one_pair``: a
    segment list that is ``None`` means one pair), the number of pairs and the uninitialised ``[P, 160]`` record tensor."""
    s = _cuda_f32(src).reshape(-1, 3)
    t = _cuda_f32(tgt, s.device).reshape(-1, 3)
    ss, seg_s = _segs([0, s.shape[0]] if one_pair and seg_src is None else seg_src)
    st, seg_t = _segs([0, t.shape[0]] if one_pair and seg_tgt is None else seg_tgt)
    P = len(seg_s) - 1
    if len(seg_t) != P + 1 or seg_s[-1] != s.shape[0] or seg_t[-1] != t.shape[0]:
        raise ValueError(f"{who}: the segments do not describe the clouds")
    return s, t, ss, st, P, torch.empty((P, RECORD_BYTES), dtype=torch.uint8, device=s.device)


def _poses(T, P, device):
    """``[P, 4, 4]`` / ``[4, 4]`` / ``[P, 16]`` poses (numpy or torch, any float type) -> contiguous f64 ``[P, 16]`` on ``device``."""
    if not isinstance(T, torch.Tensor):
        T = torch.from_numpy(np.ascontiguousarray(np.asarray(T, np.float64)))
    T = T.to(device=device, dtype=torch.float64).reshape(-1, 16)
    if T.shape[0] == 1 and P > 1:
        T = T.expand(P, 16)
    if T.shape[0] != P:
        raise ValueError(f"{T.shape[0]} poses for {P} pairs")
    return T.contiguous()


def icp_batched(src, tgt, seg_src, seg_tgt, max_correspondence_distance, init=None, max_iteration=30, relative_fitness=1e-6,
                relative_rmse=1e-6, return_correspondences=False):
    """All pairs of a batch in one call, nothing read back: ``src f32 [N, 3]`` / ``tgt f32 [M, 3]`` hold the pairs back to back (pair
    ``b`` = source rows ``seg_src[b]:seg_src[b+1]``, target rows ``seg_tgt[b]:seg_tgt[b+1]``), ``init`` f64 ``[P, 4, 4]`` (host or
    device; ``None`` = identity).  Returns the ``[P, 160]`` byte tensor of ``eyoc_icp_result`` records on the device (``decode_icp_result``)
    - and, with ``return_correspondences``, ``int32 [N]``: the target row local to the pair under the returned pose, or -1."""
    s, t, ss, st, P, res = _clouds("icp_batched", src, tgt, seg_src, seg_tgt)
    T0 = None if init is None else _poses(init, P, s.device)
    p = _lib.IcpParams(float(max_correspondence_distance), float(relative_fitness), float(relative_rmse), int(max_iteration), 0)
    corr = torch.empty(s.shape[0], dtype=torch.int32, device=s.device) if return_correspondences else None
    lib = _lib.load()
    with _lib.on_device(s.device):
        ws = _lib.workspace(lib.eyoc_icp_workspace_bytes(P, s.shape[0], t.shape[0]), s.device)
        _lib.check(lib.eyoc_icp_batched(_lib.ctx(s.device.index), _lib.ptr(s), _lib.ptr(t), ss, st, P, _lib.ptr(T0), C.byref(p),
                                        _lib.ptr(res), _lib.ptr(corr), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "eyoc_icp_batched")
    return (res, corr) if return_correspondences else res


def correspondences(src, tgt, T, max_distance, seg_src=None, seg_tgt=None, return_records=False):
    """One evaluation under ``T``: -> ``(corr int32 [N], d2 f64 [N])`` on the device - the nearest target row (local to the pair, the
    lowest row on a tie) with ``d2 < max_distance ** 2``, else -1 / +inf.  One pair unless segments are given."""
    s, t, ss, st, P, res = _clouds("correspondences", src, tgt, seg_src, seg_tgt, one_pair=True)
    Td = _poses(T, P, s.device)
    corr = torch.empty(s.shape[0], dtype=torch.int32, device=s.device)
    d2 = torch.empty(s.shape[0], dtype=torch.float64, device=s.device)
    lib = _lib.load()
    with _lib.on_device(s.device):
        ws = _lib.workspace(lib.eyoc_icp_workspace_bytes(P, s.shape[0], t.shape[0]), s.device)
        _lib.check(lib.eyoc_icp_correspondences(_lib.ctx(s.device.index), _lib.ptr(s), _lib.ptr(t), ss, st, P, _lib.ptr(Td),
                                                float(max_distance), _lib.ptr(corr), _lib.ptr(d2), _lib.ptr(res), _lib.ptr(ws), ws.numel(),
                                                _lib.stream_ptr()), "eyoc_icp_correspondences")
    return (corr, d2, res) if return_records else (corr, d2)


def decode_icp_result(res, corr=None) -> RegistrationResult:
    """One 160-byte record (device or host tensor, or bytes) -> ``RegistrationResult``; ``corr``: the pair's rows of ``icp_batched``'s
    correspondence array -> ``correspondence_set int [m, 2]`` (source row, target row)."""
    raw = bytes(res) if isinstance(res, (bytes, bytearray)) else res.cpu().numpy().tobytes()
    r = _lib.IcpResult.from_buffer_copy(raw)
    out = RegistrationResult(np.array(list(r.T), np.float64).reshape(4, 4), float(r.fitness), float(r.inlier_rmse),
                             inliers=int(r.correspondences), status=int(r.status), iterations=int(r.iterations))
    if corr is not None:
        c = corr.cpu().numpy() if isinstance(corr, torch.Tensor) else np.asarray(corr)
        rows = np.flatnonzero(c >= 0)
        out.correspondence_set = np.stack([rows, c[rows].astype(np.int64)], 1)
    return out


def _points(a):
    a = getattr(a, "points", a)
    if isinstance(a, torch.Tensor):
        return a
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """Drop-in for Open3D's ``registration_icp`` (point-to-point): ``source / target`` are ``[n, 3]`` points (numpy, torch, or anything
    with a ``points`` attribute), ``criteria`` any object with ``relative_fitness / relative_rmse / max_iteration`` (default 1e-6,
    1e-6, 30).  -> ``RegistrationResult`` with ``correspondence_set``, ``iterations`` and ``status``."""
    if estimation_method is not None and (getattr(estimation_method, "with_scaling", False) or
                                          type(estimation_method).__name__ != "TransformationEstimationPointToPoint"):
        raise NotImplementedError("only TransformationEstimationPointToPoint(with_scaling=False) is implemented")
    if not torch.cuda.is_available():
        raise _lib.EyocError("no GPU visible: ICP runs on MI355X only (no CPU fallback)")
    rf, rr, it = (1e-6, 1e-6, 30) if criteria is None else (criteria.relative_fitness, criteria.relative_rmse, criteria.max_iteration)
    s, t = _points(source), _points(target)
    T0 = np.eye(4) if init is None else np.asarray(init, np.float64)
    res, corr = icp_batched(s, t, [0, s.shape[0]], [0, t.shape[0]], max_correspondence_distance, T0[None], it, rf, rr,
                            return_correspondences=True)
    return decode_icp_result(res[0], corr)


def estimate_normals_batched(pts, seg, radius, max_nn=30, return_count=False):
    """Normals of a batch of clouds (``eyoc_normals_batched``; Open3D's ``estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))``
    restated, see ``include/eyoc_hip.h``): ``pts f32 [N, 3]`` holds the clouds back to back, cloud ``b`` = rows ``seg[b]:seg[b+1]``.
    Returns ``(normals f32 [N, 3], status int32 [B])`` on the device - with ``return_count`` ``(normals, count int32 [N], status)``.  A
    row with fewer than 3 neighbours gets the zero vector; a cloud whose status is ``RANGE`` gets zeros throughout.  ``max_nn = 0``
    keeps every neighbour inside ``radius``, otherwise ``1 <= max_nn <= 64``."""
    p = _cuda_f32(pts).reshape(-1, 3)
    sc, seg_l = _segs(seg)
    B = len(seg_l) - 1
    if B < 1 or seg_l[-1] != p.shape[0]:
        raise ValueError("estimate_normals_batched: the segments do not describe the clouds")
    normals = torch.empty((p.shape[0], 3), dtype=torch.float32, device=p.device)
    count = torch.empty(p.shape[0], dtype=torch.int32, device=p.device) if return_count else None
    status = torch.empty(B, dtype=torch.int32, device=p.device)
    lib = _lib.load()
    with _lib.on_device(p.device):
        ws = _lib.workspace(lib.eyoc_normals_workspace_bytes(B, p.shape[0]), p.device)
        _lib.check(lib.eyoc_normals_batched(_lib.ctx(p.device.index), _lib.ptr(p), sc, B, float(radius), int(max_nn), _lib.ptr(normals),
                                            _lib.ptr(count), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "eyoc_normals_batched")
    return (normals, count, status) if return_count else (normals, status)


def estimate_normals(points, radius, max_nn=30):
    """One cloud: ``[n, 3]`` points (numpy, torch, or anything with a ``points`` attribute) -> ``f32 [n, 3]`` normals on the device,
    pointing towards the origin.  Raises for a cloud the grid cannot hold (a non-finite point, a point beyond 2^17 cells)."""
    if not torch.cuda.is_available():
        raise _lib.EyocError("no GPU visible: normal estimation runs on MI355X only (no CPU fallback)")
    p = _points(points)
    normals, status = estimate_normals_batched(p, [0, p.shape[0]], radius, max_nn)
    if int(status[0]) != 0:
        raise _lib.EyocError("estimate_normals: a point is not finite or lies outside the grid's range", _lib.ERR_RANGE)
    return normals


def icp_plane_batched(src, tgt, tgt_normals, seg_src, seg_tgt, max_correspondence_distance, init=None, max_iteration=30,
                      relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False):
    """``icp_batched`` with the point-to-plane step (``eyoc_icp_plane_batched``): ``tgt_normals f32 [M, 3]`` are the target rows' normals
    (``estimate_normals_batched``).  Same records, same correspondences; a pair whose 6 x 6 system is singular stops with ``SINGULAR``."""
    s, t, ss, st, P, res = _clouds("icp_plane_batched", src, tgt, seg_src, seg_tgt)
    n = _cuda_f32(tgt_normals, s.device).reshape(-1, 3)
    if n.shape[0] != t.shape[0]:
        raise ValueError(f"icp_plane_batched: {n.shape[0]} normals for {t.shape[0]} target rows")
    T0 = None if init is None else _poses(init, P, s.device)
    p = _lib.IcpParams(float(max_correspondence_distance), float(relative_fitness), float(relative_rmse), int(max_iteration), 0)
    corr = torch.empty(s.shape[0], dtype=torch.int32, device=s.device) if return_correspondences else None
    lib = _lib.load()
    with _lib.on_device(s.device):
        ws = _lib.workspace(lib.eyoc_icp_plane_workspace_bytes(P, s.shape[0], t.shape[0]), s.device)
        _lib.check(lib.eyoc_icp_plane_batched(_lib.ctx(s.device.index), _lib.ptr(s), _lib.ptr(t), _lib.ptr(n), ss, st, P, _lib.ptr(T0),
                                              C.byref(p), _lib.ptr(res), _lib.ptr(corr), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "eyoc_icp_plane_batched")
    return (res, corr) if return_correspondences else res


def registration_icp_point_to_plane(source, target, max_correspondence_distance, init=None, criteria=None, target_normals=None,
                                    normal_radius=None, max_nn=30):
    """Open3D's ``registration_icp(..., TransformationEstimationPointToPlane())`` for one pair: -> ``RegistrationResult`` like
    ``registration_icp``.  ``target_normals [m, 3]``: the target's normals; ``None``: they are estimated on the device from the target
    itself (``estimate_normals(target, normal_radius, max_nn)``), ``normal_radius`` is then mandatory."""
    if not torch.cuda.is_available():
        raise _lib.EyocError("no GPU visible: ICP runs on MI355X only (no CPU fallback)")
    rf, rr, it = (1e-6, 1e-6, 30) if criteria is None else (criteria.relative_fitness, criteria.relative_rmse, criteria.max_iteration)
    s, t = _points(source), _points(target)
    if target_normals is None:
        if normal_radius is None:
            raise ValueError("registration_icp_point_to_plane: normal_radius is needed when no target_normals are given")
        t = _cuda_f32(t).reshape(-1, 3)
        target_normals, _ = estimate_normals_batched(t, [0, t.shape[0]], normal_radius, max_nn)    # a RANGE cloud is RANGE in the ICP too
    elif not isinstance(target_normals, torch.Tensor):
        target_normals = torch.from_numpy(np.ascontiguousarray(np.asarray(target_normals, np.float32)))
    T0 = np.eye(4) if init is None else np.asarray(init, np.float64)
    res, corr = icp_plane_batched(s, t, target_normals, [0, s.shape[0]], [0, t.shape[0]], max_correspondence_distance, T0[None], it, rf, rr,
                                  return_correspondences=True)
    return decode_icp_result(res[0], corr)


def icp_refine(src_keypts, tgt_keypts, pred_trans, max_correspondence_distance=0.10):
    """scripts/SC2_PCR/benchmark_utils.py:40-56: ``src_keypts / tgt_keypts [1, n, 3]``, ``pred_trans [1, 4, 4]`` -> the refined
    ``[1, 4, 4]`` float32 pose on ``pred_trans``'s device (gate 0.10 m, 30 iterations, like the reference)."""
    r = registration_icp(src_keypts[0].detach(), tgt_keypts[0].detach(), max_correspondence_distance,
                         pred_trans[0].detach().cpu().numpy().astype(np.float64))
    return torch.from_numpy(r.transformation[None]).to(device=pred_trans.device, dtype=torch.float32)
