"""Pose solvers with the reference's names.

``est_quad_linear_robust`` / ``pose_estimation`` mirror ``util/transform_estimation.py:89-144``;
``rigid_transform_3d`` mirrors ``scripts/SC2_PCR/common.py:7-45``; ``transform`` / ``integrate_trans``
mirror ``scripts/SC2_PCR/utils/SE3.py:44-96``.  ``estimate_transform`` is the alias named by the brief.
The reductions and the 3x3 SVD / 6x6 solve run in ``libeyoc_hip.so`` (fp64 accumulation on the GPU,
no host hop).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .eval import _cuda_f32


def est_quad_linear_robust(pts0, pts1, weight=None, iters=20):
    """util/transform_estimation.py:89-116 -> ``T f32 [4,4]`` on the device of ``pts0``."""
    src_dev = pts0.device
    p0 = _cuda_f32(pts0)
    p1 = _cuda_f32(pts1, p0.device)
    if p0.shape != p1.shape or p0.dim() != 2 or p0.shape[1] != 3:
        raise ValueError("pts0 and pts1 must both be [N,3]")
    w = None if weight is None else _cuda_f32(weight, p0.device).reshape(-1)
    if w is not None and w.numel() != p0.shape[0]:
        raise ValueError("weight must have one entry per point")
    T = torch.empty((4, 4), dtype=torch.float32, device=p0.device)
    with torch.cuda.device(p0.device):
        _lib.check(_lib.load().eyoc_irls_quad(_lib.ctx(p0.device.index), _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(w),
                                              p0.shape[0], int(iters), _lib.ptr(T), _lib.stream_ptr()), "eyoc_irls_quad")
    return T.to(src_dev)


estimate_transform = est_quad_linear_robust


def _segments(seg, rows, who):
    """A segment list -> (the C array the library takes, the ints); it must describe ``rows`` rows."""
    seg = [int(v) for v in seg]
    if len(seg) < 2 or seg[0] != 0 or seg[-1] != rows:
        raise ValueError(f"{who}: segments {seg[:1]}..{seg[-1:]} do not describe {rows} rows")
    return (C.c_int32 * len(seg))(*seg), seg


def est_quad_linear_robust_batched(P0, P1, seg0, seg1=None, idx1=None, weight=None, iters=20):
    """``est_quad_linear_robust`` for every pair of a batch in one call (``eyoc_irls_quad_batched``: one workgroup per pair, one launch
    per 64 pairs, nothing read back) -> ``T f32 [P, 4, 4]`` on the device.

    Pair ``b`` owns rows ``seg0[b]:seg0[b+1]`` of ``P0 [*, 3]`` (and of ``weight [*]``) and rows ``seg1[b]:seg1[b+1]`` of ``P1 [*, 3]``
    (``seg1=None``: the same segments).  ``idx1 int64 [len(P0)]`` - local to the pair's ``P1`` segment, what ``knn1_segmented`` returns -
    makes row ``i`` of a pair the correspondence ``(P0[i], P1[idx1[i]])``; without it row ``i`` pairs with row ``i``.  A pair's pose has
    the bytes ``est_quad_linear_robust`` gives for its gathered arrays alone; an empty pair, or one with an index outside its segment,
    gets a NaN pose."""
    p0 = _cuda_f32(P0).reshape(-1, 3)
    p1 = _cuda_f32(P1, p0.device).reshape(-1, 3)
    s0, seg0 = _segments(seg0, p0.shape[0], "est_quad_linear_robust_batched (seg0)")
    s1, seg1 = _segments(seg0 if seg1 is None else seg1, p1.shape[0], "est_quad_linear_robust_batched (seg1)")
    if len(seg1) != len(seg0):
        raise ValueError("seg0 and seg1 must list the same number of pairs")
    if idx1 is not None:
        idx1 = idx1.to(p0.device, torch.int64).contiguous().reshape(-1)
        if idx1.numel() != p0.shape[0]:
            raise ValueError("idx1 must have one entry per row of P0")
    w = None if weight is None else _cuda_f32(weight, p0.device).reshape(-1)
    if w is not None and w.numel() != p0.shape[0]:
        raise ValueError("weight must have one entry per row of P0")
    P = len(seg0) - 1
    T = torch.empty((P, 4, 4), dtype=torch.float32, device=p0.device)
    with _lib.on_device(p0.device):
        _lib.check(_lib.load().eyoc_irls_quad_batched(_lib.ctx(p0.device.index), _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(idx1), _lib.ptr(w),
                                                      s0, s1, P, int(iters), _lib.ptr(T), _lib.stream_ptr()), "eyoc_irls_quad_batched")
    return T


def rigid_transform_3d(A, B, weights=None, weight_threshold=0):
    """scripts/SC2_PCR/common.py:7-45: ``A,B [bs,n,3]``, ``weights [bs,n]`` -> ``[bs,4,4]`` with ``B ~ R A + t``."""
    src_dev = A.device
    a = _cuda_f32(A)
    b = _cuda_f32(B, a.device)
    if a.dim() != 3 or a.shape != b.shape or a.shape[2] != 3:
        raise ValueError("A and B must both be [bs,n,3]")
    w = None
    if weights is not None:
        if weight_threshold > 0:
            weights[weights < weight_threshold] = 0      # in place, as the reference does (:20)
        w = _cuda_f32(weights, a.device)
    bs, n = a.shape[0], a.shape[1]
    T = torch.empty((bs, 4, 4), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().eyoc_kabsch_batched(_lib.ctx(a.device.index), _lib.ptr(a), _lib.ptr(b), _lib.ptr(w), bs,
                                                   n, _lib.ptr(T), _lib.stream_ptr()), "eyoc_kabsch_batched")
    return T.to(src_dev)


def transform(pts, trans):
    """scripts/SC2_PCR/utils/SE3.py:44-59."""
    if len(pts.shape) == 3:
        return (trans[:, :3, :3] @ pts.permute(0, 2, 1) + trans[:, :3, 3:4]).permute(0, 2, 1)
    return (trans[:3, :3] @ pts.T + trans[:3, 3:4]).T


def integrate_trans(R, t):
    """scripts/SC2_PCR/utils/SE3.py:75-96 (tensor forms)."""
    if len(R.shape) == 3:
        T = torch.eye(4, device=R.device)[None].repeat(R.shape[0], 1, 1)
        T[:, :3, :3] = R
        T[:, :3, 3:4] = t.view([-1, 3, 1])
    else:
        T = torch.eye(4, device=R.device)
        T[:3, :3] = R
        T[:3, 3:4] = t
    return T


def pose_estimation(model, device, xyz0, xyz1, coord0, coord1, feats0, feats1, return_corr=False):
    """util/transform_estimation.py:119-144: two forwards, inner-product arg-max as weight + index,
    IRLS.  The reference materialises the full ``[N0,N1]`` correlation matrix (3.6 GB at 30k voxels);
    it is only returned here when ``return_corr`` asks for it."""
    from .sparse_tensor import SparseTensor
    F0 = model(SparseTensor(feats0.to(device), coordinates=coord0.to(device))).F
    F1 = model(SparseTensor(feats1.to(device), coordinates=coord1.to(device))).F
    if return_corr:                              # the reference's dense form, only on request
        corr = F0.mm(F1.t())
        weight, inds = corr.max(dim=1)
    else:                                        # streaming arg-max of the same inner products (eyoc_dotmax)
        from .eval import dotmax_segmented
        weight, inds = dotmax_segmented(F0, F1, [0, F0.shape[0]], [0, F1.shape[0]])
    weight = weight.unsqueeze(1).cpu()
    xyz1_corr = xyz1[inds.cpu(), :]
    trans = est_quad_linear_robust(xyz0, xyz1_corr, weight)
    if return_corr:
        return trans, weight, corr
    return trans, weight
