"""Centroid voxel down-sampling on the device (``eyoc_voxel_downsample_batched``, ``csrc/downsample.hip``): Open3D's
``pcd.voxel_down_sample(voxel_size)`` as the reference calls it (``util/pointcloud.py:38,43-44``) for a batch of clouds in one call.

Not the voxeliser of ``eyoc_amd.voxelize`` (MinkowskiEngine's ``sparse_quantize``: the first point of a voxel, grid anchored at the
origin): here a voxel's row is the MEAN of its points, on a grid anchored half a voxel below the cloud's minimum corner, summed in fp64
in ascending point order; the contract is in ``include/eyoc_hip.h`` and restated in ``tests/downsample_restatement.py``.  Opt-in:
``o3d.PointCloud.voxel_down_sample`` and the ``downsample=True`` switches of ``matches`` and ``fpfh`` are its only callers."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import icp as _icp
from .eval import _cuda_f32

MAX_CLOUDS = 1024
MAX_ATTR = 8
STAGES = ("bounds", "keys", "sort", "heads", "scan", "rows", "sums")     # eyoc_voxel_downsample_batched_timed's stage_ms


def _rows_cols(a):
    shape = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
    if len(shape) != 2:
        raise ValueError(f"voxel_down_sample_batched: expected a 2-D array, got shape {shape}")
    return int(shape[0]), int(shape[1])


def _validate(pts, seg, voxel_size, attrs):
    """Everything that can be refused without a GPU -> ``(seg list, n, stride, n_attr)``."""
    n, stride = _rows_cols(pts)
    if stride not in (3, 4):
        raise ValueError(f"voxel_down_sample_batched: points must be [N, 3] or [N, 4], got [{n}, {stride}]")
    seg_l = [int(v) for v in seg]
    B = len(seg_l) - 1
    if B < 1 or seg_l[0] != 0 or seg_l[-1] != n or any(seg_l[b + 1] < seg_l[b] for b in range(B)):
        raise ValueError("voxel_down_sample_batched: the segments do not describe the clouds")
    if B > MAX_CLOUDS:
        raise ValueError(f"voxel_down_sample_batched: {B} clouds (at most {MAX_CLOUDS} per call)")
    v = float(voxel_size)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"voxel_down_sample_batched: voxel_size = {voxel_size!r} must be positive and finite")
    n_attr = 0
    if attrs is not None:
        rows, n_attr = _rows_cols(attrs)
        if rows != n:
            raise ValueError(f"voxel_down_sample_batched: {rows} attribute rows for {n} points")
        if n_attr > MAX_ATTR:
            raise ValueError(f"voxel_down_sample_batched: {n_attr} attribute columns (at most {MAX_ATTR})")
    return seg_l, n, stride, n_attr


def voxel_down_sample_batched(pts, seg, voxel_size, attrs=None, return_trace=False, return_stage_ms=False):
    """``pts f32 [N, 3]`` (or ``[N, 4]``: the fourth column is never read) holds the clouds back to back, cloud ``b`` = rows
    ``seg[b]:seg[b+1]``; ``attrs f32 [N, c]``, ``c <= 8``: per-point columns averaged like the coordinates.  Returns
    ``(xyz f32 [M, 3], seg_out, status int32 [B])`` - cloud ``b`` owns output rows ``seg_out[b]:seg_out[b+1]`` (a host list), one row per
    occupied voxel in ascending order of the voxel's lowest point index, each the fp64 mean of the voxel's points rounded once;
    ``status[b] = icp.RANGE`` for a cloud with a non-finite point or an extent beyond 2^17 cells (it has no rows).  With ``attrs`` the
    averaged ``attrs_out f32 [M, c]`` is appended, with ``return_trace`` the tuple ``(first int32 [M], count int32 [M], inverse int32
    [N])``: the lowest point index of every row within its cloud, its number of points, and the row - within the cloud's range - every
    point went into (-1 in a refused cloud).  Everything but ``seg_out`` stays on the device; one stream synchronisation.
    ``return_stage_ms`` (diagnostics) appends the per-stage milliseconds of ``STAGES``.

    Raises ``ValueError`` before anything touches a GPU for segments that do not describe ``pts``, a ``voxel_size`` that is not positive
    and finite, an ``attrs`` row count that differs, more than 8 attribute columns or more than 1024 clouds."""
    seg_l, n, stride, n_attr = _validate(pts, seg, voxel_size, attrs)
    B = len(seg_l) - 1
    p = _cuda_f32(pts)
    a = _cuda_f32(attrs, p.device) if n_attr else None
    dev = p.device
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    a_out = torch.empty((n, n_attr), dtype=torch.float32, device=dev) if n_attr else None
    first = torch.empty(n, dtype=torch.int32, device=dev) if return_trace else None
    count = torch.empty(n, dtype=torch.int32, device=dev) if return_trace else None
    inverse = torch.empty(n, dtype=torch.int32, device=dev) if return_trace else None
    status = torch.zeros(B, dtype=torch.int32, device=dev)          # n = 0 writes nothing: every cloud is empty, status 0
    pt_off, vox_off = np.asarray(seg_l, np.int64), np.zeros(B + 1, np.int64)
    i64 = C.POINTER(C.c_int64)
    stage_ms = (C.c_float * len(STAGES))()
    lib = _lib.load()
    with _lib.on_device(dev):
        ws = _lib.workspace(lib.eyoc_voxel_downsample_workspace_bytes(n, B, n_attr), dev)
        args = (_lib.ctx(dev.index), _lib.ptr(p), stride, pt_off.ctypes.data_as(i64), B, n, float(voxel_size), _lib.ptr(a), n_attr,
                _lib.ptr(xyz), _lib.ptr(a_out), _lib.ptr(first), _lib.ptr(count), _lib.ptr(inverse), _lib.ptr(status),
                vox_off.ctypes.data_as(i64), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        if return_stage_ms:
            _lib.check(lib.eyoc_voxel_downsample_batched_timed(*args, stage_ms), "eyoc_voxel_downsample_batched_timed")
        else:
            _lib.check(lib.eyoc_voxel_downsample_batched(*args), "eyoc_voxel_downsample_batched")
    m = int(vox_off[-1])
    out = (xyz[:m], [int(v) for v in vox_off], status)
    if n_attr:
        out += (a_out[:m],)
    if return_trace:
        out += ((first[:m], count[:m], inverse),)
    if return_stage_ms:
        out += (dict(zip(STAGES, (float(v) for v in stage_ms))),)
    return out


def voxel_down_sample(points, voxel_size):
    """One cloud: ``[n, 3]`` points (numpy, torch, or anything with a ``points`` attribute) -> ``f32 [m, 3]`` on the device.  Raises
    ``EyocError(ERR_RANGE)`` for a cloud the grid cannot hold (a non-finite point, more than 2^17 cells on an axis), like
    ``fpfh.compute_fpfh_feature``."""
    p = _icp._points(points)
    if p.dim() != 2:
        p = p.reshape(-1, 3)
    _validate(p, [0, p.shape[0]], voxel_size, None)
    if not torch.cuda.is_available():
        raise _lib.EyocError("no GPU visible: voxel_down_sample runs on MI355X only (no CPU fallback)")
    xyz, _, status = voxel_down_sample_batched(p, [0, p.shape[0]], voxel_size)
    if int(status[0]) != 0:
        raise _lib.EyocError("voxel_down_sample: a point is not finite or the cloud spans more than 2^17 cells on an axis", _lib.ERR_RANGE)
    return xyz
