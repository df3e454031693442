"""Voxelisation and the one-call feature extractor with the reference's names.

``sparse_quantize`` mirrors the way the loaders call ``ME.utils.sparse_quantize(xyz / voxel_size,
return_index=True)`` (lib/data_loaders.py:940-943), ``voxelize`` adds the ``floor(...).int()`` +
ones-feature step of lib/data_loaders.py:969-972, and ``extract_features`` mirrors util/misc.py:21-93.
The hash-grid de-duplication runs in ``libeyoc_hip.so`` (``eyoc_voxelize``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .sparse_tensor import SparseTensor


def sparse_quantize(xyz, voxel_size: float, batch_index: int = 0):
    """First point of every occupied ``voxel_size`` voxel, in input order.

    ``xyz``: ``[N,3]`` (or ``[N,4]`` KITTI xyzr) float32, numpy or torch.  Returns device tensors
    ``(coords int32 [M,4] = (batch, floor(p / voxel)), sel int64 [M])`` with ``sel`` ascending.  A NaN or +-inf in x, y or z fails the
    call with ``EYOC_ERR_RANGE`` (an ``EyocError``), like a point outside the key range."""
    t = xyz if isinstance(xyz, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(xyz, np.float32))
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.EyocError("no GPU visible: the EYOC hot path runs on MI355X only (no CPU fallback)")
        t = t.cuda()
    t = t.to(torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] not in (3, 4):
        raise ValueError("xyz must be [N,3] or [N,4]")
    n = t.shape[0]
    lib = _lib.load()
    sel = torch.empty(max(n, 1), dtype=torch.int32, device=t.device)
    coords = torch.empty((max(n, 1), 4), dtype=torch.int32, device=t.device)
    if n == 0:
        return coords[:0], sel[:0].long()
    n_out = C.c_int(0)
    with torch.cuda.device(t.device):
        ws = _lib.workspace(lib.eyoc_voxelize_workspace_bytes(n), t.device)
        _lib.check(lib.eyoc_voxelize(_lib.ctx(t.device.index), _lib.ptr(t), n, t.shape[1], float(voxel_size), int(batch_index),
                                     _lib.ptr(sel), _lib.ptr(coords), C.byref(n_out), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr()), "eyoc_voxelize")
    m = n_out.value
    return coords[:m], sel[:m].long()


MAX_BATCH = 1024          # batch indices of the coordinate keys (include/eyoc_hip.h)
MAX_POINTS = 1 << 30      # points of one batched call


def _batch_layout(clouds, voxel_size, batch_base):
    """Host-side checks of ``sparse_quantize_batch`` (before anything touches the device) -> (row width, point offsets int64 [B+1])."""
    B = len(clouds)
    if B == 0:
        raise ValueError("sparse_quantize_batch: no clouds")
    if not float(voxel_size) > 0.0:
        raise ValueError(f"sparse_quantize_batch: voxel_size must be > 0, got {voxel_size}")
    if int(batch_base) < 0 or int(batch_base) + B > MAX_BATCH:
        raise ValueError(f"sparse_quantize_batch: batch indices {batch_base} .. {int(batch_base) + B - 1} outside 0 .. {MAX_BATCH - 1}")
    shapes = [tuple(c.shape) for c in clouds]
    if any(len(s) != 2 or s[1] not in (3, 4) for s in shapes):
        raise ValueError("sparse_quantize_batch: every cloud must be [N,3] or [N,4]")
    widths = {s[1] for s in shapes}
    if len(widths) != 1:
        raise ValueError(f"sparse_quantize_batch: mixed row widths {sorted(widths)} (all [N,3] or all [N,4])")
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum([s[0] for s in shapes], out=offsets[1:])
    if offsets[-1] > MAX_POINTS:
        raise ValueError(f"sparse_quantize_batch: {offsets[-1]} points in all (at most 2^30 per call)")
    return widths.pop(), offsets


def sparse_quantize_batch(clouds, voxel_size: float, batch_base: int = 0, device=None, isolate: bool = False):
    """``sparse_quantize`` of B raw clouds and their ``sparse_collate`` in one call with one stream synchronisation
    (lib/data_loaders.py:940-943,969-979 per cloud, then :31-85).

    ``clouds``: ``[N_b,3]`` or ``[N_b,4]`` float32 arrays (numpy or torch, host or device; one width for all, empty clouds allowed).
    Host clouds are packed into one pinned buffer and uploaded with one copy.  ``device``: where host-only input goes (default: the
    current device).  Returns device tensors ``(coords int32 [M,4] = (batch_base + b, floor(p / voxel)), sel int64 [M] = index of the
    kept point within its cloud, xyz f32 [M,3] = the kept points)`` and the clouds' row ranges ``offsets np.int64 [B+1]`` - bit for bit
    the concatenation of ``sparse_quantize(clouds[b], voxel_size, batch_base + b)``.

    ``isolate=True`` (``eyoc_voxelize_batched_isolating``): a point outside the key range or with a NaN / inf coordinate no longer fails
    the call; a fifth value comes back, ``faults np.int32 [B,2]`` = per cloud the finite points out of range and the non-finite points,
    and a cloud with a count has an empty row range.  The other clouds' rows are those of the plain call."""
    clouds = list(clouds)
    width, pt_off = _batch_layout(clouds, voxel_size, batch_base)
    B, n = len(clouds), int(pt_off[-1])
    if not torch.cuda.is_available():
        raise _lib.EyocError("no GPU visible: the EYOC hot path runs on MI355X only (no CPU fallback)")
    on_dev = [c for c in clouds if isinstance(c, torch.Tensor) and c.is_cuda]
    dev = torch.device(device) if device is not None else on_dev[0].device if on_dev else torch.device("cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    faults = np.zeros((B, 2), np.int32)
    if n == 0:
        empty = (torch.empty((0, 4), dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                 torch.empty((0, 3), dtype=torch.float32, device=dev), np.zeros(B + 1, np.int64))
        return empty + (faults,) if isolate else empty
    lib = _lib.load()
    vox_off = np.zeros(B + 1, np.int64)
    i64 = C.POINTER(C.c_int64)
    with torch.cuda.device(dev):
        if on_dev:
            packed = torch.cat([(c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, np.float32)))
                                .to(dev, torch.float32) for c in clouds], 0).contiguous()
        else:
            host = torch.empty((n, width), dtype=torch.float32, pin_memory=True)
            h = host.numpy()
            for b, c in enumerate(clouds):
                h[pt_off[b]:pt_off[b + 1]] = c.detach().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
            packed = host.to(dev, non_blocking=True)   # on the library's stream, which the call synchronises
        sel = torch.empty(n, dtype=torch.int32, device=dev)
        coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
        xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
        args = (_lib.ptr(packed), width, pt_off.ctypes.data_as(i64), B, n, float(voxel_size), int(batch_base), _lib.ptr(sel),
                _lib.ptr(coords), _lib.ptr(xyz), vox_off.ctypes.data_as(i64))
        if isolate:
            ws = _lib.workspace(lib.eyoc_voxelize_batched_isolating_workspace_bytes(n, B), dev)
            _lib.check(lib.eyoc_voxelize_batched_isolating(_lib.ctx(dev.index), *args, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(),
                                                           faults.ctypes.data), "eyoc_voxelize_batched_isolating")
        else:
            ws = _lib.workspace(lib.eyoc_voxelize_batched_workspace_bytes(n, B), dev)
            _lib.check(lib.eyoc_voxelize_batched(_lib.ctx(dev.index), *args, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "eyoc_voxelize_batched")
    m = int(vox_off[-1])
    out = coords[:m], sel[:m].long(), xyz[:m], vox_off
    return out + (faults,) if isolate else out


def voxelize(xyz, voxel_size: float, batch_index: int = 0):
    """``(xyz[sel], coords, feats = ones [M,1])`` - the per-cloud part of lib/data_loaders.py:936-979."""
    t = xyz if isinstance(xyz, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(xyz, np.float32))
    coords, sel = sparse_quantize(t, voxel_size, batch_index)
    pts = t.to(coords.device)[sel][:, :3]
    return pts, coords, torch.ones((len(sel), 1), dtype=torch.float32, device=coords.device)


def _optional_channels(name, arr, n_points, upper):
    """One optional per-point attribute of ``extract_features``: ``None`` or a ``[n_points, 3]`` array with no value
    above ``upper`` (the reference refuses colours / normals above 1, util/misc.py:47-57)."""
    if arr is None:
        return None
    a = np.asarray(arr)
    if a.ndim != 2 or a.shape != (n_points, 3):
        raise AssertionError(f"{name} must be [{n_points}, 3], got {tuple(a.shape)}")
    if bool(np.any(a > upper)):              # the reference's own test (np.any(rgb > 1)); any dtype, empty arrays included
        raise ValueError("Invalid color. Color must range from [0, 1]" if name == "rgb"
                         else "Invalid normal. Normal must range from [-1, 1]")
    return a


def extract_features(model, xyz, rgb=None, normal=None, voxel_size=0.05, device=None, skip_check=False, is_eval=True):
    """Voxelise one cloud, run ``model`` on it and return ``(xyz of the kept points, their features)`` - the one-call API
    of util/misc.py:21-93.  Input channels, in the reference's order: colour shifted to [-0.5, 0.5], normal halved, or a
    single column of ones when neither is given.  The de-duplication runs on the GPU first; only the kept rows of the
    attributes are shifted / scaled and uploaded."""
    if is_eval:
        model.eval()
    pts = np.asarray(xyz)
    if not skip_check:
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise AssertionError(f"xyz must be [N, 3], got {tuple(pts.shape)}")
        rgb = _optional_channels("rgb", rgb, len(pts), 1.0)
        normal = _optional_channels("normal", normal, len(pts), 1.0)
    dev = torch.device("cuda:0") if device is None else torch.device(device)
    coords, kept = sparse_quantize(torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(dev), voxel_size)
    kept_host = kept.cpu().numpy()
    # arithmetic in the attribute's own dtype, then ONE rounding to fp32 (what `torch.tensor(rgb - 0.5, float32)` does)
    columns = [torch.as_tensor(np.asarray(a)[kept_host] * scale + shift, dtype=torch.float32, device=dev)
               for a, scale, shift in ((rgb, 1.0, -0.5), (normal, 0.5, 0.0)) if a is not None]
    feats = torch.cat(columns, dim=1) if columns else torch.ones((len(kept_host), 1), dtype=torch.float32, device=dev)
    return pts[kept_host], model(SparseTensor(feats, coordinates=coords)).F
