"""Per-pair failure isolation, the device calls: dropping clouds from a collated batch (``eyoc_batch_drop``) and sending index
arrays through the resulting row map (``eyoc_remap_rows``).  ``harness.DeviceBatch.without_pairs`` is built on them."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_BATCH = 1024          # batch indices of the coordinate keys (include/eyoc_hip.h)


def batch_mask(batches) -> np.ndarray:
    """Batch indices -> the 1024-bit mask (``uint32 [32]``, bit ``b & 31`` of word ``b >> 5``) of ``eyoc_maps_last_fault_batches``."""
    mask = np.zeros(32, np.uint32)
    for b in batches:
        b = int(b)
        if not 0 <= b < MAX_BATCH:
            raise ValueError(f"batch index {b} outside 0 .. {MAX_BATCH - 1}")
        mask[b >> 5] |= np.uint32(1 << (b & 31))
    return mask


def drop_model(coords, feats, mask):
    """What ``batch_drop`` computes, in numpy (host arrays; the tests' model of the kernel): ``(coords[keep], feats[keep] or None,
    row_map int32 [N], kept int32 [1024])``."""
    coords = np.asarray(coords)
    b = coords[:, 0].astype(np.int64)
    inside = (b >= 0) & (b < MAX_BATCH)
    bits = np.unpackbits(np.asarray(mask, np.uint32).view(np.uint8), bitorder="little").astype(bool)
    keep = ~(inside & bits[np.clip(b, 0, MAX_BATCH - 1)])
    row_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    kept = np.bincount(b[keep & inside], minlength=MAX_BATCH).astype(np.int32)
    return coords[keep], None if feats is None else np.asarray(feats)[keep], row_map, kept


def batch_drop(coords: torch.Tensor, feats: torch.Tensor | None, drop_batches):
    """The collated batch ``coords int32 [N,4]`` / ``feats f32 [N,C]`` (or ``None``) without the rows of the batch indices in
    ``drop_batches`` (an iterable of indices, or the ``uint32 [32]`` mask itself): ``(coords', feats', row_map int32 [N], kept
    np.int32 [1024])`` - the kept rows in input order with their batch indices unchanged, old row -> new row (-1: dropped), the kept
    rows per batch index.  On the current stream, which it synchronises once; the inputs are not modified."""
    if not coords.is_cuda:
        raise _lib.EyocError("batch_drop: the batch must live on the GPU (no CPU path)")
    if coords.dim() != 2 or coords.shape[1] != 4 or coords.dtype != torch.int32:
        raise ValueError(f"coords must be int32 [N,4], got {coords.dtype} {tuple(coords.shape)}")
    mask = np.ascontiguousarray(drop_batches, np.uint32) if isinstance(drop_batches, np.ndarray) and drop_batches.dtype == np.uint32 \
        else batch_mask(drop_batches)
    if mask.shape != (32,):
        raise ValueError("a drop mask has 32 words")
    coords = coords.contiguous()
    n = coords.shape[0]
    c = 0
    if feats is not None:
        if feats.dim() != 2 or feats.shape[0] != n or feats.dtype != torch.float32 or feats.device != coords.device:
            raise ValueError("feats must be f32 [N,C] on the device of coords")
        feats = feats.contiguous()
        c = feats.shape[1]
    dev = coords.device
    lib = _lib.load()
    coords_out = torch.empty_like(coords)
    feats_out = None if feats is None else torch.empty_like(feats)
    row_map = torch.empty(n, dtype=torch.int32, device=dev)
    n_kept = C.c_int(0)
    kept = np.zeros(MAX_BATCH, np.int32)
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.eyoc_batch_drop_workspace_bytes(n), dev)
        _lib.check(lib.eyoc_batch_drop(_lib.ctx(dev.index), _lib.ptr(coords), _lib.ptr(feats), n, c, mask.ctypes.data,
                                       _lib.ptr(coords_out), _lib.ptr(feats_out), _lib.ptr(row_map), C.byref(n_kept),
                                       kept.ctypes.data, _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "eyoc_batch_drop")
    m = n_kept.value
    return coords_out[:m], None if feats_out is None else feats_out[:m], row_map, kept


def remap_rows(idx: torch.Tensor, row_map: torch.Tensor) -> torch.Tensor:
    """``row_map[idx]`` as int64 (-1 for an index outside the map) in one launch on the current stream; ``idx`` int64 on the device."""
    if not idx.is_cuda or idx.dtype != torch.int64 or row_map.dtype != torch.int32 or row_map.device != idx.device:
        raise ValueError("remap_rows: idx int64 and row_map int32 on one GPU")
    idx = idx.contiguous()
    out = torch.empty_like(idx)
    with torch.cuda.device(idx.device):
        _lib.check(_lib.load().eyoc_remap_rows(_lib.ctx(idx.device.index), _lib.ptr(idx), idx.numel(), _lib.ptr(row_map.contiguous()),
                                               row_map.numel(), _lib.ptr(out), _lib.stream_ptr()), "eyoc_remap_rows")
    return out
