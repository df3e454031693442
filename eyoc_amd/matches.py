"""Ground-truth matching indices on the GPU (``eyoc_radius_matches_count`` / ``eyoc_radius_matches_fill``, csrc/icp.hip): the
reference's ``get_matching_indices`` and ``compute_overlap_ratio`` (util/pointcloud.py:42-66) and, for a batch, what the dataset and
``collate_pair_fn`` (lib/data_loaders.py:948-954, :48-72) make of them - the ``correspondences`` tensor that
``contrastive_hardest_negative_loss`` takes as ``positive_pairs``.

For every source point under the pair's pose ALL target points with ``d2 < search_voxel_size ** 2`` are returned as ``(i, j)``, inside
a source row ascending by ``(d2, j)``, cut to the first ``K``; the contract is in ``include/eyoc_hip.h``.  The clouds are handed to
the GPU as float32, like every cloud of this package.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .icp import _clouds, _poses
from .labels import _pack_clouds

BAD_INIT, RANGE = 2, 8      # status bits (EYOC_ICP_BAD_INIT, EYOC_ICP_RANGE)


def _need_gpu(who):
    if not torch.cuda.is_available():
        raise _lib.EyocError(f"no GPU visible: {who} runs on MI355X only (no CPU fallback)")


def _packed(who, pcd0, pcd1, seg0, seg1):
    """Lists of ``[n, 3]`` clouds, or packed ``[N, 3]`` tensors with their segments -> what ``icp._clouds`` returns, plus the segments
    as Python lists."""
    if seg0 is None and seg1 is None and isinstance(pcd0, (list, tuple)):
        pcd0, seg0 = _pack_clouds(pcd0)
        pcd1, seg1 = _pack_clouds(pcd1, pcd0.device)
    elif seg0 is None or seg1 is None:
        raise ValueError(f"{who}: packed clouds need seg0 and seg1")
    s, t, ss, st, P, _ = _clouds(who, pcd0, pcd1, seg0, seg1)
    return s, t, ss, st, P, [int(v) for v in seg0], [int(v) for v in seg1]


class _Search:
    """One call's arguments, its workspace and its count pass; ``fill`` runs on the same workspace."""

    def __init__(self, who, pcd0, pcd1, T, radius, K, seg0, seg1):
        _need_gpu(who)
        self.s, self.t, self.ss, self.st, self.P, self.seg0, self.seg1 = _packed(who, pcd0, pcd1, seg0, seg1)
        dev = self.s.device
        self.T = None if T is None else _poses(T, self.P, dev)
        self.radius, self.K = float(radius), 0 if K is None else int(K)
        if self.K < 0:
            raise ValueError(f"{who}: K = {K} is negative")
        self.offsets = torch.empty(self.s.shape[0] + 1, dtype=torch.int64, device=dev)
        self.status = torch.empty(self.P, dtype=torch.int32, device=dev)
        lib = _lib.load()
        with _lib.on_device(dev):
            # the grids live in the workspace from the count to the fill: nothing else may ask for this stream's scratch in between
            self.ws = _lib.scratch(lib.eyoc_radius_matches_workspace_bytes(self.P, self.s.shape[0], self.t.shape[0]), dev)
            _lib.check(lib.eyoc_radius_matches_count(*self._args(), _lib.ptr(self.offsets), _lib.ptr(self.status), _lib.ptr(self.ws),
                                                     self.ws.numel(), _lib.stream_ptr()), "eyoc_radius_matches_count")

    def _args(self):
        return (_lib.ctx(self.s.device.index), _lib.ptr(self.s), _lib.ptr(self.t), self.ss, self.st, self.P, _lib.ptr(self.T), self.radius,
                self.K)

    def fill(self, total):
        dev = self.s.device
        pairs = torch.empty((total, 2), dtype=torch.int64, device=dev)
        d2 = torch.empty(total, dtype=torch.float64, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.load().eyoc_radius_matches_fill(*self._args(), _lib.ptr(self.offsets), _lib.ptr(self.status), total,
                                                            _lib.ptr(pairs), _lib.ptr(d2), _lib.ptr(self.ws), self.ws.numel(),
                                                            _lib.stream_ptr()), "eyoc_radius_matches_fill")
        return pairs, d2

    def pair_offsets(self):
        """``int64 [P + 1]`` on the device: where every pair's slice of the result starts."""
        return self.offsets[torch.tensor(self.seg0, dtype=torch.int64).to(self.s.device, non_blocking=True)]


def matching_indices_batched(pcd0, pcd1, T=None, search_voxel_size=0.45, K=None, collated=True, seg0=None, seg1=None, return_d2=False):
    """``get_matching_indices`` for every pair of a batch and the collation of ``collate_pair_fn``, on the device.

    ``pcd0 / pcd1``: lists of ``[n, 3]`` clouds (numpy or torch), or packed ``[N, 3]`` tensors with the host offsets ``seg0 / seg1``;
    ``T``: ``[P, 4, 4]`` (host or device, any float type; ``None`` = the identity, the base stage); ``K``: at most that many matches per
    source point, the nearest first (``None`` = all).  One count pass, ONE read-back (the number of matches), one allocation, one fill
    pass.  Returns ``(correspondences int64 [M, 2], seg_m int64 [P + 1], status int32 [P])`` on the device: pair ``b`` owns rows
    ``seg_m[b]:seg_m[b+1]``, ordered by source row, inside a source row by ``(d2, target row)``.  ``collated=True`` shifts the rows by the
    running cloud sizes, exactly as ``collate_pair_fn`` does (``False``: rows local to the pair).  A pair without matches - or with a status:
    ``BAD_INIT`` for a non-finite pose, ``RANGE`` for a non-finite or far-out point - has an empty slice; whether to drop it, as the
    reference's collate does, is the caller's decision.  ``return_d2`` appends the fp64 squared distances ``[M]``.  The grids live in the
    stream's scratch buffer (``_lib.scratch``: it grows to the largest batch seen, ``_lib.scratch_clear()`` releases it)."""
    q = _Search("matching_indices_batched", pcd0, pcd1, T, search_voxel_size, K, seg0, seg1)
    total = int(q.offsets[-1].item())                                  # the one read-back
    pairs, d2 = q.fill(total)
    seg_m = q.pair_offsets()
    if collated and total and q.P > 1:
        dev = pairs.device
        shift = torch.tensor([q.seg0[:-1], q.seg1[:-1]], dtype=torch.int64).t().contiguous().to(dev, non_blocking=True)
        pairs += torch.repeat_interleave(shift, seg_m[1:] - seg_m[:-1], dim=0, output_size=total)
    return (pairs, seg_m, q.status, d2) if return_d2 else (pairs, seg_m, q.status)


def _points(a):
    a = getattr(a, "points", a)
    return a if isinstance(a, torch.Tensor) else np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1, 3)


def _host_poses(T):
    return np.asarray(T.detach().cpu() if isinstance(T, torch.Tensor) else T, np.float64).reshape(-1, 4, 4)


def get_matching_indices(source, target, trans, search_voxel_size, K=None):
    """util/pointcloud.py:53-66 with the reference's signature: ``source / target`` are ``[n, 3]`` points (numpy, torch, or an
    ``eyoc_amd.o3d`` point cloud), ``trans`` the 4 x 4 pose applied to ``source``.  Returns an ``[m, 2]`` int64 device tensor of
    ``(source row, target row)``; ``.tolist()`` gives the reference's list of pairs."""
    _need_gpu("get_matching_indices")
    return matching_indices_batched([_points(source)], [_points(target)], None if trans is None else _host_poses(trans), search_voxel_size,
                                    K, collated=False)[0]


def _share(q):
    """The share of every pair's source rows that have a match, from a count pass: ``f64 [P]`` (0 / 0 = nan for an empty cloud)."""
    hit = torch.zeros_like(q.offsets)
    torch.cumsum(q.offsets[1:] > q.offsets[:-1], 0, out=hit[1:])
    seg = torch.tensor(q.seg0, dtype=torch.int64).to(hit.device, non_blocking=True)
    return (hit[seg[1:]] - hit[seg[:-1]]).double() / (seg[1:] - seg[:-1]).double()


def _downsampled(who, pcd0, pcd1, seg0, seg1, voxel_size):
    """Both sides of a batch through ``downsample.voxel_down_sample_batched`` -> packed clouds and their segments."""
    from .downsample import voxel_down_sample_batched
    s, t, _, _, _, seg0, seg1 = _packed(who, pcd0, pcd1, seg0, seg1)
    s, seg0, _ = voxel_down_sample_batched(s, seg0, voxel_size)
    t, seg1, _ = voxel_down_sample_batched(t, seg1, voxel_size)
    return s, t, seg0, seg1


def overlap_ratio_batched(pcd0, pcd1, T, voxel_size, seg0=None, seg1=None, downsample=False):
    """``compute_overlap_ratio`` for every pair of a batch -> ``f64 [P]`` on the device.  Both directions with ``K = 1``, the count pass
    only: the share of source rows with at least one match, then the larger of the two directions.  ``downsample=False`` (the default)
    takes the clouds as they are: they must then ALREADY be voxel down-sampled.  ``downsample=True`` does what the reference's function
    does inside (util/pointcloud.py:43-44): both clouds of every pair go through ``downsample.voxel_down_sample_batched`` at
    ``voxel_size`` first (a cloud that call refuses is empty afterwards: its pair's ratio is nan).  The inverse poses are
    ``np.linalg.inv`` on the host, like the reference's."""
    if downsample:
        _need_gpu("overlap_ratio_batched")
        pcd0, pcd1, seg0, seg1 = _downsampled("overlap_ratio_batched", pcd0, pcd1, seg0, seg1, voxel_size)
    fwd = _Search("overlap_ratio_batched", pcd0, pcd1, T, voxel_size, 1, seg0, seg1)
    a = _share(fwd)
    back = _Search("overlap_ratio_batched", fwd.t, fwd.s, None if T is None else np.linalg.inv(_host_poses(T)), voxel_size, 1, fwd.seg1,
                   fwd.seg0)
    return torch.maximum(a, _share(back))


def compute_overlap_ratio(pcd0, pcd1, trans, voxel_size, downsample=False):
    """util/pointcloud.py:42-50: ``max(|matching01| / |pcd0|, |matching10| / |pcd1|)`` with ``K = 1`` and ``trans`` / its inverse.
    ``downsample=False`` (the default): on clouds that are ALREADY voxel down-sampled at ``voxel_size``, no down-sampling happens here;
    ``downsample=True``: both clouds are down-sampled at ``voxel_size`` first, as the reference's function does (:43-44)."""
    _need_gpu("compute_overlap_ratio")
    return float(overlap_ratio_batched([_points(pcd0)], [_points(pcd1)], _host_poses(trans), voxel_size, downsample=downsample)[0].item())
