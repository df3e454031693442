"""Training batches from raw scans: the reference's ``PairDataset.__getitem__`` + ``collate_pair_fn`` (lib/data_loaders.py:892-979,
:31-85) for ``P`` pairs in one device pass - ``eyoc_cloud_centroids``, ``eyoc_augment_poses``, ``eyoc_voxelize_batched_posed``
(csrc/augment.hip, csrc/coordmap.hip), then ``matching_indices_batched`` for the positives.

The reference centres and rotates every cloud with an fp64 pose (``sample_random_trans``, :93-100), optionally scales it (:927-933),
divides by the voxel size and floors in fp64 (:940-943, :969-970), casts the kept points to fp32 (:978), and searches the positives under
``T1 @ M2 @ inv(T0)`` (:917, :948-954).  The expressions and their association order are in ``include/eyoc_hip.h``.  Two stated
deviations: the centroid is an fp64 mean (the reference's ``np.mean`` of an fp32 array accumulates in fp32; the same ``T0 / T1`` move the
points and form ``T_gt``, so the batch is self-consistent), and the matches are decided on the fp32 kept points the batch carries
(Open3D searches their fp64 originals, so a pair within fp32 rounding of the radius can differ).
"""
from __future__ import annotations

import ctypes as C
import random as _random

import numpy as np
import torch

from . import _lib
from .matches import matching_indices_batched
from .sparse_tensor import SparseTensor
from .voxelize import _batch_layout, sparse_quantize_batch


def rodrigues(axis, theta):
    """Rotation by ``theta`` (rad) about ``axis`` (normalised here), fp64 ``[3,3]`` - the reference's
    ``expm(np.cross(np.eye(3), axis / norm(axis) * theta))`` (lib/data_loaders.py:89-90) in closed form."""
    a0, a1, a2 = (float(v) for v in axis)
    nrm = np.sqrt((a0 * a0 + a1 * a1) + a2 * a2)
    x, y, z = a0 / nrm, a1 / nrm, a2 / nrm
    c, s = np.cos(float(theta)), np.sin(float(theta))
    t = 1.0 - c
    return np.array([[c + x * x * t, x * y * t - z * s, x * z * t + y * s],
                     [y * x * t + z * s, c + y * y * t, y * z * t - x * s],
                     [z * x * t - y * s, z * y * t + x * s, c + z * z * t]], np.float64)


def draw_augmentation(randg, n_pairs, rotation_range=360, random_rotation=True, random_scale=False, min_scale=0.8, max_scale=1.2,
                      pyrandom=None):
    """The random draws of ``__getitem__`` for ``n_pairs`` consecutive items -> ``(R f64 [2P,3,3], scale f64 [P])`` on the host.

    In the reference's order, per pair: cloud 0 ``randg.rand(3)`` (axis ``- 0.5``, normalised) then ``randg.rand(1)`` (angle =
    ``rotation_range * pi / 180 * (u - 0.5)``), cloud 1 the same two draws (``sample_random_trans``, lib/data_loaders.py:93-100), then
    ``pyrandom.random() < 0.95`` and, if true, a second ``pyrandom.random()`` for the scale (:927-929).  ``rotation_range`` keeps the
    reference's unit (degrees) even where its callers pass ``np.pi / 4`` (:915): that is what it trains with.  ``randg``: a
    ``np.random.RandomState``; ``pyrandom``: an object with ``random()`` (default: the ``random`` module, as in the reference).
    Without ``random_rotation`` / ``random_scale`` nothing is drawn from the respective generator and ``R`` = identity / ``scale`` = 1."""
    P = int(n_pairs)
    R = np.tile(np.eye(3), (2 * P, 1, 1))
    scale = np.ones(P, np.float64)
    pyrandom = _random if pyrandom is None else pyrandom
    for b in range(P):
        if random_rotation:
            for i in (0, 1):
                axis = randg.rand(3) - 0.5
                theta = rotation_range * np.pi / 180.0 * (randg.rand(1) - 0.5)
                R[2 * b + i] = rodrigues(axis, theta[0])
        if random_scale and pyrandom.random() < 0.95:
            scale[b] = min_scale + (max_scale - min_scale) * pyrandom.random()
    return R, scale


def _device_of(clouds, device):
    on_dev = [c for c in clouds if isinstance(c, torch.Tensor) and c.is_cuda]
    dev = torch.device(device) if device is not None else on_dev[0].device if on_dev else torch.device("cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev, bool(on_dev)


def _upload_clouds(clouds, width, pt_off, dev, any_on_dev):
    """Host clouds through ONE pinned buffer and one copy (on the library's stream), device clouds as they are - the packing of
    ``sparse_quantize_batch``."""
    n = int(pt_off[-1])
    if any_on_dev:
        return torch.cat([(c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, np.float32)))
                          .to(dev, torch.float32) for c in clouds], 0).contiguous()
    host = torch.empty((n, width), dtype=torch.float32, pin_memory=True)
    h = host.numpy()
    for b, c in enumerate(clouds):
        h[pt_off[b]:pt_off[b + 1]] = c.detach().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
    return host.to(dev, non_blocking=True)


def cloud_centroids(packed, pt_off):
    """``eyoc_cloud_centroids``: ``packed`` f32 ``[N, 3 | 4]`` on the device, host offsets ``int64 [B+1]`` -> f64 ``[B,4]`` = (fp64 mean of
    x, y, z, count) on the device; an empty cloud gives zeros.  Stream-ordered, nothing is read back."""
    pt_off = np.ascontiguousarray(pt_off, np.int64)
    B, n = len(pt_off) - 1, int(pt_off[-1])
    lib, dev = _lib.load(), packed.device
    out = torch.empty((B, 4), dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        ws = _lib.workspace(lib.eyoc_cloud_centroids_workspace_bytes(n, B), dev)
        _lib.check(lib.eyoc_cloud_centroids(_lib.ctx(dev.index), _lib.ptr(packed), packed.shape[1], pt_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                            B, n, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "eyoc_cloud_centroids")
    return out


def augment_poses(rot, centroids, scale, M2):
    """``eyoc_augment_poses``: device f64 ``rot [2P,3,3]``, ``centroids [2P,4]``, ``scale [P]`` or ``None``, ``M2 [P,4,4]`` ->
    ``(pose [2P,4,4], T_gt [P,4,4])`` f64 on the device: ``T_c = [R_c | R_c (-mean_c)]`` and ``T_1 M2 inv(T_0)`` with its translation
    times the pair's scale."""
    P, dev = M2.shape[0], M2.device
    pose = torch.empty((2 * P, 4, 4), dtype=torch.float64, device=dev)
    T_gt = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.load().eyoc_augment_poses(_lib.ctx(dev.index), _lib.ptr(rot), _lib.ptr(centroids), _lib.ptr(scale), _lib.ptr(M2), P,
                                                  _lib.ptr(pose), _lib.ptr(T_gt), _lib.stream_ptr()), "eyoc_augment_poses")
    return pose, T_gt


def voxelize_posed(packed, pt_off, pose, scale, voxel_size, batch_base=0, isolate=False):
    """``eyoc_voxelize_batched_posed``: the clouds of ``packed`` (device f32 ``[N, 3 | 4]``, host offsets ``pt_off``) under ``pose`` (device
    f64 ``[B,4,4]``) and ``scale`` (device f64 ``[B]`` or ``None``) -> what ``sparse_quantize_batch`` returns: ``(coords int32 [M,4], sel
    int64 [M], xyz f32 [M,3] = float32 of the posed, scaled points, offsets np.int64 [B+1])`` and, with ``isolate``, ``faults np.int32
    [B,2]``.  One stream synchronisation."""
    pt_off = np.ascontiguousarray(pt_off, np.int64)
    B, n = len(pt_off) - 1, int(pt_off[-1])
    lib, dev = _lib.load(), packed.device
    i64 = C.POINTER(C.c_int64)
    vox_off = np.zeros(B + 1, np.int64)
    faults = np.zeros((B, 2), np.int32)
    sel = torch.empty(n, dtype=torch.int32, device=dev)
    coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        ws = _lib.workspace(lib.eyoc_voxelize_batched_posed_workspace_bytes(n, B), dev)
        _lib.check(lib.eyoc_voxelize_batched_posed(_lib.ctx(dev.index), _lib.ptr(packed), packed.shape[1], pt_off.ctypes.data_as(i64), B, n,
                                                   _lib.ptr(pose), _lib.ptr(scale), float(voxel_size), int(batch_base), _lib.ptr(sel),
                                                   _lib.ptr(coords), _lib.ptr(xyz), vox_off.ctypes.data_as(i64), _lib.ptr(ws), ws.numel(),
                                                   _lib.stream_ptr(), faults.ctypes.data if isolate else None),
                   "eyoc_voxelize_batched_posed")
    m = int(vox_off[-1])
    out = coords[:m], sel[:m].long(), xyz[:m], vox_off
    return out + (faults,) if isolate else out


class TrainBatch:
    """What ``collate_pair_fn`` returns for ``P`` pairs, resident on the device.

    ``pcd0 / pcd1``: per-pair views of the kept fp32 points; ``sinput0_C / sinput1_C``: the two collated coordinate sets int32 ``[N,4]``
    with batch index ``b``; ``sinput0_F / sinput1_F``: ones ``[N,1]``; ``sinput0 / sinput1``: ``SparseTensor``s ready for
    ``forward_train`` (built on first use); ``correspondences`` int64 ``[M,2]``, collated, and ``seg_m`` int64 ``[P+1]`` (pair ``b`` owns
    rows ``seg_m[b]:seg_m[b+1]``); ``T_gt`` fp32 ``[P,4,4]`` as ``collate_pair_fn`` casts it and ``T_gt64``; ``len_batch`` ``[[N0, N1]]``
    per pair; ``seg0 / seg1``: the clouds' row offsets (host); ``frame_distance``; ``valid`` bool ``[P]`` on the device: False for a pair
    without matches (``labels != "none"``) or with a fault; ``faults`` np.int32 ``[2P,2]`` (``isolate``) or ``None``; ``R / scale``: the
    draws; ``pose`` f64 ``[2P,4,4]`` and ``centroids`` f64 ``[2P,4]`` on the device (``None`` without augmentation)."""

    @classmethod
    def from_scans(cls, scans0, scans1, M2, voxel_size, labels="gt", search_voxel_size=None, randg=None, random_rotation=True,
                   random_scale=False, rotation_range=360, min_scale=0.8, max_scale=1.2, pyrandom=None, frame_distance=None, isolate=False,
                   device=None):
        """``scans0[b] / scans1[b]``: the raw ``[N,3]`` / ``[N,4]`` float32 clouds of pair ``b`` (numpy or torch; host clouds go through
        one pinned buffer and one upload, device clouds are taken as they are), ``M2``: ``[P,4,4]`` their relative poses
        (``inv(pos_1) @ pos_0``, lib/data_loaders.py:909).  ``labels``: ``"gt"`` - positives under ``T_gt`` (supervised / validation, :954),
        ``"identity"`` - under the identity (base stage, :950), ``"none"`` - extension-mode training: an empty correspondence tensor
        where the reference puts its dummy ``zeros((1, 2))`` (:957).  ``search_voxel_size``: the search radius (default ``1.5 *
        voxel_size``, the reference's multiplier).  ``randg / pyrandom / rotation_range / min_scale / max_scale``: see
        ``draw_augmentation`` (``randg`` defaults to a fresh ``np.random.RandomState()``).  ``isolate``: a cloud with a posed point
        outside the key range or a non-finite one gets an empty row range and its pair ``valid = False`` instead of an error.

        One device pass: centroids, poses, one posed voxelisation of the ``2P`` clouds (pair ``b`` = clouds ``2b``, ``2b + 1``), a split
        into the two coordinate sets, the radius search on the kept fp32 points with ``T_gt`` as it lies on the device.  HOST
        SYNCHRONISATIONS per batch: ONE (the voxeliser's) with ``labels="none"``, otherwise TWO (the voxeliser's and the match count);
        neither the centroids nor the poses come to the host.  ``as_input_dict()`` reads ``valid`` back (one more).  With
        ``random_scale`` the radius differs per pair (:930): one search call - and its read-backs - per distinct radius.

        ``random_rotation=False`` without scaling: the reference's points stay fp32, so this routes to ``sparse_quantize_batch`` and
        returns its bytes, with ``T_gt = M2``.  Scaling without rotation (fp32 points times a Python float) is not provided.
        Substituting another pair for one without overlap (:958-961) is the dataset's business; ``valid`` is what it needs."""
        if labels not in ("gt", "identity", "none"):
            raise ValueError(f"TrainBatch.from_scans: labels = {labels!r} (\"gt\", \"identity\" or \"none\")")
        P = len(scans0)
        M2 = np.ascontiguousarray(np.asarray(M2.detach().cpu() if isinstance(M2, torch.Tensor) else M2, np.float64)).reshape(-1, 4, 4)
        if P == 0 or len(scans1) != P or len(M2) != P:
            raise ValueError(f"TrainBatch.from_scans: {P} / {len(scans1)} scans, {len(M2)} poses")
        if random_scale and not random_rotation:
            raise ValueError("TrainBatch.from_scans: random_scale needs random_rotation (fp32 points times a scale are not provided)")
        if not torch.cuda.is_available():
            raise _lib.EyocError("no GPU visible: TrainBatch.from_scans runs on MI355X only (no CPU fallback)")
        clouds = [c for pair in zip(scans0, scans1) for c in pair]
        dev, any_on_dev = _device_of(clouds, device)
        self = cls.__new__(cls)
        self.P, self.labels, self.voxel_size = P, labels, float(voxel_size)
        self.frame_distance = tuple(frame_distance) if frame_distance is not None else (None,) * P
        self.R, self.scale = draw_augmentation(randg if randg is not None or not random_rotation else np.random.RandomState(), P,
                                               rotation_range, random_rotation, random_scale, min_scale, max_scale, pyrandom)
        self.pose = self.centroids = self.faults = None
        if not random_rotation:
            coords, _, xyz, offsets, *faults = sparse_quantize_batch(clouds, voxel_size, 0, device=dev, isolate=bool(isolate))
            with torch.cuda.device(dev):
                self.T_gt64 = torch.from_numpy(M2).pin_memory().to(dev, non_blocking=True)
        else:
            width, pt_off = _batch_layout(clouds, voxel_size, 0)
            if 2 * P > 1024:
                raise ValueError(f"TrainBatch.from_scans: {P} pairs (at most 512)")
            with torch.cuda.device(dev):
                packed = _upload_clouds(clouds, width, pt_off, dev, any_on_dev)
                # the draws and the odometry: one pinned buffer, one copy
                host = torch.empty(18 * P + 3 * P + 16 * P, dtype=torch.float64, pin_memory=True)
                h = host.numpy()
                h[:18 * P] = self.R.ravel()
                h[18 * P:19 * P] = self.scale
                h[19 * P:21 * P] = np.repeat(self.scale, 2)
                h[21 * P:] = M2.ravel()
                par = host.to(dev, non_blocking=True)
                rot, sc_pair, sc_cloud, M2_dev = par[:18 * P], par[18 * P:19 * P], par[19 * P:21 * P], par[21 * P:].view(P, 4, 4)
                if not random_scale:
                    sc_pair = sc_cloud = None
                self.centroids = cloud_centroids(packed, pt_off)
                self.pose, self.T_gt64 = augment_poses(rot, self.centroids, sc_pair, M2_dev)
                if int(pt_off[-1]) == 0:
                    coords, xyz = torch.empty((0, 4), dtype=torch.int32, device=dev), torch.empty((0, 3), dtype=torch.float32, device=dev)
                    offsets, faults = np.zeros(2 * P + 1, np.int64), [np.zeros((2 * P, 2), np.int32)] * bool(isolate)
                else:
                    coords, _, xyz, offsets, *faults = voxelize_posed(packed, pt_off, self.pose, sc_cloud, voxel_size, 0, bool(isolate))
        if isolate:
            self.faults = faults[0]
        with torch.cuda.device(dev):
            self._split(coords, xyz, offsets, dev)
            self.T_gt = self.T_gt64.float()
            ok = np.ones(P, bool) if self.faults is None else ~(self.faults.reshape(P, 4) != 0).any(1)
            ok_dev = torch.from_numpy(ok).to(dev, non_blocking=True)
            radius = 1.5 * float(voxel_size) if search_voxel_size is None else float(search_voxel_size)
            if labels == "none":
                self.correspondences = torch.empty((0, 2), dtype=torch.int64, device=dev)
                self.seg_m = torch.zeros(P + 1, dtype=torch.int64, device=dev)
                self.valid = ok_dev
            else:
                self._match(None if labels == "identity" else self.T_gt64, radius * self.scale)
                self.valid = (self.seg_m[1:] > self.seg_m[:-1]) & ok_dev
        self._sinput = [None, None]
        return self

    def _split(self, coords, xyz, offsets, dev):
        """The rows of the ``2P`` voxelised clouds -> the two collated sets (rows of cloud ``2b + i`` go to set ``i`` with batch index
        ``b``); the row lists come from the offsets the voxeliser returned, nothing is read back."""
        P = self.P
        sizes = np.diff(offsets)
        self.seg0 = np.concatenate([[0], np.cumsum(sizes[0::2])]).astype(np.int64)
        self.seg1 = np.concatenate([[0], np.cumsum(sizes[1::2])]).astype(np.int64)
        self.len_batch = [[int(sizes[2 * b]), int(sizes[2 * b + 1])] for b in range(P)]
        C_, X = [], []
        for i in (0, 1):
            rows = np.concatenate([np.zeros(0, np.int64)] + [np.arange(offsets[2 * b + i], offsets[2 * b + i + 1], dtype=np.int64)
                                                              for b in range(P)])
            idx = torch.from_numpy(rows).to(dev, non_blocking=True)
            c = coords.index_select(0, idx)
            c[:, 0] >>= 1
            C_.append(c)
            X.append(xyz.index_select(0, idx))
        self.sinput0_C, self.sinput1_C = C_
        self.xyz0, self.xyz1 = X                      # packed [N,3]; pcd0 / pcd1 are views
        self.sinput0_F = torch.ones((len(C_[0]), 1), dtype=torch.float32, device=dev)
        self.sinput1_F = torch.ones((len(C_[1]), 1), dtype=torch.float32, device=dev)
        self.pcd0 = [self.xyz0[self.seg0[b]:self.seg0[b + 1]] for b in range(P)]
        self.pcd1 = [self.xyz1[self.seg1[b]:self.seg1[b + 1]] for b in range(P)]

    def _match(self, T, radii):
        """``correspondences / seg_m``: one ``matching_indices_batched`` call when every pair has the same radius, else one per distinct
        radius on that radius's pairs, re-assembled in pair order."""
        seg0, seg1 = [int(v) for v in self.seg0], [int(v) for v in self.seg1]
        distinct = sorted(set(float(r) for r in radii))
        if len(distinct) == 1:
            self.correspondences, self.seg_m, self.match_status = matching_indices_batched(self.xyz0, self.xyz1, T, distinct[0], None,
                                                                                           collated=True, seg0=seg0, seg1=seg1)
            return
        dev = self.xyz0.device
        parts, counts, status = [None] * self.P, np.zeros(self.P, np.int64), torch.zeros(self.P, dtype=torch.int32, device=dev)
        for r in distinct:
            members = [b for b in range(self.P) if float(radii[b]) == r]
            corr, seg, st = matching_indices_batched([self.pcd0[b] for b in members], [self.pcd1[b] for b in members],
                                                     None if T is None else T[members], r, None, collated=False)
            seg = seg.cpu().numpy()
            status[members] = st
            for k, b in enumerate(members):
                parts[b] = corr[seg[k]:seg[k + 1]] + torch.tensor([[seg0[b], seg1[b]]], dtype=torch.int64).to(dev, non_blocking=True)
                counts[b] = seg[k + 1] - seg[k]
        self.correspondences = torch.cat(parts, 0)
        self.seg_m = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])).to(dev, non_blocking=True)
        self.match_status = status

    def _tensor(self, i):
        if self._sinput[i] is None:
            self._sinput[i] = SparseTensor((self.sinput0_F, self.sinput1_F)[i], coordinates=(self.sinput0_C, self.sinput1_C)[i])
        return self._sinput[i]

    @property
    def sinput0(self):
        return self._tensor(0)

    @property
    def sinput1(self):
        return self._tensor(1)

    def as_input_dict(self):
        """The reference's ``input_dict`` (``collate_pair_fn``, lib/data_loaders.py:74-85).  ``T_gt`` (a list of fp32 ``[4,4]``) and
        ``len_batch`` list only the valid pairs, as its ``if len(matching_inds[batch_id]) != 0`` does; ``correspondences`` is ``.int()``
        like the reference's.  Reads ``valid`` back (one synchronisation)."""
        valid = self.valid.cpu().numpy()
        keep = [b for b in range(self.P) if valid[b]]
        return {"pcd0": list(self.pcd0), "pcd1": list(self.pcd1),
                "sinput0_C": self.sinput0_C, "sinput0_F": self.sinput0_F, "sinput1_C": self.sinput1_C, "sinput1_F": self.sinput1_F,
                "correspondences": self.correspondences.int(),
                "T_gt": [self.T_gt[b] for b in keep], "len_batch": [self.len_batch[b] for b in keep],
                "frame_distance": self.frame_distance}
