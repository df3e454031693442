"""The evaluation loop of the reference, batched: ``scripts/test_kitti.py:130-225`` processes one pair
per iteration (two batch-1 forwards, NN, registration, metrics); here ``P`` pairs share one batched
forward (the batch column keeps their neighbourhoods apart, exactly as ``sparse_collate`` stacks
clouds, lib/data_loaders.py:65-66), one segmented NN launch, and ``P`` registration launches.

Differences from the reference that are deliberate and documented in DESIGN.md:
  * the NN of the 5000-point sample sets is computed once and feeds both the ``dists_nn`` diagnostic
    and the registration (the reference computes it twice on two different random sub-samples);
  * the random draws are injectable / seeded.
"""
from __future__ import annotations

import contextlib
import copy
import ctypes as C
import json
import logging
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, icp
from . import eval as ev
from . import registration as reg
from .eval import gather_rows, knn1_segmented
from .isolate import batch_drop, remap_rows
from .metrics import registration_errors
from .sparse_tensor import CoordinateManager, SparseTensor
from .synthetic import batch_coords, plant_correspondences, subsample_indices
from .voxelize import sparse_quantize_batch


@dataclass
class RegistrationConfig:
    """The hot-path subset of the reference's flags (config.py:82-86,102,125; scripts/test_kitti.py:240-292)."""
    model: str = "ResUNetBN2C"
    model_n_out: int = 32
    conv1_kernel_size: int = 5
    normalize_feature: bool = True
    bn_momentum: float = 0.05
    voxel_size: float = 0.3
    n_points: int = 5000                 # scripts/test_kitti.py:156
    use_RANSAC: bool = True
    ransac_max_iteration: int = 4000000  # scripts/test_kitti.py:176
    # RANSAC route only: RANSACConvergenceCriteria's confidence.  1.0 (the reference's 10000, clamped) runs every iteration; below 1 a pair
    # stops at the first checkpoint (ransac_first_check, then doubling) at which its best fitness meets the criterion, decided on the
    # device (registration.ransac_batched_from_correspondences), and the results carry ``iterations``.  ``load_config`` leaves both alone
    ransac_confidence: float = 1.0
    ransac_first_check: int = reg.RANSAC_FIRST_CHECK
    rte_thresh: float = 2.0
    rre_thresh: float = 5.0
    sc2pcr: dict = field(default_factory=lambda: dict(
        inlier_threshold=0.6, num_node=8000, use_mutual=False, d_thre=0.1, num_iterations=20, ratio=0.2,
        nms_radius=0.6, max_points=8000, k1=30, k2=20))   # scripts/SC2_PCR/config_json/config_KITTI.json
    # what a split16 overflow of the pipeline costs (automatic arithmetic only): False - the model switches to fp32 MFMAs for good and
    # the step runs again (a third of the throughput from then on); True - that step alone runs again in fp32, its pairs carry
    # RETRIED_FP32 in ``status``, and the next step is split16 again
    fp32_retry_per_step: bool = False
    # per-pair failure isolation (the reference's loops skip a bad pair and go on, lib/trainer.py:1306-1310,1596-1604): a pair whose cloud
    # fails the map build (duplicate rows, rows outside the key range) is dropped from the batch and gets a failed record with its
    # DROPPED_* bits in ``status``; the other pairs of the step are registered as without it
    isolate_failures: bool = False
    # point-to-point ICP on the pairs' sample sets right after the back-end, started from its poses on the device (eyoc_amd.icp; the
    # reference refines with Open3D on the CPU, scripts/SC2_PCR/benchmark_utils.py:40-56 behind --use_icp).  The gate defaults to
    # 2 x voxel_size: the samples are ~one voxel apart, one voxel finds a fifth of them a partner, two voxels 56-67 %
    icp_refine: bool = False
    icp_max_correspondence_distance: float | None = None
    icp_max_iteration: int = 30
    # the ICP's step: "point" (Kabsch over the correspondences) or "plane" (point-to-plane: the normals of the step's target sample sets
    # are estimated on the device first, eyoc_amd.icp.estimate_normals_batched, inside icp_normal_radius - None: 5 x voxel_size - from at
    # most icp_normal_max_nn neighbours).  Anything else raises here
    icp_method: str = "point"
    icp_normal_radius: float | None = None
    icp_normal_max_nn: int = 30
    # RANSAC route only: the reciprocity check of Open3D's ``mutual_filter`` between the feature search and the back-end - RANSAC runs on
    # the source points whose neighbour's own nearest source point is them (all of a pair's correspondences when fewer than 4 are
    # reciprocal); ``fitness`` is over the correspondences used.  One host wait per step for the kept counts (an event, not a device
    # synchronisation).  SC2-PCR resamples to a fixed ``num_node``: a filter in front of it is a separate design, asking for it raises
    mutual_filter: bool = False

    def __post_init__(self):
        if self.icp_method not in ("point", "plane"):
            raise ValueError(f"icp_method = {self.icp_method!r}: \"point\" or \"plane\"")
        if self.mutual_filter and not self.use_RANSAC:
            raise ValueError("mutual_filter is implemented for the RANSAC route only (use_RANSAC=True)")
        if not self.ransac_confidence > 0.0 or self.ransac_first_check < 1:
            raise ValueError(f"ransac_confidence = {self.ransac_confidence!r} must be above 0, ransac_first_check = {self.ransac_first_check!r} at least 1")


# ``RegistrationResult.status`` / ``PendingStep.status`` bit: the pair's step overflowed split16 and was registered again in fp32
# (``fp32_retry_per_step``); the records are those of the fp32 run
RETRIED_FP32 = 1 << 4
# why a pair was dropped from its batch (``isolate_failures`` / ``DeviceBatch.without_pairs``): a cloud of it held duplicate rows, rows
# (points) outside the key range, no voxels at all, or NaN / inf points.  A dropped pair's record: T all NaN, fitness 0, inliers 0.
DROPPED_DUPLICATE = 1 << 0
DROPPED_RANGE = 1 << 1
DROPPED_EMPTY = 1 << 2
DROPPED_NONFINITE = 1 << 3
DROPPED = DROPPED_DUPLICATE | DROPPED_RANGE | DROPPED_EMPTY | DROPPED_NONFINITE
MAX_REBUILDS = 2     # per step: the range check of a map build runs before its duplicate check, so a second fault of the other kind can follow


def pairs_of_clouds(clouds, offsets, P):
    """Collated clouds (= their batch indices) -> pairs.  ``offsets`` lists the clouds in the order ``DeviceBatch`` collates them - source
    and target of pair 0, of pair 1, ... -, so there are ``2 P`` of them and cloud ``c`` belongs to pair ``c // 2``."""
    n_clouds = len(offsets) - 1
    if n_clouds != 2 * P:
        raise ValueError(f"{n_clouds} clouds for {P} pairs")
    clouds = np.asarray(list(clouds), np.int64)
    if clouds.size and (clouds.min() < 0 or clouds.max() >= n_clouds):
        raise ValueError(f"cloud {int(clouds.max() if clouds.max() >= n_clouds else clouds.min())} is not one of the batch's {n_clouds}")
    return clouds // 2


def fault_bits(dup, rng, offsets, P):
    """The batch indices a failed map build reports (``_lib.fault_batches``) -> ``int64 [P]`` of DROPPED_* bits."""
    bits = np.zeros(P, np.int64)
    np.bitwise_or.at(bits, pairs_of_clouds(dup, offsets, P), DROPPED_DUPLICATE)
    np.bitwise_or.at(bits, pairs_of_clouds(rng, offsets, P), DROPPED_RANGE)
    return bits


def live_segments(dropped, n_points):
    """``seg int64 [P+1]`` of the per-pair sample sets when only the live pairs' rows are stored: ``n_points`` rows for a live pair, an
    EMPTY segment for a dropped one - pair ``b`` keeps slot ``b`` (and with it its seed ``seed + b``) in the batched back-ends."""
    return np.concatenate([[0], np.cumsum(np.where(np.asarray(dropped) == 0, int(n_points), 0))]).astype(np.int64)


def build_with_isolation(batch, build, fault_batches):
    """``build(batch)`` with a failed map build answered by dropping the faulty pairs: -> ``(what build returned, the batch it was built
    for)``.  An EYOC_ERR_DUPLICATE / EYOC_ERR_RANGE is looked up in ``fault_batches() -> (dup, range)`` batch indices, their pairs are
    taken out (``batch.without_pairs``: a new batch, the caller's is not modified) and the build runs again - at most MAX_REBUILDS
    times, then the ORIGINAL error is raised.  An error that names no batch index (a row whose own index is outside [0, 1024)) is raised
    as it is."""
    first = None
    for attempt in range(MAX_REBUILDS + 1):
        try:
            return build(batch), batch
        except _lib.EyocError as e:
            if e.code not in (_lib.ERR_DUPLICATE, _lib.ERR_RANGE):
                raise
            # kept as a copy without its traceback: the traceback's frames hold the failed build's workspace (gigabytes on a large
            # batch) and, through this frame, the exception itself - a cycle only the garbage collector would free
            first = first or _lib.EyocError(str(e), e.code)
            if attempt == MAX_REBUILDS:
                raise first
            dup, rng = fault_batches()
            bits = fault_bits(dup, rng, batch.offsets, batch.P)
            if not bits[batch.dropped == 0].any():      # no live pair named: nothing to drop
                raise first
            batch = batch.without_pairs(bits)


_SC2_KEYS = ("inlier_threshold", "num_node", "use_mutual", "d_thre", "num_iterations", "ratio", "nms_radius", "max_points",
             "k1", "k2")


def load_config(config, sc2pcr_config=None, use_RANSAC=True, rte_thresh=2.0, rre_thresh=5.0) -> RegistrationConfig:
    """The reference's run configuration -> ``RegistrationConfig`` (scripts/test_kitti.py:258-292).

    ``config``: the ``config.json`` a training run leaves in its ``save_dir`` (a path or the loaded dict) - the keys
    ``model``, ``model_n_out``, ``conv1_kernel_size``, ``normalize_feature``, ``bn_momentum``, ``voxel_size`` are read,
    everything else (trainer / loader settings) is ignored.  With ``use_RANSAC=False`` the SC2-PCR constants are merged
    in from ``sc2pcr_config`` (path or dict; the reference reads scripts/SC2_PCR/config_json/config_KITTI.json) exactly
    like test_kitti.py does; ``rte_thresh`` / ``rre_thresh`` are its command-line flags."""
    def as_dict(c):
        return json.load(open(c)) if isinstance(c, (str, bytes)) or hasattr(c, "__fspath__") else dict(c)
    c = as_dict(config)
    kw = {k: c[k] for k in ("model", "model_n_out", "conv1_kernel_size", "normalize_feature", "bn_momentum", "voxel_size") if k in c}
    out = RegistrationConfig(use_RANSAC=bool(use_RANSAC), rte_thresh=float(rte_thresh), rre_thresh=float(rre_thresh), **kw)
    if not use_RANSAC and sc2pcr_config is not None:
        sc = as_dict(sc2pcr_config)
        out.sc2pcr = {**out.sc2pcr, **{k: sc[k] for k in _SC2_KEYS if k in sc}}
    return out


def sample_indices(seed, i, n, n_points):
    """``random_sample`` of scripts/test_kitti.py:159-160 for cloud ``i`` (0 source, 1 target) of the pair with ``seed``: ``n_points``
    of the ``n`` voxels, without replacement when there are enough of them, with replacement otherwise."""
    if n >= n_points:
        return subsample_indices(seed * 2 + i, n, n_points)
    return np.random.default_rng(seed * 2 + i + 10**6).choice(n, n_points)



def distinct_draws(draws, live, n):
    """The bookkeeping that lets the SC2-PCR path search the DISTINCT rows of its re-sampled draws.  ``draws int64 [P, 2, nn_pts]``: per
    pair the rows (``< n``) drawn with replacement of its source (``[:, 0]``) and target (``[:, 1]``) sample set; ``live``: the pairs that
    take part, in order (live pair ``p`` is block ``q`` of every packed array).  -> ``(us, ut, inv, first, seg_a, seg_b, base)``:
    ``us`` the distinct source rows (ascending, ``+ q n``) with segments ``seg_a``; ``ut`` the distinct target rows in the order of their
    FIRST draw (``+ q n``) with segments ``seg_b``; ``inv [L nn_pts]`` draw of a source row -> its row of ``us``; ``first`` the first
    draw (``+ q nn_pts``: a row of the packed target draws) of every row of ``ut``; ``base`` row of ``us`` -> where its pair starts in ``ut``.

    With ``nn_u`` the first arg-min of every ``us`` row over the ``ut`` rows of its pair, ``first[nn_u + base][inv]`` is the first arg-min of
    every source draw over the target draws of its pair: an arg-min returns the first of equal distances, a duplicated target ties with
    itself exactly, so the winner among duplicates is the first draw, and the lowest first draw among tied distinct rows is the lowest
    index overall (tests/test_host_logic.py)."""
    nn_pts = draws.shape[2]
    us, ut, inv, first, seg_a, seg_b = [], [], [], [], [0], [0]
    pos = np.arange(nn_pts, dtype=np.int64)
    for q, p in enumerate(live):
        d0, d1 = draws[p, 0], draws[p, 1]
        present = np.zeros(n, bool)
        present[d0] = True
        u0 = np.flatnonzero(present)                                   # distinct source rows
        i0 = (np.cumsum(present) - 1)[d0]                               # draw -> its distinct row
        fst = np.full(n, nn_pts, np.int64)
        np.minimum.at(fst, d1, pos)                                     # first draw of every target row
        f1 = np.flatnonzero(fst[d1] == pos)                             # the first draws, ascending: distinct targets in that order
        u1 = d1[f1]
        us.append(u0 + q * n); inv.append(i0 + seg_a[-1])
        ut.append(u1 + q * n); first.append(f1 + q * nn_pts)
        seg_a.append(seg_a[-1] + len(u0)); seg_b.append(seg_b[-1] + len(u1))
    base = np.repeat(np.asarray(seg_b[:-1], np.int64), np.diff(seg_a))
    us, ut, inv, first = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (us, ut, inv, first))
    return us, ut, inv, first, seg_a, seg_b, base


class DeviceBatch:
    """``P`` pairs resident in HBM: batched coordinates/features for the 2P clouds, the voxel centres'
    points, and the (seeded) sample indices of ``random_sample`` (scripts/test_kitti.py:159-160).

    ``descriptor=dict(inlier_ratio=p, beta=8.0, plant_radius=0.3)`` switches on the benchmark's descriptor mode
    (``synthetic.plant_correspondences``): the sample sets contain ``p * n_points`` ground-truth partners and the
    per-sample descriptors ``G0 / G1`` are blended into the network's features inside the timed path
    (``eyoc_gather_rows``), so that the matcher sees a stated inlier ratio instead of the zero signal of
    random-init weights."""

    def __init__(self, pairs, seeds, device, n_points=5000, descriptor=None, isolate=False):
        """``isolate=True``: a pair with a cloud of 0 voxels is dropped at construction (DROPPED_EMPTY in ``dropped``) instead of
        failing the sample draw; see ``without_pairs`` for what a dropped pair leaves behind."""
        clouds = [p[f"coords{i}"] for p in pairs for i in (0, 1)]
        feats = np.concatenate([p[f"feats{i}"] for p in pairs for i in (0, 1)], 0)
        self._collate(torch.from_numpy(batch_coords(clouds)).to(device), torch.from_numpy(feats).to(device),
                      np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), [p["T_gt"] for p in pairs], descriptor)
        if isolate:
            self.dropped[np.minimum(self.sizes[0::2], self.sizes[1::2]) == 0] = DROPPED_EMPTY
        planted = {}
        if self.descriptor:
            d = self.descriptor
            planted = {j: plant_correspondences(pairs[j], seeds[j], n_points, d.get("inlier_ratio", 0.3), d.get("plant_radius", 0.3),
                                                d.get("feat_dim", 32)) for j in np.flatnonzero(self.dropped == 0)}
            self.planted = [planted[j]["planted"] if j in planted else None for j in range(self.P)]
            if planted:
                self.G0 = torch.from_numpy(np.concatenate([pl["G0"] for pl in planted.values()])).to(device)
                self.G1 = torch.from_numpy(np.concatenate([pl["G1"] for pl in planted.values()])).to(device)

        def points(i, live, rows, sel):
            xyz = [pairs[j][f"xyz{i}"][r] for j, r in zip(live, rows)]
            return torch.from_numpy(np.stack(xyz) if xyz else np.zeros((0, n_points, 3), np.float32)).to(device)
        self._draw_samples(seeds, n_points, device, points, planted)

    @classmethod
    def from_scans(cls, scans, T_gt, seeds, device, voxel_size=0.3, n_points=5000, descriptor=None, isolate=False):
        """The same batch from RAW scans: ``scans`` = ``[(src, tgt), ...]`` unvoxelised ``[N,3]`` / ``[N,4]`` float32 clouds (numpy or
        torch), voxelised and collated on the GPU by ONE ``sparse_quantize_batch`` call (one read-back: the clouds' voxel counts) -
        lib/data_loaders.py:936-979 per cloud and ``collate_pair_fn`` (:31-85) for the batch.  The sample draws are ``__init__``'s
        (``sample_indices`` on the counts); the sampled points are gathered on the device.  Equal, attribute for attribute, to
        ``DeviceBatch(pairs, seeds, device, n_points)`` of the pairs these scans voxelise to.  The descriptor mode plants its
        correspondences on the host and is not available here.

        ``isolate=True``: the isolating voxeliser (``sparse_quantize_batch(isolate=True)``); a pair with a cloud that holds a point
        outside the key range or a NaN / inf point, or that has no voxels at all, is dropped at construction (DROPPED_RANGE /
        DROPPED_NONFINITE / DROPPED_EMPTY in ``dropped``, see ``without_pairs``) instead of failing the call.  The live pairs' draws
        are seeded per pair and do not change."""
        if descriptor:
            raise ValueError("DeviceBatch.from_scans: the descriptor mode (plant_correspondences) needs host-voxelised pairs")
        if not len(scans) == len(T_gt) == len(seeds):
            raise ValueError(f"DeviceBatch.from_scans: {len(scans)} scan pairs, {len(T_gt)} poses, {len(seeds)} seeds")
        clouds = [c for pair in scans for c in pair]
        coords, _, kept_xyz, offsets, *faults = sparse_quantize_batch(clouds, voxel_size, 0, device=torch.device(device), isolate=bool(isolate))
        self = cls.__new__(cls)
        self._collate(coords, torch.ones((len(coords), 1), dtype=torch.float32, device=coords.device), offsets, T_gt, None)
        if isolate:
            per_cloud = (np.where(faults[0][:, 0] > 0, DROPPED_RANGE, 0) | np.where(faults[0][:, 1] > 0, DROPPED_NONFINITE, 0)).astype(np.int64)
            per_cloud[(per_cloud == 0) & (np.diff(offsets) == 0)] = DROPPED_EMPTY
            self.dropped = per_cloud[0::2] | per_cloud[1::2]
        self._draw_samples(seeds, n_points, coords.device, lambda i, live, rows, sel: kept_xyz[sel].reshape(-1, n_points, 3))
        return self

    def _collate(self, coords, feats, offsets, T_gt, descriptor):
        """What both constructors know once the clouds are collated: the batched rows, the clouds' row ranges, the poses; no pair dropped
        yet, no descriptors."""
        self.P = len(T_gt)
        self.descriptor = dict(descriptor) if descriptor else None
        self.beta = float(self.descriptor.get("beta", 8.0)) if self.descriptor else 0.0
        self.coords, self.feats, self.offsets = coords, feats, offsets
        self.sizes = [int(v) for v in np.diff(offsets)]
        self.T_gt = [np.asarray(T, np.float32) for T in T_gt]
        self.dropped = np.zeros(self.P, np.int64)     # DROPPED_* bits per pair (0: the pair is live)
        self.G0 = self.G1 = None
        self.planted = []

    def _draw_samples(self, seeds, n_points, device, points, planted=None):
        """The tail both constructors share: the live pairs' draws (``planted[j]``'s in the descriptor mode, else ``sample_indices``)
        -> ``sel0 / sel1`` (rows of ``coords``), ``xyz0 / xyz1`` (``points(i, live, rows, sel)``: the points of cloud ``i``'s draws -
        given as the live pairs and their rows within the cloud, and as ``sel`` - ``[L, n_points, 3]`` on the device), ``seg / counts /
        n_points``; then the partner clouds of the dropped pairs go (a faulty or empty cloud has no rows already)."""
        live = np.flatnonzero(self.dropped == 0)
        sel, xyz = [], []
        for i in (0, 1):
            rows = [planted[j][f"sel{i}"] if planted else sample_indices(seeds[j], i, self.sizes[2 * j + i], n_points) for j in live]
            idx = np.concatenate([np.zeros(0, np.int64)] + [r + self.offsets[2 * j + i] for j, r in zip(live, rows)])
            sel.append(torch.from_numpy(idx).to(device))
            xyz.append(points(i, live, rows, sel[i]))
        self.sel0, self.sel1 = sel
        self.xyz0, self.xyz1 = xyz     # [P, n_points, 3] (the live pairs only, like sel / G, once pairs were dropped)
        self.counts = [n_points] * self.P
        self.seg = np.arange(self.P + 1) * n_points
        self.n_points = n_points
        if self.dropped.any():
            self.seg = live_segments(self.dropped, n_points)
            self._remove_clouds(np.flatnonzero(self.dropped))

    def _remove_clouds(self, pairs):
        """Takes the rows of both clouds of ``pairs`` out of ``coords / feats`` (``eyoc_batch_drop``: the other rows keep their order and
        their batch indices), sends ``sel0 / sel1`` - which hold the live pairs only by now - through the row map on the device and
        updates ``sizes / offsets``.  In place: for a batch under construction."""
        clouds = [2 * int(p) + i for p in pairs for i in (0, 1)]
        self.coords, self.feats, row_map, kept = batch_drop(self.coords, self.feats, clouds)
        self.sel0, self.sel1 = remap_rows(self.sel0, row_map), remap_rows(self.sel1, row_map)
        self.sizes = [int(v) for v in kept[:2 * self.P]]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)])

    def without_pairs(self, bits_by_pair):
        """A new batch without the clouds of some pairs; this one is not modified.  ``bits_by_pair``: DROPPED_* bits per pair (``[P]``, 0 =
        keep; or a ``{pair: bits}`` dict).  ``P``, ``T_gt``, ``n_points`` and every pair's slot stay: the dropped pairs' rows are removed
        from ``coords / feats`` on the device (batch indices unchanged), ``sel0 / sel1 / xyz0 / xyz1 / G0 / G1`` hold the live pairs only,
        back to back, ``seg`` gives a dropped pair an EMPTY segment - pair ``b`` still samples with ``seed + b`` in the batched
        back-ends, which answer an empty segment with a failed record (``eyoc_registration_accept_degenerate``) -, ``sizes / offsets``
        are those of the remaining rows and ``dropped`` carries the bits."""
        if isinstance(bits_by_pair, dict):
            bits = np.zeros(self.P, np.int64)
            for p, b in bits_by_pair.items():
                bits[int(p)] = int(b)
        else:
            bits = np.asarray(bits_by_pair, np.int64)
        if bits.shape != (self.P,) or (bits & ~DROPPED).any():
            raise ValueError(f"without_pairs: DROPPED_* bits for each of the {self.P} pairs")
        out = copy.copy(self)
        out.T_gt, out.counts, out.planted, out.sizes = list(self.T_gt), list(self.counts), list(self.planted), list(self.sizes)
        out.dropped = self.dropped | bits
        new = (bits != 0) & (self.dropped == 0)
        if not new.any():
            return out
        # the per-pair arrays hold the pairs that were live so far: keep those that still are
        stay = torch.from_numpy(np.flatnonzero(~new[self.dropped == 0])).to(self.sel0.device)
        n = self.n_points
        out.sel0 = self.sel0.reshape(-1, n).index_select(0, stay).reshape(-1)
        out.sel1 = self.sel1.reshape(-1, n).index_select(0, stay).reshape(-1)
        out.xyz0, out.xyz1 = self.xyz0.index_select(0, stay), self.xyz1.index_select(0, stay)
        if self.G0 is not None:
            c = self.G0.shape[1]
            out.G0 = self.G0.reshape(-1, n, c).index_select(0, stay).reshape(-1, c)
            out.G1 = self.G1.reshape(-1, n, c).index_select(0, stay).reshape(-1, c)
        out.seg = live_segments(out.dropped, n)
        out._remove_clouds(np.flatnonzero(new))
        return out

    def record_stream(self, stream):
        """A batch made on one stream (``prepare_maps``' side stream drops pairs there) and read on another: ties its device tensors to
        the reading stream, so that the caching allocator reuses their memory only after that stream's work."""
        for t in (self.coords, self.feats, self.sel0, self.sel1, self.xyz0, self.xyz1, self.G0, self.G1):
            if t is not None:
                t.record_stream(stream)

    @property
    def voxels(self):
        return int(self.offsets[-1])


class MapsHandle(NamedTuple):
    """What ``prepare_maps`` returns and ``register`` / ``enqueue`` take as ``maps=``."""
    cm: CoordinateManager      # the coordinate manager with the maps built
    ready: torch.cuda.Event    # recorded on the side stream behind the build
    batch: DeviceBatch         # the batch the maps describe: the caller's own, or (isolate_failures) it without the pairs that failed the build


class _Step:
    """What ONE enqueued step produced (``RegistrationPipeline._step``).  Nothing of it is on the pipeline: ``_publish`` makes a step
    "the last step", a retry hands its step to whoever asked for it."""
    __slots__ = ("slot", "timers", "batch", "F", "featured", "matched", "nn_idx", "kept_rows", "kept_seg", "result", "packed", "icp", "words",
                 "host", "icp_host", "done")

    def __init__(self, slot, timers):
        self.slot, self.timers = slot, timers      # the buffer set the step uses; its four stage-timer events (None: not timed)
        self.batch = self.F = None                 # the batch the step actually ran on (isolate_failures: reduced) and its features
        self.featured = self.matched = None        # events: the forward is enqueued / forward and matching are enqueued
        self.nn_idx = None                         # RANSAC path: the feature correspondences on the device
        self.kept_rows = self.kept_seg = None      # mutual_filter: the source rows RANSAC ran on (device, row inside its pair) and their segments (host, [P + 1])
        self.result = self.icp = None              # the back-end's records on the device; icp_refine: the ``eyoc_icp_result`` records
        self.packed = None                         # ransac_confidence < 1: ONE device buffer, the records (= ``result``, a view) in front and the
                                                   # pairs' int32 iterations behind - what the step's one read-back copies
        self.words = self.host = self.icp_host = self.done = None    # the read-back, when it was enqueued with the step


class PendingStep:
    """A step whose read-back was enqueued with it (``RegistrationPipeline.enqueue``)."""

    def __init__(self, host, words, done, device_result, keep=None, retry=None, dropped=None, icp=None, packed=False):
        self.host, self.words, self.done, self.device_result = host, words, done, device_result
        self.iterations = None    # ransac_confidence < 1: int32 [P] in the same pinned buffer, behind the records (valid like ``host``)
        self._packed = None
        if packed:                # the read-back was the step's packed buffer: records in front, iterations behind
            self._packed, (self.host, self.iterations) = host, split_packed(host)
        self.icp = icp            # icp_refine: the step's ``eyoc_icp_result`` records, ``uint8 [P, 160]`` in pinned host memory (valid like ``host``)
        self.dropped = dropped    # isolate_failures: the step's DROPPED_* bits per pair (their records are the back-end's failed ones)
        self.keep = keep          # tensors another stream still reads (the features under ``tail_stream``): released by ``wait``
        self.retry = retry        # fp32_retry_per_step: (pipeline, batch, seed, maps, slot) to run the step again in fp32 after an overflow
        self.status = None        # per-pair status bits (int64 [P]), set by ``wait``

    def wait(self):
        """-> (result records ``uint8 [P, 84]`` in pinned host memory - valid until the slot is enqueued again -, whether this
        step's split16 forward overflowed).  Waits for this step only.  Sets ``status``; under ``fp32_retry_per_step`` an overflowed step
        is run again in fp32 right here (its records replace the split16 ones, every pair is flagged RETRIED_FP32)."""
        self.done.synchronize()
        self.keep = None
        overflow = bool(int(self.words[0]) != 0)
        self.status = np.zeros(self.host.shape[0], np.int64) if self.dropped is None else np.array(self.dropped, np.int64)
        if overflow and self.retry is not None:
            pipe, batch, seed, maps, slot = self.retry
            again = pipe._retry_fp32(batch, seed, maps, slot, pipelined=True)
            if self._packed is not None:
                self._packed.copy_(again.packed.cpu())
            else:
                self.host.copy_(again.result.cpu())
            if self.icp is not None:
                self.icp.copy_(again.icp.cpu())
            self.status |= RETRIED_FP32
        self.retry = None
        return self.host, overflow


RECORD_BYTES = C.sizeof(_lib.RansacResult)


def split_packed(buf):
    """A step's packed buffer (``uint8 [P * (RECORD_BYTES + 4)]``, device or host) -> views ``(records uint8 [P, RECORD_BYTES],
    iterations int32 [P])``."""
    P = buf.numel() // (RECORD_BYTES + 4)
    return buf[:P * RECORD_BYTES].view(P, RECORD_BYTES), buf[P * RECORD_BYTES:].view(torch.int32)


_CALLERS_STREAM = contextlib.nullcontext()      # the tail of a step that stays on the stream of its forward


class RegistrationPipeline:
    def __init__(self, model, config: RegistrationConfig | None = None):
        self.model = model
        self.cfg = config or RegistrationConfig()
        self.matcher = None if self.cfg.use_RANSAC else reg.Matcher(**self.cfg.sc2pcr)
        # per-stage timers like the reference's feat / reg timers (scripts/test_kitti.py:109,217-222): with
        # ``timing = True`` every ``register`` brackets its stages with events on the launch stream and
        # ``stage_ms()`` returns the durations of the last call (synchronises)
        self.timing = False
        self.slot = 0          # which of two event sets the next ``register`` records into (see ``stage_ms``)
        self._ev = None
        self.fp32_retries = 0  # fp32_retry_per_step: steps run again in fp32 after a split16 overflow
        self.dropped_pairs = 0  # isolate_failures: pairs that got a failed record because their batch was registered without them
        # the last step (``_publish``): its events - the forward is enqueued / forward and matching are enqueued, what ``prepare_maps(after=)``
        # of the NEXT batch may wait for -, the RANSAC path's correspondences (``correspondence_inlier_ratio``), ...
        self.featured = self.matched = self.last_nn_idx = None
        self.registered_batch = None   # isolate_failures: the batch the last step actually ran on (the caller's, or it without the dropped pairs)
        self.last_icp = None    # icp_refine: the ICP results of the last ``register`` (one RegistrationResult per pair: status, iterations, fitness)
        self._icp_dev = None    # ... and the last step's ``eyoc_icp_result`` records on the device
        # streams and pinned buffers, made on first use (a stream needs a device)
        self.side_priority = 0            # of ``prepare_maps``' side stream; read when that stream is made
        self._side = self._tail = None
        self._pinned, self._pinned_w, self._stage = {}, {}, {}     # by (slot, shape, dtype) / slot / slot
        self._range_words = None          # ``register``'s own copy of the guard's words
        self._ransac_budget = None

    def _mark(self, step, i):
        if step.timers is not None:
            step.timers[i].record()

    def stage_ms(self, slot=None):
        """``dict(feat=, match=, reg=)`` of the last timed ``register`` of event set ``slot`` (default: the current
        one): maps + forward; row gather + feature NN; RANSAC / SC2-PCR.  Two sets, so that step k's timers can be read
        after step k+1 was enqueued."""
        e = self._ev[self.slot if slot is None else slot]
        e[3].synchronize()
        return {"feat": e[0].elapsed_time(e[1]), "match": e[1].elapsed_time(e[2]), "reg": e[2].elapsed_time(e[3])}

    @torch.no_grad()
    def features(self, batch: DeviceBatch, maps=None) -> SparseTensor:
        """scripts/test_kitti.py:141-150 for all 2P clouds at once (the maps are rebuilt per call, like
        the reference rebuilds its coordinate manager for every SparseTensor - or taken from ``prepare_maps``)."""
        # the split16 range check is deferred to where ``register`` synchronises anyway (no host wait after the forward)
        return self._features(batch, maps)[0]

    @torch.no_grad()
    def _features(self, batch, maps, sampled=False):
        """``features`` -> (the features, the batch they belong to): under ``isolate_failures`` that is ``batch`` without the pairs a
        failed map build named - dropped here, or by ``prepare_maps``, whose handle then carries the reduced batch.  Without a graph
        on every route (``enqueue`` and ``validate`` come here outside ``no_grad``): the packed plan never builds one, and an opted-in
        ``ResUNetIN2`` model takes that plan only where no gradient can be asked for (``model._runs_packed``).

        ``sampled`` (the step): only the rows matching reads, ``model(x, rows=cat(sel0, sel1))`` of the batch the forward runs on -
        a dense ``[2 P n, C]`` tensor, ``sel0``'s rows first, bit for bit ``model(x).F[rows]``."""
        check, self.model.range_check = self.model.range_check, False
        try:
            if maps is None and not self.cfg.isolate_failures:
                return self._forward(SparseTensor(batch.feats, coordinates=batch.coords), batch, sampled), batch
            if maps is None:
                cm, batch = self._build_maps(batch)
            else:
                cm, ready, reduced = maps
                torch.cuda.current_stream().wait_event(ready)
                if self.cfg.isolate_failures and reduced is not batch:
                    batch = reduced
                    batch.record_stream(torch.cuda.current_stream())     # made on the side stream, read on this one
            return self._forward(SparseTensor(batch.feats, coordinate_manager=cm), batch, sampled), batch
        finally:
            self.model.range_check = check

    def _forward(self, x, batch, sampled):
        if not sampled:
            return self.model(x)
        # the sample is drawn before the forward (``DeviceBatch``), by index only - like the reference's ``random_sample``
        cached = batch.__dict__.get("_sel01")
        if cached is None or cached[0] is not batch.sel0 or cached[1] is not batch.sel1:
            cached = batch.__dict__["_sel01"] = (batch.sel0, batch.sel1, torch.cat((batch.sel0.reshape(-1), batch.sel1.reshape(-1))))
        return self.model(x, rows=cached[2])

    def _build_maps(self, batch):
        """The maps of ``batch`` on the current stream -> ``(coordinate manager, the batch it describes)``: under ``isolate_failures``
        ``batch`` without the pairs whose clouds failed the build."""
        def build(b):
            cm = CoordinateManager(b.coords)
            cm.maps(-1)
            return cm
        if not self.cfg.isolate_failures:
            return build(batch), batch
        return build_with_isolation(batch, build, lambda: _lib.fault_batches(batch.coords.device))

    @contextlib.contextmanager
    def _accept_degenerate(self, device):
        """isolate_failures: the back-ends' switch for pairs below their minimum (``eyoc_registration_accept_degenerate``), on inside the
        block - a dropped pair is an empty segment and gets a failed record instead of failing the call."""
        if not self.cfg.isolate_failures:
            yield
            return
        prev = _lib.knob("eyoc_registration_accept_degenerate", 1, device=device)
        try:
            yield
        finally:
            _lib.knob("eyoc_registration_accept_degenerate", prev, device=device)

    def _step(self, batch, seed, maps, slot, timed, tail=None, read_back=False):
        """Enqueues ONE step - forward, row gather + feature NN + back-end, ICP if configured - and returns what it produced; publishes
        nothing on the pipeline.  ``slot``: the buffer set (event set, SC2-PCR index staging, pinned read-back buffers).  ``tail``: the
        stream everything behind the forward goes on (it waits for the forward); None keeps it on the caller's stream.  The
        arithmetic is the model's ``spconv_math`` of the moment.

        ``read_back``: the read-back of the records (and the ICP records) into the slot's pinned buffers and of the split16 guard's
        verdict on THIS forward is enqueued with the step, ``done`` recorded behind it.  A read-back issued after the next step was
        enqueued queues behind that whole step on the stream: the host then never runs ahead of the GPU, and the GPU idles while the
        host decodes results and launches the next step (measured: 2 ms of a 24 ms step)."""
        if timed and self._ev is None:
            self._ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(2)]
        step = _Step(slot, self._ev[slot] if timed else None)
        main = torch.cuda.current_stream()
        self._mark(step, 0)
        step.F, step.batch = self._features(batch, maps, sampled=True)     # the sampled rows only: [sel0's rows | sel1's rows]
        self._mark(step, 1)
        if read_back:
            step.words = self._pinned_words(slot)
            if tail is not None:
                # the guard's words are this forward's own only until the next forward starts: snapshot them on the forward's stream
                self.model.range_snapshot(step.words)
        step.featured = torch.cuda.Event()
        step.featured.record(main)
        if tail is not None:
            tail.wait_event(step.featured)
        with _CALLERS_STREAM if tail is None else torch.cuda.stream(tail):
            if tail is not None and self.cfg.isolate_failures and step.batch.dropped.any():
                step.batch.record_stream(tail)
            step.result = (self._match_and_register if self.cfg.use_RANSAC else self._match_and_register_sc2)(step, seed)
            self._mark(step, 3)
            if read_back:
                dev = step.result if step.packed is None else step.packed      # records and iterations come back in the one copy
                step.host = self._pinned_set(slot, dev)
                step.host.copy_(dev, non_blocking=True)
                if self.cfg.icp_refine:
                    step.icp_host = self._pinned_set(slot, step.icp)
                    step.icp_host.copy_(step.icp, non_blocking=True)
                if tail is None:
                    self.model.range_snapshot(step.words)     # one stream: the next forward is behind all of this anyway
                step.done = torch.cuda.Event()
                step.done.record(main if tail is None else tail)
        return step

    def _publish(self, step, count_dropped=True):
        """``step`` becomes what the pipeline keeps about the LAST step; -> ``step``."""
        self.featured, self.matched, self.last_nn_idx, self._icp_dev = step.featured, step.matched, step.nn_idx, step.icp
        if self.cfg.isolate_failures:
            self.registered_batch = step.batch
            if count_dropped:
                self.dropped_pairs += int((step.batch.dropped != 0).sum())
        return step

    @torch.no_grad()
    def _retry_fp32(self, batch, seed, maps, slot, pipelined):
        """fp32_retry_per_step: this step again with fp32 MFMAs on the current stream, and back to the model's own arithmetic for the
        next one -> the step.  The re-run uses the overflowed step's own buffer set ``slot`` (the SC2-PCR index staging of the other
        slot may still feed a step in flight).  It is not published here: a pipelined step's re-run (``PendingStep.wait``) leaves
        what the pipeline keeps about the LAST enqueued step, stage timers included, as it was; ``register``'s own IS the last step
        and ``register`` publishes it."""
        self.fp32_retries += 1
        if pipelined:     # a pipelined step knew of its overflow from its own words: clear the sticky flag the guard still holds
            try:
                self.model.check_range()
            except _lib.EyocError as e:
                if e.code != _lib.ERR_RANGE:
                    raise
        math, self.model.spconv_math = self.model.spconv_math, "fp32"
        try:
            return self._step(batch, seed, maps, slot, self.timing and not pipelined)
        finally:
            self.model.spconv_math = math

    @torch.no_grad()
    def prepare_maps(self, batch: DeviceBatch, after=None) -> MapsHandle:
        """Build the coordinate maps of ``batch`` NOW, on a side stream: they only depend on the coordinates, so a
        serving loop builds the next batch's maps (hash / sort / rulebook kernels, latency- and atomics-bound) while the
        previous batch is still in its RANSAC (VALU-bound) on the main stream.  Returns the handle ``register(...,
        maps=)`` takes, a ``MapsHandle(cm, ready, batch')``; it may be dropped right after the step was enqueued (the maps' workspace is
        recorded on every stream that reads it, ``CoordinateManager._reading``).  ``batch'`` is ``batch`` itself or, under
        ``isolate_failures``, ``batch`` without the pairs whose clouds failed the build, and ``register`` / ``enqueue`` run on it.
        ``after``: an event the side stream waits for
        first - ``self.matched`` (recorded by ``register`` when its forward and matching are enqueued) puts the build
        beside that step's RANSAC instead of beside whatever the main stream happens to run at enqueue time (the forward:
        both want LDS and the atomics path, and the forward's kernels slow down by ~10 %)."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=batch.coords.device, priority=self.side_priority)
        if after is not None:
            self._side.wait_event(after)
        with torch.cuda.stream(self._side):
            # (isolate_failures: a failed build has synchronised the side stream and raised: stream and ctx are free for the drop and the rebuild)
            cm, batch = self._build_maps(batch)
            ready = torch.cuda.Event()
            ready.record(self._side)
        return MapsHandle(cm, ready, batch)

    def enqueue(self, batch: DeviceBatch, seed: int = 0, maps=None, slot: int = 0, tail_stream: bool = False) -> "PendingStep":
        """``register`` for a caller that pipelines steps: everything - the read-back of the ``[P, 84]`` result records (RANSAC path;
        ``T f32 [P, 4, 4]`` on the SC2-PCR path) into pinned host memory and of the split16 guard's verdict on THIS forward included -
        is enqueued now (``_step(read_back=True)`` says why); the host waits on ``PendingStep.wait()`` later.
        ``slot``: which of the two pinned buffer sets to use (a set is free again once its ``wait()`` returned).

        ``tail_stream=True`` (two steps in flight): only the forward (+ the guard's snapshot) goes on the caller's
        stream; row gather, feature NN, RANSAC and the read-back of the records go on a second stream of the pipeline that waits
        for the forward.  A caller that enqueues the next step right away gets that step's forward (matrix pipe, LDS) beside this
        step's matching / RANSAC (fp64 VALU, no LDS) - same kernels, same inputs, bit-identical records."""
        self.slot = slot
        if tail_stream and self._tail is None:
            self._tail = torch.cuda.Stream(device=batch.coords.device)
        step = self._publish(self._step(batch, seed, maps, slot, self.timing, self._tail if tail_stream else None, read_back=True))
        retry = None
        if self.cfg.fp32_retry_per_step and self.model.spconv_math == "auto":
            # what a retry runs on - under isolate_failures the reduced batch, which builds cleanly without the handle
            retry = (self, step.batch, seed, None if self.cfg.isolate_failures else maps, slot)
        # under ``tail_stream`` F was allocated on the caller's stream and is read on the tail stream: it stays referenced until wait()
        return PendingStep(step.host, step.words, step.done, step.result, keep=(step.F,) if tail_stream else None, retry=retry,
                           dropped=step.batch.dropped.copy() if self.cfg.isolate_failures else None, icp=step.icp_host,
                           packed=step.packed is not None)

    def _icp_refine(self, step, T):
        """icp_refine: one batched ICP over the pairs' sample sets on the CURRENT stream, started from the back-end's poses ``T f32 [P, 16]``
        as they are on the device -> the refined poses, f32 ``[P, 16]`` (the fp64 result rounded once).  A pair without a pose (NaN:
        dropped, degenerate) keeps it and gets BAD_INIT, an empty segment FEW; the records stay in ``step.icp``."""
        batch, gate = step.batch, self.cfg.icp_max_correspondence_distance
        gate = 2.0 * self.cfg.voxel_size if gate is None else gate
        if self.cfg.icp_method == "plane":     # the same records from the point-to-plane step, normals from the target sample sets themselves
            xyz1, radius = batch.xyz1.reshape(-1, 3), self.cfg.icp_normal_radius
            normals, _ = icp.estimate_normals_batched(xyz1, batch.seg, 5.0 * self.cfg.voxel_size if radius is None else radius,
                                                      self.cfg.icp_normal_max_nn)
            step.icp = icp.icp_plane_batched(batch.xyz0.reshape(-1, 3), xyz1, normals, batch.seg, batch.seg, gate, T.to(torch.float64),
                                             self.cfg.icp_max_iteration)
        else:
            step.icp = icp.icp_batched(batch.xyz0.reshape(-1, 3), batch.xyz1.reshape(-1, 3), batch.seg, batch.seg, gate,
                                       T.to(torch.float64), self.cfg.icp_max_iteration)
        return step.icp.view(torch.float64)[:, :16].to(torch.float32)

    def _pinned_stage(self, slot, count):
        """Pinned int64 staging for the index upload of the SC2-PCR path; one buffer per slot (a slot's previous upload was consumed by
        the time its step's results were read)."""
        buf = self._stage.get(slot)
        if buf is None or buf.numel() < count:
            buf = self._stage[slot] = torch.empty(max(count, 1), dtype=torch.int64, pin_memory=True)
        return buf

    def _pinned_words(self, slot):
        if slot not in self._pinned_w:
            self._pinned_w[slot] = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        return self._pinned_w[slot]

    def _pinned_set(self, slot, res):
        key = (slot, tuple(res.shape), res.dtype)
        if key not in self._pinned:
            self._pinned[key] = torch.empty(res.shape, dtype=res.dtype, pin_memory=True)
        return self._pinned[key]

    def _matched(self, step):
        """Forward and matching are enqueued on the current stream: the step's ``matched`` event (``prepare_maps(after=)``), timer 2."""
        self._mark(step, 2)
        step.matched = torch.cuda.Event()
        step.matched.record()

    def _sampled_halves(self, step):
        """``step.F`` holds the forward's rows ``sel0`` then ``sel1`` -> what ``gather_rows(F, sel, G, beta)`` gave on the full features:
        the halves as they are, or blended with the planted descriptors by the same kernel (``eyoc_gather_rows`` without an index
        list), so that the blended rows keep their bits."""
        batch, F = step.batch, step.F
        n0 = batch.sel0.numel()
        F0, F1 = F[:n0], F[n0:]
        if batch.G0 is not None:
            F0 = gather_rows(F0, None, batch.G0, batch.beta)
        if batch.G1 is not None:
            F1 = gather_rows(F1, None, batch.G1, batch.beta)
        return F0, F1

    def _match_and_register(self, step, seed):
        """Row gather (+ descriptor blend), segmented feature NN and the batched RANSAC of all pairs on the CURRENT stream ->
        ``[P, 84]`` result records on the device."""
        batch, F = step.batch, step.F
        F0, F1 = self._sampled_halves(step)                        # the sampled rows (+ descriptor blend, if any)
        # isolate_failures: a dropped pair is an empty segment - for the neighbour search, which gives the live rows what the live
        # segments alone give (tests/test_gpu_isolate_batch.py), and for the back-end, where it keeps the pair's slot and every seed
        src, seg_src = batch.xyz0.reshape(-1, 3), batch.seg
        if self.cfg.mutual_filter:
            # nn_idx stays the full forward result; RANSAC gets the kept source rows, their neighbours and their segments
            _, step.nn_idx, flags, _ = ev._knn1_mutual_flags(F0, F1, batch.seg, batch.seg, "SquareL2", False)
            rows, corr, seg_dev = ev.mutual_compact_device(step.nn_idx, flags, batch.seg, min_keep=4)
        else:
            step.nn_idx = corr = knn1_segmented(F0, F1, batch.seg, batch.seg, "SquareL2", return_distance=False)
        self._matched(step)
        if self.cfg.mutual_filter:
            # the step's one extra host wait: this stream's event behind a copy into the slot's own pinned staging
            step.kept_seg = seg_src = ev.read_back_segments(seg_dev, self._pinned_set(step.slot, seg_dev))
            m = int(seg_src[-1])
            counts = (seg_dev[1:] - seg_dev[:-1]).to(torch.int64)
            # the pairs' first rows on the device: uploaded once per batch (keyed by the ``seg`` object, like ``_sel01``)
            cached = batch.__dict__.get("_seg_first")
            if cached is None or cached[0] is not batch.seg:
                cached = batch.__dict__["_seg_first"] = (batch.seg, torch.as_tensor(np.asarray(batch.seg[:-1], np.int64)).to(F.device))
            first = cached[1]
            step.kept_rows, corr = rows[:m], corr[:m]
            src = src[step.kept_rows + torch.repeat_interleave(first, counts, output_size=m)]
        # all pairs in one batched call (pair p samples with seed + p, exactly like a per-pair loop would)
        # (the scratch budget - a quarter of the free memory, a driver round trip - is asked for once per pipeline: any launch-chunk
        # size gives the same records)
        if self._ransac_budget is None:
            self._ransac_budget = reg._ransac_budget(F.device)
        out, more = None, {}
        if self.cfg.ransac_confidence < 1.0:
            # records and iterations in one buffer, so that the step's one read-back brings both
            step.packed = torch.empty(batch.P * (RECORD_BYTES + 4), dtype=torch.uint8, device=F.device)
            out = split_packed(step.packed)
            more = dict(confidence=self.cfg.ransac_confidence, first_check=self.cfg.ransac_first_check, _out=out)
        with self._accept_degenerate(F.device):
            res = reg.ransac_batched_from_correspondences(
                src, batch.xyz1.reshape(-1, 3), corr, seg_src, batch.seg,
                self.cfg.voxel_size * 1.0, self.cfg.ransac_max_iteration, seed=seed,
                workspace_budget=self._ransac_budget, **more)                          # [P, 84] bytes on the device
        if self.cfg.icp_refine:
            res.view(torch.float32)[:, :16] = self._icp_refine(step, res.view(torch.float32)[:, :16])
        return res

    @torch.no_grad()
    def register(self, batch: DeviceBatch, seed: int = 0, return_device=False, maps=None):
        """One pass of the hot path over ``P`` pairs -> ``T f32 [P,4,4]`` (host) and per-pair stats."""
        step = self._publish(self._step(batch, seed, maps, self.slot, self.timing))
        if return_device:
            return step.result            # the caller reads back later - and calls model.check_range() then
        return self._read_back(step, seed, maps)

    def validate(self, batch: DeviceBatch, pcd0=None, hit_ratio_thresh=0.1, maps=None):
        """The validation step of the reference (lib/trainer.py:340-378) for all pairs of ``batch``: sampled forward, feature NN, the
        batched IRLS pose and the loop's metrics, one read-back -> ``validate.ValidStep`` (``eyoc_amd.validate.valid_step`` documents the
        arguments and the two deviations: seeded draws, ``pcd0=None``).  ``_step``'s registration routes are not involved."""
        from .validate import valid_step
        return valid_step(self, batch, pcd0, hit_ratio_thresh, maps)

    def _read_back(self, step, seed, maps, status=0):
        """``register``: the records of ``step`` on the host, decoded (``status`` or-ed in) - or, after a split16 overflow in automatic
        mode, those of the step run again: that step alone in fp32 (``fp32_retry_per_step``), or with the model switched to fp32 MFMAs for good."""
        words = self._range_snapshot()
        if step.packed is None:
            host, its = step.result.cpu(), None
        else:                         # still one copy: the iterations lie behind the records
            host, its = split_packed(step.packed.cpu())
        if self.cfg.icp_refine:     # the ICP records follow the results to the host (the stream is drained by then)
            icp_host = step.icp.cpu()
            self.last_icp = [icp.decode_icp_result(icp_host[p]) for p in range(icp_host.shape[0])]
        batch = step.batch
        if self.cfg.isolate_failures:
            maps = None               # what a re-run runs on: the reduced batch builds cleanly without the handle
        # words all clear: nothing overflowed since the last check, no need to ask the device again
        if int(words[0]) != 0 or int(words[3]) != 0:
            try:
                self.model.check_range()
            except _lib.EyocError as e:
                if e.code != _lib.ERR_RANGE or self.model.spconv_math != "auto" or status:      # (status: this IS the fp32 re-run)
                    raise
                if self.cfg.fp32_retry_per_step:
                    again = self._publish(self._retry_fp32(batch, seed, maps, self.slot, pipelined=False), count_dropped=False)
                    return self._read_back(again, seed, maps, RETRIED_FP32)
                logging.warning("eyoc_amd: split16 overflow in the registration pipeline; switching the model to fp32 MFMAs")
                self.model.spconv_math = "fp32"
                return self.register(batch, seed, False, maps)
        if self.cfg.use_RANSAC:
            used = np.full(batch.P, batch.n_points) if step.kept_seg is None else np.diff(step.kept_seg)      # mutual_filter: fitness over the kept rows
            results = [reg.decode_ransac_result(host[p], int(used[p])) for p in range(batch.P)]
            if its is not None:
                for p in range(batch.P):
                    results[p].iterations = int(its[p])
        else:
            Th = host.numpy().astype(np.float64)
            results = [reg.RegistrationResult(Th[p], 0.0, 0.0) for p in range(batch.P)]
        # isolate_failures: a dropped pair's result - the failed record (T all NaN, fitness 0, no inliers, best_hypothesis -1) with the
        # pair's DROPPED_* bits in ``status``
        if self.cfg.isolate_failures:
            for p in np.flatnonzero(batch.dropped):
                results[p] = reg.RegistrationResult(np.full((4, 4), np.nan), 0.0, 0.0, status=int(batch.dropped[p]))
        if status:
            for r in results:
                r.status |= status
        return results

    def _range_snapshot(self):
        """The range guard's words on their way to pinned memory, enqueued IN FRONT of the result read-back: the read-back's own
        synchronisation then covers them, and a clean step needs no second host wait (``check_range`` is a copy + a stream
        synchronisation of its own: 35 us of a single pair's 1.5 ms)."""
        if self._range_words is None:
            self._range_words = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.model.range_snapshot(self._range_words)
        return self._range_words

    def _match_and_register_sc2(self, step, seed):
        """SC2-PCR path (scripts/test_kitti.py:179-181) on the CURRENT stream -> ``T f32 [P,4,4]`` on the device.
        Matcher.estimator re-samples both clouds to num_node with replacement, matches them and registers the matched pairs.
        Same draws (pair by pair from one seeded RandomState, source before target) and the same arithmetic as a per-pair loop
        over ``matcher.estimator``, but no per-pair device work: ONE index upload, row gathers, one segmented nearest-neighbour
        launch and one batched SC2-PCR call for all pairs.  The host draws overlap the forward, which is still running.

        The 8000 draws of a pair hold only ~4000 distinct rows of either cloud, and a duplicated target ties with itself
        exactly - such rows (60 %) fall through the MFMA pre-filter into the exact pass (2.3 of the step's 18 ms on 16 pairs).  So the
        neighbour search runs on the DISTINCT rows (``distinct_draws``), and every draw of a source row takes the result of its row.
        Identical indices (``tests/test_gpu_sc2pcr.py`` compares with the per-pair estimator), a quarter of the products."""
        batch, F, m = step.batch, step.F, self.matcher
        n, P, dev = batch.n_points, batch.P, F.device
        F0, F1 = self._sampled_halves(step)
        rng = np.random.RandomState(seed)
        # isolate_failures: the per-pair arrays hold the live pairs only, back to back (``L`` of them; live pair ``p`` is block ``q``);
        # the draws are still made for all P, so that a live pair's do not depend on who was dropped, and the back-end gets an empty
        # segment for a dropped pair.  Without dropped pairs ``q == p`` and ``L == P``.
        live = np.flatnonzero(batch.dropped == 0)
        L = len(live)
        if m.num_node == 'all':
            nn_pts = n
            src_k, tgt_k = batch.xyz0.reshape(-1, 3), batch.xyz1.reshape(-1, 3)
            seg = np.arange(L + 1) * nn_pts
            nn = knn1_segmented(F0, F1, seg, seg, "GemmL2", return_distance=False)      # match_pair's own formula
            self._matched(step)
            nn = nn + torch.arange(L, device=dev).repeat_interleave(nn_pts) * nn_pts     # local -> packed target row
        else:
            nn_pts = int(m.num_node)
            # RandomState.choice(n, k) IS randint(0, n, k) on the same stream, and one call for all pairs draws what the per-pair
            # calls of Matcher.match_pair draw one after the other (source before target; tests/test_gpu_sc2pcr.py compares)
            draws = rng.randint(0, n, (P, 2, nn_pts)).astype(np.int64, copy=False)
            us, ut, inv, first, seg_a, seg_b, base_u = distinct_draws(draws, live, n)
            if L < P:
                draws = draws[live]                       # the dropped pairs' draws stay out of the upload
            draws += (np.arange(L, dtype=np.int64) * n)[:, None, None]
            parts = [draws[:, 0].reshape(-1), draws[:, 1].reshape(-1), inv, us, ut, first, base_u]
            cuts = np.cumsum([0] + [len(a) for a in parts])
            # ONE upload, from pinned memory: a copy from pageable memory blocks the host until everything enqueued on this stream
            # before it is done - with two steps in flight that is the previous step's whole SC2-PCR (the steps then run one after
            # the other however they were enqueued)
            stage = self._pinned_stage(step.slot, int(cuts[-1]))
            np.concatenate(parts, out=stage.numpy()[:cuts[-1]])
            packed = stage[:cuts[-1]].to(dev, non_blocking=True)
            gsi_d, gti_d, inv_d, us_d, ut_d, first_d, base_d = (packed[cuts[k]:cuts[k + 1]] for k in range(7))
            src_k = batch.xyz0.reshape(-1, 3).index_select(0, gsi_d)
            tgt_k = batch.xyz1.reshape(-1, 3).index_select(0, gti_d)
            nn_u = knn1_segmented(gather_rows(F0, us_d), gather_rows(F1, ut_d), seg_a, seg_b, "GemmL2", return_distance=False)
            self._matched(step)
            # distinct source row -> first draw (packed row of tgt_k) of its nearest distinct target; then every draw of that row
            nn = first_d.index_select(0, nn_u + base_d).index_select(0, inv_d)
        keep = min(nn_pts, int(m.max_points))                                            # SC2_PCR.py:318-319 truncation
        tgt_m = tgt_k.index_select(0, nn)
        if keep < nn_pts:
            src_k = src_k.reshape(L, nn_pts, 3)[:, :keep].reshape(-1, 3)
            tgt_m = tgt_m.reshape(L, nn_pts, 3)[:, :keep].reshape(-1, 3)
        with self._accept_degenerate(dev):
            T, _, _ = m.SC2_PCR_packed(src_k.contiguous(), tgt_m.contiguous(), live_segments(batch.dropped, keep))
        if self.cfg.icp_refine:
            T = self._icp_refine(step, T.reshape(-1, 16)).reshape(-1, 4, 4)
        return T

    def correspondence_inlier_ratio(self, batch: DeviceBatch, nn_idx=None, thresh=None):
        """Diagnostic (outside the timed path): per pair, the fraction of the feature correspondences of the last
        RANSAC-path ``register`` whose ground-truth residual ``|T_gt x0 - x1|`` is below ``thresh`` (default: the
        RANSAC distance threshold).  Under ``isolate_failures`` pass the batch the step ran on (``registered_batch``); a dropped
        pair's ratio is NaN."""
        nn_idx = self.last_nn_idx if nn_idx is None else nn_idx
        thresh = self.cfg.voxel_size if thresh is None else thresh
        n = batch.n_points
        nn = nn_idx.cpu().numpy().reshape(-1, n)                     # the live pairs' rows, back to back
        x0, x1 = batch.xyz0.cpu().numpy(), batch.xyz1.cpu().numpy()
        out, q = [], 0
        for p in range(batch.P):
            if batch.dropped[p]:                                     # a dropped pair has no correspondences
                out.append(float("nan"))
                continue
            T = batch.T_gt[p].astype(np.float64)
            r = x0[q].astype(np.float64) @ T[:3, :3].T + T[:3, 3] - x1[q][nn[q]]
            out.append(float((np.linalg.norm(r, axis=1) < thresh).mean()))
            q += 1
        return out

    def evaluate(self, batch: DeviceBatch, results):
        """RTE / RRE / success per pair (scripts/test_kitti.py:187-211)."""
        rows = []
        for p, r in enumerate(results):
            if r.status & DROPPED:                                   # a dropped pair: a failure, and no errors to compute on NaN
                rows.append({"rte": float("nan"), "rre_deg": float("nan"), "success": False})
                continue
            rte, rre, ok = registration_errors(r.transformation.astype(np.float32), batch.T_gt[p],
                                               self.cfg.rte_thresh, self.cfg.rre_thresh)
            rows.append({"rte": rte, "rre_deg": float(np.rad2deg(rre)), "success": ok})
        return rows
