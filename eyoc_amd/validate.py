"""The validation pass of the reference (``lib/trainer.py:321-403``, ``_valid_epoch``), batched.

The reference validates one pair per iteration, half of it on the host: two forwards, ``find_corr``, ``est_quad_linear_robust``,
``corr_dist``, RTE / RRE and ``evaluate_hit_ratio``, with a read-back per number.  Here ``P`` pairs share the sampled forward and one
segmented nearest-neighbour launch, then one ``eyoc_irls_quad_batched`` and one ``eyoc_valid_metrics_batched`` call (a launch per 64
pairs each) leave one 64-byte record per pair on the device, and ONE read-back brings the ``[P, 64]`` records to the host.

Two deliberate deviations from the reference:
  * the 5000-row sample sets are ``DeviceBatch``'s seeded draws (``harness.sample_indices``), where ``find_corr`` calls the global
    ``np.random.choice``;
  * ``pcd0=None`` averages ``corr_dist`` over the pair's SAMPLE set ``batch.xyz0``; the reference averages it over the full cloud
    ``input_dict['pcd0']``, which a caller passes as ``pcd0``.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .eval import _cuda_f32, knn1_segmented
from .metrics import AverageMeter
from .transform_estimation import _segments, est_quad_linear_robust_batched

EMPTY, BAD_INDEX, POSE_NONFINITE = 1, 2, 4        # eyoc_valid_record.status
RECORD_BYTES = C.sizeof(_lib.ValidRecord)         # 64
RECORD_DTYPE = np.dtype([("loss", "<f8"), ("hit_ratio", "<f8"), ("rte", "<f8"), ("rre", "<f8"), ("cos_rre", "<f8"), ("hits", "<i4"),
                         ("n_corr", "<i4"), ("n_points", "<i4"), ("status", "<u4"), ("reserved", "<f8")])
assert RECORD_DTYPE.itemsize == RECORD_BYTES == 64


def valid_metrics_batched(P0, P1, seg0, seg1, idx1, X0, segx, T_est, T_gt, hit_thresh=0.1, max_dist=1.0):
    """The metrics of ``_valid_epoch`` for every pair of a batch (``eyoc_valid_metrics_batched``) -> ``uint8 [P, 64]`` on the device,
    one ``eyoc_valid_record`` per pair (``decode_valid_records``); nothing is read back.

    ``P0 / P1 / seg0 / seg1 / idx1``: the correspondences, as ``est_quad_linear_robust_batched`` takes them.  ``X0 [*, 3]`` with
    ``segx``: the pairs' full source clouds, ``corr_dist`` runs over them.  ``T_est``: ``f32 [P, 4, 4]``, on the device where the IRLS
    call left it; ``T_gt``: the same shape, host or device.  ``hit_thresh``: the reference's ``hit_ratio_thresh``; ``max_dist``:
    ``corr_dist``'s clamp."""
    p0 = _cuda_f32(P0).reshape(-1, 3)
    p1 = _cuda_f32(P1, p0.device).reshape(-1, 3)
    x0 = _cuda_f32(X0, p0.device).reshape(-1, 3)
    s0, seg0 = _segments(seg0, p0.shape[0], "valid_metrics_batched (seg0)")
    s1, seg1 = _segments(seg0 if seg1 is None else seg1, p1.shape[0], "valid_metrics_batched (seg1)")
    sx, segx = _segments(segx, x0.shape[0], "valid_metrics_batched (segx)")
    P = len(seg0) - 1
    if len(seg1) != P + 1 or len(segx) != P + 1:
        raise ValueError("seg0, seg1 and segx must list the same number of pairs")
    if idx1 is not None:
        idx1 = idx1.to(p0.device, torch.int64).contiguous().reshape(-1)
        if idx1.numel() != p0.shape[0]:
            raise ValueError("idx1 must have one entry per row of P0")
    Te = _cuda_f32(T_est, p0.device).reshape(-1, 16)
    Tg = _cuda_f32(T_gt, p0.device).reshape(-1, 16)
    if Te.shape[0] != P or Tg.shape[0] != P:
        raise ValueError(f"{Te.shape[0]} estimated and {Tg.shape[0]} ground-truth poses for {P} pairs")
    rec = torch.empty((P, RECORD_BYTES), dtype=torch.uint8, device=p0.device)
    with _lib.on_device(p0.device):
        _lib.check(_lib.load().eyoc_valid_metrics_batched(_lib.ctx(p0.device.index), _lib.ptr(p0), _lib.ptr(p1), _lib.ptr(idx1), s0, s1,
                                                          _lib.ptr(x0), sx, P, _lib.ptr(Te), _lib.ptr(Tg), float(hit_thresh), float(max_dist),
                                                          _lib.ptr(rec), _lib.stream_ptr()), "eyoc_valid_metrics_batched")
    return rec


def decode_valid_records(raw):
    """``[P, 64]`` record bytes (a device or host tensor, a numpy array, or ``bytes``) -> a numpy structured array ``[P]`` with the fields
    of ``eyoc_valid_record``: ``loss, hit_ratio, rte, rre, cos_rre`` (f8), ``hits, n_corr, n_points`` (i4), ``status`` (u4), ``reserved``."""
    if isinstance(raw, torch.Tensor):
        raw = raw.cpu().numpy()
    if isinstance(raw, np.ndarray):
        raw = np.ascontiguousarray(raw).tobytes()
    raw = bytes(raw)
    if len(raw) % RECORD_BYTES:
        raise ValueError(f"{len(raw)} bytes are no whole number of {RECORD_BYTES}-byte records")
    return np.frombuffer(raw, dtype=RECORD_DTYPE).copy()


class ValidMeters:
    """The five ``AverageMeter``s of ``_valid_epoch`` (lib/trainer.py:326-327), fed with records.  A NaN ``rre`` is left out of the ``rre``
    mean only (:369-370); a pair without correspondences (EMPTY: dropped from its batch, or an empty segment) or with a BAD_INDEX has no
    hit ratio - it is left out of every mean and counted in ``skipped``."""
    KEYS = ("loss", "rre", "rte", "feat_match_ratio", "hit_ratio")

    def __init__(self):
        self.meters = {k: AverageMeter() for k in self.KEYS}
        self.skipped = 0
        self.count = 0

    def update(self, records):
        for r in np.atleast_1d(records):
            if int(r["status"]) & (EMPTY | BAD_INDEX):
                self.skipped += 1
                continue
            self.count += 1
            self.meters["loss"].update(float(r["loss"]))
            self.meters["rte"].update(float(r["rte"]))
            if not np.isnan(r["rre"]):
                self.meters["rre"].update(float(r["rre"]))
            self.meters["hit_ratio"].update(float(r["hit_ratio"]))
            self.meters["feat_match_ratio"].update(float(r["hit_ratio"] > 0.05))     # strictly above, :378

    def summary(self):
        """The dict ``_valid_epoch`` returns (:397-403)."""
        return {k: self.meters[k].avg for k in self.KEYS}


class ValidStep(NamedTuple):
    """What ``valid_step`` returns."""
    records: np.ndarray        # structured [P] (``decode_valid_records``)
    T_est: torch.Tensor        # f32 [P, 4, 4] on the device; NaN for a pair without correspondences
    nn_idx: torch.Tensor       # int64, the feature correspondences of the live pairs (local to the pair's sample set)
    batch: object              # the batch the step ran on (``isolate_failures``: without the pairs that failed the map build)


def _full_clouds(pcd0, batch, device):
    """``pcd0`` -> (packed ``f32 [*, 3]`` on the device, segments ``[P + 1]``): ``None`` = the pairs' sample sets; a list of ``P`` clouds
    ``[N_b, 3]``; or the tuple ``(packed, seg)``."""
    if pcd0 is None:
        return batch.xyz0.reshape(-1, 3), batch.seg
    if isinstance(pcd0, tuple):
        x0, seg = pcd0
        return _cuda_f32(x0, device).reshape(-1, 3), [int(v) for v in seg]
    clouds = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(c, np.float32))) for c in pcd0]
    if len(clouds) != batch.P:
        raise ValueError(f"pcd0 holds {len(clouds)} clouds for {batch.P} pairs")
    seg = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    return _cuda_f32(torch.cat([c.reshape(-1, 3).to(torch.float32) for c in clouds]), device), seg


@torch.no_grad()
def valid_step(pipe, batch, pcd0=None, hit_ratio_thresh=0.1, maps=None) -> ValidStep:
    """One iteration body of ``_valid_epoch`` (lib/trainer.py:340-378) for all ``P`` pairs of ``batch``: the sampled forward
    (``model(x, rows=)``), the descriptor blend if the batch has one, ``knn1_segmented`` on ``batch.seg``, ``eyoc_irls_quad_batched`` and
    ``eyoc_valid_metrics_batched`` on ``batch.xyz0 / xyz1 / nn_idx / T_gt``, then ONE read-back of the ``[P, 64]`` records.

    ``pcd0``: the pairs' full source clouds (the reference's ``input_dict['pcd0']``) as a list of ``P`` ``[N_b, 3]`` arrays or as
    the tuple ``(packed [*, 3], seg [P + 1])``.  DEVIATION: ``None`` uses the pair's sample set ``batch.xyz0`` instead of the full cloud.
    DEVIATION: the sample draws are ``DeviceBatch``'s seeded ones; the reference draws with ``np.random.choice`` (``find_corr``).
    Under ``isolate_failures`` a dropped pair is an empty segment: its record is EMPTY and its pose NaN."""
    from .harness import _Step
    step = _Step(0, None)
    step.F, step.batch = pipe._features(batch, maps, sampled=True)
    b = step.batch
    F0, F1 = pipe._sampled_halves(step)
    dev = step.F.device
    nn_idx = knn1_segmented(F0, F1, b.seg, b.seg, "SquareL2", return_distance=False)
    xyz0, xyz1 = b.xyz0.reshape(-1, 3), b.xyz1.reshape(-1, 3)
    T_est = est_quad_linear_robust_batched(xyz0, xyz1, b.seg, b.seg, idx1=nn_idx)
    x0, segx = _full_clouds(pcd0, b, dev)
    T_gt = torch.from_numpy(np.stack([np.asarray(T, np.float32).reshape(4, 4) for T in b.T_gt])).to(dev, non_blocking=True)
    rec = valid_metrics_batched(xyz0, xyz1, b.seg, b.seg, nn_idx, x0, segx, T_est, T_gt, hit_ratio_thresh)
    words = pipe._range_snapshot()       # the split16 guard's verdict rides in front of the read-back, like ``register``'s
    host = rec.cpu()
    if int(words[0]) != 0 or int(words[3]) != 0:
        try:
            pipe.model.check_range()
        except _lib.EyocError as e:
            if e.code != _lib.ERR_RANGE or pipe.model.spconv_math != "auto":
                raise
            logging.warning("eyoc_amd: split16 overflow in the validation step; switching the model to fp32 MFMAs")
            pipe.model.spconv_math = "fp32"
            return valid_step(pipe, batch, pcd0, hit_ratio_thresh, maps)
    return ValidStep(decode_valid_records(host), T_est, nn_idx, b)


def valid_epoch(pipe, batches, pcd0=None, hit_ratio_thresh=0.1, meters=None):
    """``_valid_epoch`` over an iterable of ``DeviceBatch``es -> the reference's dict (``loss, rre, rte, feat_match_ratio, hit_ratio``).
    ``pcd0``: ``None``, or a callable ``pcd0(k, batch)`` giving batch ``k``'s full source clouds (see ``valid_step``).  ``meters``: a
    ``ValidMeters`` to feed (its ``skipped`` then counts the pairs left out)."""
    meters = ValidMeters() if meters is None else meters
    for k, batch in enumerate(batches):
        meters.update(valid_step(pipe, batch, None if pcd0 is None else pcd0(k, batch), hit_ratio_thresh).records)
    return meters.summary()
