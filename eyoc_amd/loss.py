"""The hardest-contrastive loss of EYOC's trainer (lib/trainer.py:935-991) and its gradient in one device pass.

``hardest_contrastive_loss`` is ``autograd.contrastive_hardest_negative_loss`` with the same draws and the same value, as ONE autograd
node on ``eyoc_hcloss_forward`` / ``eyoc_hcloss_backward`` (csrc/loss.hip): the positives may be a device tensor and then never leave
the device (the label stages produce them there), the three host draws go up in one asynchronous copy, nothing is read back, the
number of launches is fixed (5 + 4) and the gradient rows are summed in a fixed order without floating-point atomics - their bytes do
not change from run to run.  The existing function stays; this route is opt-in.

Every loss here takes ``rng=DeviceDraws(seed)`` (eyoc_amd/draws.py) beside ``None``, a ``RandomState`` or a ``Generator``: the draws are
then made on the device by a counter-based generator, in the reference's order of slots, and handed straight to the same autograd
nodes - no host permutation, no staging buffer, one ``subsets`` or one ``pairs`` call per loss call.  With any other ``rng`` nothing
changes.

``triplet_loss`` / ``hardest_triplet_loss`` (second half of the file) are the losses of the reference's other two trainers
(lib/trainer.py:567-621, :701-782) on ``eyoc_triplet_forward`` / ``eyoc_triplet_backward``, built the same way.

``contrastive_loss`` (last part) is the loss of the base trainer, ``ContrastiveLossTrainer`` (lib/trainer.py:201-221, :262-286): all
positives against random negatives, on ``eyoc_closs_forward`` / ``eyoc_closs_backward``."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .autograd import _draw_loss_samples
from .draws import DeviceDraws

BAD_INDEX, MASKED, VALID = 1, 1, 2        # record status bit; per-direction flag bits (include/eyoc_hip.h)
_RECORD_FLOATS = C.sizeof(_lib.HclossRecord) // 4


# The call plumbing of the three losses; ``name`` is the prefix of a loss's C symbols (``eyoc_hcloss``, ``eyoc_triplet``, ``eyoc_closs``).
def _layout(name, struct, *shape):
    out = struct()
    _lib.check(getattr(_lib.load(), name + "_workspace_layout")(*shape, C.byref(out)), name + "_workspace_layout")
    return out


def _forward(name, record_floats, shape, args, F0):
    """``<name>_forward`` with a workspace of ``<name>_workspace_bytes(*shape)`` -> ``(record, workspace)``; ``args``: the C arguments up
    to the record."""
    lib = _lib.load()
    with _lib.on_device(F0.device):
        ws = _lib.workspace(getattr(lib, name + "_workspace_bytes")(*shape), F0.device)
        rec = torch.empty(record_floats, dtype=torch.float32, device=F0.device)
        _lib.check(getattr(lib, name + "_forward")(*args, _lib.ptr(rec), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), name + "_forward")
    return rec, ws


def _backward(name, args, F0, F1, grads, ws):
    """``<name>_backward`` -> ``(dF0, dF1)``; ``args``: the C arguments up to the upstream gradients ``grads``."""
    lib = _lib.load()
    dF0, dF1 = torch.empty_like(F0), torch.empty_like(F1)
    with _lib.on_device(F0.device):
        _lib.check(getattr(lib, name + "_backward")(*args, *[_lib.ptr(g) for g in grads], _lib.ptr(dF0), _lib.ptr(dF1), _lib.ptr(ws),
                                                    ws.numel(), _lib.stream_ptr()), name + "_backward")
    return dF0, dF1


def _read(rec, struct):
    return struct.from_buffer_copy(rec.detach().cpu().numpy().tobytes())


def _view(ws, off, count, dtype):
    return ws[off:off + 4 * count].view(dtype)


def _scalar(g, device):
    """An upstream gradient as a float32 device scalar; a missing one is zero."""
    if g is None:
        return torch.zeros((), dtype=torch.float32, device=device)
    return g.to(torch.float32).contiguous()


def _upload_draws(parts, dev):
    """The host draws of a loss call: one pinned staging buffer, one asynchronous copy -> the parts as slices of the device copy."""
    stage = torch.empty(sum(len(p) for p in parts), dtype=torch.int64, pin_memory=True)
    host, bounds, at = stage.numpy(), [], 0
    for p in parts:
        host[at:at + len(p)] = p
        bounds.append((at, at + len(p)))
        at += len(p)
    draws = stage.to(dev, non_blocking=True)
    return [draws[a:b] for a, b in bounds]


class _Node(torch.autograd.Function):
    """The backward of the three nodes.  A subclass's forward saves ``(F0, F1)`` and leaves in ``ctx.call`` its raw backward, that
    function's arguments between the features and the gradients (the node's other inputs) and the number of gradients it takes."""

    @staticmethod
    def backward(ctx, *grads):
        F0, F1 = ctx.saved_tensors
        raw_backward, rest, n_grads = ctx.call
        dF0, dF1 = raw_backward(F0, F1, *rest, *[_scalar(g, F0.device) for g in grads[:n_grads]], ctx.ws)
        return (dF0, dF1) + (None,) * len(rest)


def layout(n_pairs, n_used, s0, s1, c):
    return _layout("eyoc_hcloss", _lib.HclossLayout, n_pairs, n_used, s0, s1, c)


def _args(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh):
    n_used = pairs.shape[0] if used is None else used.shape[0]
    return (_lib.ctx(F0.device.index), _lib.ptr(F0), F0.shape[0], _lib.ptr(F1), F1.shape[0], F0.shape[1], _lib.ptr(pairs), pairs.shape[0],
            _lib.ptr(used), n_used, _lib.ptr(sel0), sel0.shape[0], _lib.ptr(sel1), sel1.shape[0], float(pos_thresh), float(neg_thresh))


def _check_inputs(F0, F1, pairs, used, sel0, sel1):
    for t in (F0, F1):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda:
            raise _lib.EyocError("hardest-contrastive loss: features must be contiguous float32 [n, c] device tensors", _lib.ERR_INVALID)
    if F0.shape[1] != F1.shape[1]:
        raise _lib.EyocError("hardest-contrastive loss: F0 and F1 differ in width", _lib.ERR_INVALID)
    for t in (pairs, used, sel0, sel1):
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous() or t.device != F0.device):
            raise _lib.EyocError("hardest-contrastive loss: index arrays must be contiguous int64 tensors on the features' device",
                                 _lib.ERR_INVALID)
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise _lib.EyocError("hardest-contrastive loss: positive pairs must be [n, 2]", _lib.ERR_INVALID)


def forward_raw(F0, F1, pairs, used, sel0, sel1, pos_thresh=0.1, neg_thresh=1.4):
    """``eyoc_hcloss_forward`` on device tensors -> ``(record, workspace)``: ``record`` a float32 view of the 48-byte
    ``eyoc_hcloss_record`` (``record[10]`` = pos_loss, ``record[11]`` = neg_loss; ``read_record`` decodes all of it), ``workspace`` what
    ``backward_raw`` and ``results`` read.  ``used = None`` takes every positive."""
    _check_inputs(F0, F1, pairs, used, sel0, sel1)
    n_used = pairs.shape[0] if used is None else used.shape[0]
    return _forward("eyoc_hcloss", _RECORD_FLOATS, (pairs.shape[0], n_used, sel0.shape[0], sel1.shape[0], F0.shape[1]),
                    _args(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh), F0)


def backward_raw(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh, g_pos, g_neg, ws):
    """``eyoc_hcloss_backward`` -> ``(dF0, dF1)``; ``g_pos`` / ``g_neg`` float32 device scalars, ``ws`` from ``forward_raw`` on the same arguments."""
    return _backward("eyoc_hcloss", _args(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh), F0, F1, (g_pos, g_neg), ws)


def read_record(rec) -> _lib.HclossRecord:
    """The record on the host (tests, logging): this READS BACK, the loss itself never does."""
    return _read(rec, _lib.HclossRecord)


def results(ws, n_pairs, n_used, s0, s1, c):
    """The per-positive results the forward left in its workspace, as device views: ``tstar`` int32 [2, n_used] (-1: none), ``dist``
    float32 [2, n_used], ``pos_d2`` float32 [n_used], ``flags`` int32 [2, n_used] (``MASKED`` / ``VALID``); row 0 is direction 01."""
    lay = layout(n_pairs, n_used, s0, s1, c)
    return {"tstar": _view(ws, lay.off_tstar, 2 * n_used, torch.int32).view(2, n_used),
            "dist": _view(ws, lay.off_dist, 2 * n_used, torch.float32).view(2, n_used),
            "pos_d2": _view(ws, lay.off_pos_d2, n_used, torch.float32),
            "flags": _view(ws, lay.off_flags, 2 * n_used, torch.int32).view(2, n_used)}


class _HardestContrastive(_Node):
    @staticmethod
    def forward(ctx, F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh):
        rec, ws = forward_raw(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh)
        ctx.save_for_backward(F0, F1)
        ctx.call, ctx.ws = (backward_raw, (pairs, used, sel0, sel1, pos_thresh, neg_thresh), 2), ws
        return rec[_RECORD_FLOATS - 2], rec[_RECORD_FLOATS - 1]


def hardest_contrastive_loss(F0, F1, positive_pairs, num_pos=5192, num_hn_samples=2048, pos_thresh=0.1, neg_thresh=1.4, rng=None):
    """lib/trainer.py:935-991 -> ``(pos_loss, neg_loss)``, 0-dim tensors with grad, the values of
    ``autograd.contrastive_hardest_negative_loss`` for the same ``rng`` (the three draws are the same function, in the reference's order).

    ``positive_pairs``: a DEVICE int64 ``[n, 2]`` tensor stays on the device; a host tensor or ndarray costs one upload.  No double
    backward; ``c`` in {16, 32, 64}."""
    dev = F0.device
    pairs = _device_pairs(positive_pairs, dev)
    n0, n1, n_pairs = F0.shape[0], F1.shape[0], pairs.shape[0]
    if isinstance(rng, DeviceDraws):
        # slots in the reference's order: candidates of cloud 0, of cloud 1, the positive sub-sample (an empty slot when all are kept)
        sel0, sel1, used = rng.subsets([(n0, min(n0, num_hn_samples)), (n1, min(n1, num_hn_samples)),
                                        (n_pairs, num_pos) if n_pairs > num_pos else (0, 0)], device=dev)
        return _HardestContrastive.apply(F0.contiguous(), F1.contiguous(), pairs, used if n_pairs > num_pos else None, sel0, sel1,
                                         float(pos_thresh), float(neg_thresh))
    cand0, cand1, keep = _draw_loss_samples(np.random if rng is None else rng, n0, n1, n_pairs, num_hn_samples, num_pos)
    sel0, sel1, *used = _upload_draws([cand0, cand1] + ([] if keep is None else [keep]), dev)
    return _HardestContrastive.apply(F0.contiguous(), F1.contiguous(), pairs, used[0] if used else None, sel0, sel1, float(pos_thresh),
                                     float(neg_thresh))


# ------------------------------------------------------------------------------------------------------------------------------------
# Triplet and hardest-triplet loss (lib/trainer.py:567-621 and :701-782) on eyoc_triplet_forward / eyoc_triplet_backward: one autograd
# node, 5 launches forward, 4 and one radix sort backward; the gradient rows are summed per destination row from a sorted contribution
# list (linear in the number of contributions), in a fixed order, without floating-point atomics.
TRIPLET_BAD_INDEX, TRIPLET_MASKED, TRIPLET_VALID, TRIPLET_ACTIVE = 1, 1, 2, 4
_TRIPLET_FLOATS = C.sizeof(_lib.TripletRecord) // 4
_TRIPLET_LOSS = _lib.TripletRecord.loss.offset // 4          # loss, pos_dist_mean, neg_dist_mean follow each other


def triplet_layout(n_pairs, n_used, s0, s1, n_rand, c):
    return _layout("eyoc_triplet", _lib.TripletLayout, n_pairs, n_used, s0, s1, n_rand, c)


def _triplet_args(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, margin):
    n_used = pairs.shape[0] if used is None else used.shape[0]
    return (_lib.ctx(F0.device.index), _lib.ptr(F0), F0.shape[0], _lib.ptr(F1), F1.shape[0], F0.shape[1], _lib.ptr(pairs), pairs.shape[0],
            _lib.ptr(used), n_used, _lib.ptr(sel0), sel0.shape[0], _lib.ptr(sel1), sel1.shape[0], _lib.ptr(rand_idx), _lib.ptr(negatives),
            rand_idx.shape[0], float(margin))


def check_triplet_lengths(n_pairs, n1, num_rand_triplet):
    """The reference adds the random triplets' anchors and negatives element-wise (``_hash``) and raises a broadcast ``ValueError``
    unless both draws have one length; so does this, before anything is drawn or enqueued."""
    a, b = min(n_pairs, num_rand_triplet), min(n1, num_rand_triplet)
    if a != b:
        raise ValueError(f"triplet loss: {a} random (anchor, positive) pairs = min(n_pairs {n_pairs}, num_rand_triplet {num_rand_triplet}) "
                         f"but {b} random negatives = min(N1 {n1}, num_rand_triplet): the reference cannot broadcast them either")


def draw_triplet_samples(rng, n0, n1, n_pairs, num_hn_samples, num_pos, num_rand_triplet):
    """The reference's draws in the reference's order -> ``(sel0, sel1, used, rand_idx, negatives)``: the two candidate sets only with
    ``num_hn_samples`` (HardestTripletLossTrainer, :715-716; ``None``: empty), the positive sub-sample only if ``n_pairs > num_pos``
    (``None`` otherwise), then the random triplets' pairs and negatives."""
    check_triplet_lengths(n_pairs, n1, num_rand_triplet)
    empty = np.zeros(0, np.int64)
    sel0 = sel1 = empty
    if num_hn_samples is not None:
        sel0 = rng.choice(n0, min(n0, num_hn_samples), replace=False)
        sel1 = rng.choice(n1, min(n1, num_hn_samples), replace=False)
    used = rng.choice(n_pairs, num_pos, replace=False) if n_pairs > num_pos else None
    rand_idx = rng.choice(n_pairs, min(n_pairs, num_rand_triplet), replace=False)
    negatives = rng.choice(n1, min(n1, num_rand_triplet), replace=False)
    return sel0, sel1, used, rand_idx, negatives


def triplet_raw_forward(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, margin=1.4):
    """``eyoc_triplet_forward`` on device tensors -> ``(record, workspace)``: ``record`` a float32 view of the 96-byte
    ``eyoc_triplet_record`` (``read_triplet_record`` decodes it), ``workspace`` what ``triplet_raw_backward`` and ``triplet_results``
    read.  ``used = None`` takes every positive; empty ``sel0`` and ``sel1`` give the plain variant."""
    _check_inputs(F0, F1, pairs, used, sel0, sel1)
    _check_inputs(F0, F1, pairs, None, rand_idx, negatives)
    if rand_idx.shape[0] != negatives.shape[0]:
        raise ValueError(f"triplet loss: {rand_idx.shape[0]} random pairs, {negatives.shape[0]} random negatives")
    n_used = pairs.shape[0] if used is None else used.shape[0]
    return _forward("eyoc_triplet", _TRIPLET_FLOATS, (pairs.shape[0], n_used, sel0.shape[0], sel1.shape[0], rand_idx.shape[0], F0.shape[1]),
                    _triplet_args(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, margin), F0)


def triplet_raw_backward(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, margin, g, ws):
    """``eyoc_triplet_backward`` -> ``(dF0, dF1)``; ``g`` a float32 device scalar, ``ws`` from ``triplet_raw_forward`` on the same arguments."""
    return _backward("eyoc_triplet", _triplet_args(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, margin), F0, F1, (g,), ws)


def read_triplet_record(rec) -> _lib.TripletRecord:
    """The record on the host (tests, logging): this READS BACK, the loss itself never does."""
    return _read(rec, _lib.TripletRecord)


def triplet_results(ws, n_pairs, n_used, s0, s1, n_rand, c):
    """The per-term results the forward left in its workspace, as device views: ``tstar`` int32 [2, n_used] (-1: none), ``dist`` (d01,
    d10), ``term`` float32 [2, n_used], ``pos_dist`` float32 [n_used], ``flags`` int32 [2, n_used] (``TRIPLET_MASKED`` / ``_VALID`` /
    ``_ACTIVE``; row 0 is direction 01); ``rand_pos``, ``rand_neg``, ``rand_term`` float32 [n_rand], ``rand_flags`` int32 [n_rand];
    ``contrib_key`` int32 [3 (n_rand + 2 n_used)], written by the backward (2 row + matrix + 1, 0 = empty)."""
    lay = triplet_layout(n_pairs, n_used, s0, s1, n_rand, c)
    out = {"tstar": _view(ws, lay.off_tstar, 2 * n_used, torch.int32).view(2, n_used),
           "dist": _view(ws, lay.off_dist, 2 * n_used, torch.float32).view(2, n_used),
           "term": _view(ws, lay.off_term, 2 * n_used, torch.float32).view(2, n_used),
           "pos_dist": _view(ws, lay.off_pos_dist, n_used, torch.float32),
           "flags": _view(ws, lay.off_flags, 2 * n_used, torch.int32).view(2, n_used),
           "rand_flags": _view(ws, lay.off_rand_flags, n_rand, torch.int32),
           "contrib_key": _view(ws, lay.off_contrib_key, lay.n_contrib, torch.int32)}
    for k in ("pos", "neg", "term"):
        out["rand_" + k] = _view(ws, getattr(lay, "off_rand_" + k), n_rand, torch.float32)
    return out


class _Triplet(_Node):
    @staticmethod
    def forward(ctx, F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, margin):
        rec, ws = triplet_raw_forward(F0, F1, pairs, used, sel0, sel1, rand_idx, negatives, margin)
        ctx.save_for_backward(F0, F1)
        ctx.call, ctx.ws = (triplet_raw_backward, (pairs, used, sel0, sel1, rand_idx, negatives, margin), 1), ws
        loss, pos, neg = rec[_TRIPLET_LOSS], rec[_TRIPLET_LOSS + 1], rec[_TRIPLET_LOSS + 2]
        ctx.mark_non_differentiable(pos, neg)
        return loss, pos, neg


def _triplet(F0, F1, positive_pairs, num_pos, num_hn_samples, num_rand_triplet, neg_thresh, rng):
    dev = F0.device
    pairs = _device_pairs(positive_pairs, dev)
    n0, n1, n_pairs = F0.shape[0], F1.shape[0], pairs.shape[0]
    if isinstance(rng, DeviceDraws):
        check_triplet_lengths(n_pairs, n1, num_rand_triplet)           # before anything is drawn or enqueued, as on the host route
        hn = 0 if num_hn_samples is None else num_hn_samples
        # slots in the reference's order (draw_triplet_samples); a draw the variant does not make keeps its slot, empty
        sel0, sel1, used, rand_idx, negatives = rng.subsets([(n0, min(n0, hn)), (n1, min(n1, hn)),
                                                             (n_pairs, num_pos) if n_pairs > num_pos else (0, 0),
                                                             (n_pairs, min(n_pairs, num_rand_triplet)), (n1, min(n1, num_rand_triplet))],
                                                            device=dev)
        return _Triplet.apply(F0.contiguous(), F1.contiguous(), pairs, used if n_pairs > num_pos else None, sel0, sel1, rand_idx, negatives,
                              float(neg_thresh))
    sel0, sel1, used, rand_idx, negatives = draw_triplet_samples(np.random if rng is None else rng, n0, n1, n_pairs, num_hn_samples,
                                                                 num_pos, num_rand_triplet)
    d = _upload_draws([sel0, sel1, rand_idx, negatives] + ([] if used is None else [used]), dev)
    return _Triplet.apply(F0.contiguous(), F1.contiguous(), pairs, None if used is None else d[4], d[0], d[1], d[2], d[3], float(neg_thresh))


def triplet_loss(F0, F1, positive_pairs, num_pos=1024, num_hn_samples=None, num_rand_triplet=1024, neg_thresh=1.4, rng=None):
    """``TripletLossTrainer.triplet_loss`` (lib/trainer.py:567-621) -> ``(loss, pos_dist_mean, neg_dist_mean)``: ``loss`` a 0-dim tensor
    with grad, the monitors 0-dim device tensors without (``neg_dist_mean``: the kept random triplets' mean negative distance).  The
    draws are the reference's, in its order, from ``rng`` (default: the global ``np.random``); ``num_hn_samples`` is not read, as in the
    reference.  ``positive_pairs`` on the device stays there; nothing is read back.  Raises ``ValueError`` where the reference does:
    ``min(n_pairs, num_rand_triplet) != min(N1, num_rand_triplet)``.  No double backward; ``c`` in {16, 32, 64}."""
    return _triplet(F0, F1, positive_pairs, num_pos, None, num_rand_triplet, neg_thresh, rng)


def hardest_triplet_loss(F0, F1, positive_pairs, num_pos=1024, num_hn_samples=512, num_rand_triplet=1024, neg_thresh=1.4, rng=None):
    """``HardestTripletLossTrainer.triplet_loss`` (lib/trainer.py:701-782): the random triplets plus, per used positive, its hardest
    negative among ``num_hn_samples`` candidates in both directions -> ``(loss, pos_dist_mean, neg_dist_mean)`` as ``triplet_loss``;
    ``neg_dist_mean`` is ``(D01min.mean() + D10min.mean()) / 2`` as a device tensor (the reference's ``.item()`` is the caller's)."""
    return _triplet(F0, F1, positive_pairs, num_pos, int(num_hn_samples), num_rand_triplet, neg_thresh, rng)


# ------------------------------------------------------------------------------------------------------------------------------------
# Random-negative contrastive loss of the base trainer (lib/trainer.py:201-221 and :262-286) on eyoc_closs_forward / eyoc_closs_backward:
# one autograd node, 4 launches forward, 4 and one radix sort backward.  Every positive of the batch is used; the candidate negatives are
# tested against the positives' key table on the device and keep their places (flags, nothing compacted); the gradient rows are summed per
# destination row from a sorted contribution list, in a fixed order, without floating-point atomics.
CLOSS_BAD_INDEX, CLOSS_MASKED, CLOSS_VALID, CLOSS_ACTIVE = 1, 1, 2, 4
_CLOSS_FLOATS = C.sizeof(_lib.ClossRecord) // 4
_CLOSS_POS = _lib.ClossRecord.pos_loss.offset // 4            # pos_loss, neg_loss follow each other


def contrastive_layout(n_pairs, n_neg, c):
    return _layout("eyoc_closs", _lib.ClossLayout, n_pairs, n_neg, c)


def draw_negative_pairs(rng, n_pairs, n0, n1, n_neg=0):
    """The reference's draw (lib/trainer.py:212-218) -> int64 ``[N, 2]`` on the host: ``floor(rand(N, 2) * [[n0, n1]])`` from ONE call,
    row-major, ``N = 2 n_pairs`` when ``n_neg < 1``.  ``rng``: ``np.random`` or a ``RandomState``, as the other losses accept."""
    n = int(n_neg) if n_neg >= 1 else 2 * int(n_pairs)
    return np.floor(rng.rand(n, 2) * np.array([[n0, n1]])).astype(np.int64)


def _contrastive_args(F0, F1, pairs, neg, neg_thresh):
    return (_lib.ctx(F0.device.index), _lib.ptr(F0), F0.shape[0], _lib.ptr(F1), F1.shape[0], F0.shape[1], _lib.ptr(pairs), pairs.shape[0],
            _lib.ptr(neg), neg.shape[0], float(neg_thresh))


def contrastive_raw_forward(F0, F1, pairs, neg, neg_thresh=1.4):
    """``eyoc_closs_forward`` on device tensors -> ``(record, workspace)``: ``record`` a float32 view of the 48-byte
    ``eyoc_closs_record`` (``read_contrastive_record`` decodes it), ``workspace`` what ``contrastive_raw_backward`` and
    ``contrastive_results`` read.  ``pairs`` int64 ``[n_pairs, 2]``: all positives; ``neg`` int64 ``[n_neg, 2]``: the raw candidates."""
    _check_inputs(F0, F1, pairs, None, None, None)
    _check_inputs(F0, F1, neg, None, None, None)
    return _forward("eyoc_closs", _CLOSS_FLOATS, (pairs.shape[0], neg.shape[0], F0.shape[1]),
                    _contrastive_args(F0, F1, pairs, neg, neg_thresh), F0)


def contrastive_raw_backward(F0, F1, pairs, neg, neg_thresh, g_pos, g_neg, ws):
    """``eyoc_closs_backward`` -> ``(dF0, dF1)``; ``g_pos`` / ``g_neg`` float32 device scalars, ``ws`` from ``contrastive_raw_forward``
    on the same arguments."""
    return _backward("eyoc_closs", _contrastive_args(F0, F1, pairs, neg, neg_thresh), F0, F1, (g_pos, g_neg), ws)


def read_contrastive_record(rec) -> _lib.ClossRecord:
    """The record on the host (tests, logging): this READS BACK, the loss itself never does."""
    return _read(rec, _lib.ClossRecord)


def contrastive_results(ws, n_pairs, n_neg, c):
    """The per-term results the forward left in its workspace, as device views: ``pos_d2`` float32 [n_pairs]; ``dist``, ``term`` float32
    [n_neg], ``flags`` int32 [n_neg] (``CLOSS_MASKED`` / ``_VALID`` / ``_ACTIVE``); ``contrib_key`` int32 [2 (n_pairs + n_neg)], written
    by the backward (2 row + matrix + 1, 0 = empty)."""
    lay = contrastive_layout(n_pairs, n_neg, c)
    return {"pos_d2": _view(ws, lay.off_pos_d2, n_pairs, torch.float32), "dist": _view(ws, lay.off_dist, n_neg, torch.float32),
            "term": _view(ws, lay.off_term, n_neg, torch.float32), "flags": _view(ws, lay.off_flags, n_neg, torch.int32),
            "contrib_key": _view(ws, lay.off_contrib_key, lay.n_contrib, torch.int32)}


class _Contrastive(_Node):
    @staticmethod
    def forward(ctx, F0, F1, pairs, neg, neg_thresh):
        rec, ws = contrastive_raw_forward(F0, F1, pairs, neg, neg_thresh)
        ctx.save_for_backward(F0, F1)
        ctx.call, ctx.ws = (contrastive_raw_backward, (pairs, neg, neg_thresh), 2), ws
        return rec[_CLOSS_POS], rec[_CLOSS_POS + 1]


def _device_pairs(positive_pairs, dev):
    if isinstance(positive_pairs, torch.Tensor):
        pairs = positive_pairs
    else:
        pairs = torch.from_numpy(np.ascontiguousarray(np.asarray(positive_pairs), dtype=np.int64))
    return pairs.reshape(-1, 2).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()


def _upload_negatives(neg, dev):
    """One pinned staging buffer, one asynchronous copy."""
    stage = torch.empty((neg.shape[0], 2), dtype=torch.int64, pin_memory=True)
    stage.numpy()[...] = neg
    return stage.to(dev, non_blocking=True)


def _candidate_negatives(rng, n_pairs, n0, n1, n_neg, dev):
    """The candidate negatives on the device: drawn there by a ``DeviceDraws`` (one launch), else the reference's host draw, uploaded."""
    if isinstance(rng, DeviceDraws):
        return rng.pairs(int(n_neg) if n_neg >= 1 else 2 * int(n_pairs), n0, n1, device=dev)
    return _upload_negatives(draw_negative_pairs(np.random if rng is None else rng, n_pairs, n0, n1, n_neg), dev)


def contrastive_loss(F0, F1, positive_pairs, neg_thresh=1.4, n_neg=0, rng=None):
    """``ContrastiveLossTrainer``'s loss (lib/trainer.py:262-286 with the negatives of :201-221) -> ``(pos_loss, neg_loss)``, 0-dim
    tensors with grad: ``pos_loss`` the mean squared distance over ALL positives, ``neg_loss`` the mean of
    ``relu(neg_thresh - sqrt(d2 + 1e-4))^2`` over the random candidates that are no known positive (``2 n_pairs`` candidates when
    ``n_neg < 1``; the draw is the reference's, from ``rng``, default the global ``np.random``).  The caller forms
    ``pos_loss + neg_weight * neg_loss`` and the ``/ iter_size``.

    ``positive_pairs``: a DEVICE int64 ``[n, 2]`` tensor stays on the device; a host tensor or ndarray costs one upload.  The candidates
    go up in one asynchronous copy and are tested against the positives on the device; nothing is read back.  A mean over nothing is
    NaN (no positive: both values).  No double backward; ``c`` in {16, 32, 64}."""
    dev = F0.device
    pairs = _device_pairs(positive_pairs, dev)
    neg = _candidate_negatives(rng, pairs.shape[0], F0.shape[0], F1.shape[0], n_neg, dev)
    return _Contrastive.apply(F0.contiguous(), F1.contiguous(), pairs, neg, float(neg_thresh))


def generate_rand_negative_pairs(positive_pairs, hash_seed, N0, N1, N_neg=0, rng=None):
    """``ContrastiveLossTrainer.generate_rand_negative_pairs`` (lib/trainer.py:201-221) -> the kept negatives in draw order, a device
    int64 ``[k, 2]`` tensor.  For callers that want the list (``contrastive_loss`` never forms it): the membership flags come from
    ``eyoc_closs_forward`` on zero features, and the compaction READS BACK once, for the count.  ``hash_seed`` must be
    ``max(N0, N1)``, the reference's only call and the only value for which the key is exact pair membership."""
    if int(hash_seed) != max(int(N0), int(N1)):
        raise ValueError(f"generate_rand_negative_pairs: hash_seed {hash_seed} != max(N0, N1) = {max(int(N0), int(N1))}")
    on_dev = isinstance(positive_pairs, torch.Tensor) and positive_pairs.is_cuda
    dev = positive_pairs.device if on_dev else torch.device("cuda", torch.cuda.current_device())
    pairs = _device_pairs(positive_pairs, dev)
    neg = _candidate_negatives(rng, pairs.shape[0], int(N0), int(N1), N_neg, dev)
    Z0 = torch.zeros((int(N0), 16), dtype=torch.float32, device=dev)
    Z1 = torch.zeros((int(N1), 16), dtype=torch.float32, device=dev)
    _, ws = contrastive_raw_forward(Z0, Z1, pairs, neg, 0.0)
    flags = contrastive_results(ws, pairs.shape[0], neg.shape[0], 16)["flags"]
    return neg[(flags & CLOSS_MASKED) == 0]
