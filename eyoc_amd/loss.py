"""The hardest-contrastive loss of EYOC's trainer (lib/trainer.py:935-991) and its gradient in one device pass.

``hardest_contrastive_loss`` is ``autograd.contrastive_hardest_negative_loss`` with the same draws and the same value, as ONE autograd
node on ``eyoc_hcloss_forward`` / ``eyoc_hcloss_backward`` (csrc/loss.hip): the positives may be a device tensor and then never leave
the device (the label stages produce them there), the three host draws go up in one asynchronous copy, nothing is read back, the
number of launches is fixed (5 + 4) and the gradient rows are summed in a fixed order without floating-point atomics - their bytes do
not change from run to run.  The existing function stays; this route is opt-in."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .autograd import _draw_loss_samples

BAD_INDEX, MASKED, VALID = 1, 1, 2        # record status bit; per-direction flag bits (include/eyoc_hip.h)
_RECORD_FLOATS = C.sizeof(_lib.HclossRecord) // 4


def layout(n_pairs, n_used, s0, s1, c):
    out = _lib.HclossLayout()
    _lib.check(_lib.load().eyoc_hcloss_workspace_layout(n_pairs, n_used, s0, s1, c, C.byref(out)), "eyoc_hcloss_workspace_layout")
    return out


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
    lib = _lib.load()
    n_used = pairs.shape[0] if used is None else used.shape[0]
    with _lib.on_device(F0.device):
        ws = _lib.workspace(lib.eyoc_hcloss_workspace_bytes(pairs.shape[0], n_used, sel0.shape[0], sel1.shape[0], F0.shape[1]), F0.device)
        rec = torch.empty(_RECORD_FLOATS, dtype=torch.float32, device=F0.device)
        _lib.check(lib.eyoc_hcloss_forward(*_args(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh), _lib.ptr(rec), _lib.ptr(ws),
                                           ws.numel(), _lib.stream_ptr()), "eyoc_hcloss_forward")
    return rec, ws


def backward_raw(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh, g_pos, g_neg, ws):
    """``eyoc_hcloss_backward`` -> ``(dF0, dF1)``; ``g_pos`` / ``g_neg`` float32 device scalars, ``ws`` from ``forward_raw`` on the same arguments."""
    lib = _lib.load()
    dF0, dF1 = torch.empty_like(F0), torch.empty_like(F1)
    with _lib.on_device(F0.device):
        _lib.check(lib.eyoc_hcloss_backward(*_args(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh), _lib.ptr(g_pos), _lib.ptr(g_neg),
                                            _lib.ptr(dF0), _lib.ptr(dF1), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                   "eyoc_hcloss_backward")
    return dF0, dF1


def read_record(rec) -> _lib.HclossRecord:
    """The record on the host (tests, logging): this READS BACK, the loss itself never does."""
    return _lib.HclossRecord.from_buffer_copy(rec.detach().cpu().numpy().tobytes())


def results(ws, n_pairs, n_used, s0, s1, c):
    """The per-positive results the forward left in its workspace, as device views: ``tstar`` int32 [2, n_used] (-1: none), ``dist``
    float32 [2, n_used], ``pos_d2`` float32 [n_used], ``flags`` int32 [2, n_used] (``MASKED`` / ``VALID``); row 0 is direction 01."""
    lay = layout(n_pairs, n_used, s0, s1, c)

    def view(off, count, dtype):
        return ws[off:off + 4 * count].view(dtype)
    return {"tstar": view(lay.off_tstar, 2 * n_used, torch.int32).view(2, n_used),
            "dist": view(lay.off_dist, 2 * n_used, torch.float32).view(2, n_used),
            "pos_d2": view(lay.off_pos_d2, n_used, torch.float32),
            "flags": view(lay.off_flags, 2 * n_used, torch.int32).view(2, n_used)}


class _HardestContrastive(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh):
        rec, ws = forward_raw(F0, F1, pairs, used, sel0, sel1, pos_thresh, neg_thresh)
        ctx.save_for_backward(F0, F1)
        ctx.idx, ctx.thresh, ctx.ws = (pairs, used, sel0, sel1), (pos_thresh, neg_thresh), ws
        return rec[_RECORD_FLOATS - 2], rec[_RECORD_FLOATS - 1]

    @staticmethod
    def backward(ctx, g_pos, g_neg):
        F0, F1 = ctx.saved_tensors

        def scalar(g):                                  # a missing gradient is zero
            if g is None:
                return torch.zeros((), dtype=torch.float32, device=F0.device)
            return g.to(torch.float32).contiguous()
        dF0, dF1 = backward_raw(F0, F1, *ctx.idx, *ctx.thresh, scalar(g_pos), scalar(g_neg), ctx.ws)
        return dF0, dF1, None, None, None, None, None, None


def hardest_contrastive_loss(F0, F1, positive_pairs, num_pos=5192, num_hn_samples=2048, pos_thresh=0.1, neg_thresh=1.4, rng=None):
    """lib/trainer.py:935-991 -> ``(pos_loss, neg_loss)``, 0-dim tensors with grad, the values of
    ``autograd.contrastive_hardest_negative_loss`` for the same ``rng`` (the three draws are the same function, in the reference's order).

    ``positive_pairs``: a DEVICE int64 ``[n, 2]`` tensor stays on the device; a host tensor or ndarray costs one upload.  No double
    backward; ``c`` in {16, 32, 64}."""
    dev = F0.device
    if isinstance(positive_pairs, torch.Tensor):
        pairs = positive_pairs
    else:
        pairs = torch.from_numpy(np.ascontiguousarray(np.asarray(positive_pairs), dtype=np.int64))
    pairs = pairs.reshape(-1, 2).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
    n0, n1, n_pairs = F0.shape[0], F1.shape[0], pairs.shape[0]
    cand0, cand1, keep = _draw_loss_samples(np.random if rng is None else rng, n0, n1, n_pairs, num_hn_samples, num_pos)
    s0, s1, n_keep = len(cand0), len(cand1), 0 if keep is None else len(keep)
    # the draws: one pinned staging buffer, one asynchronous copy
    stage = torch.empty(s0 + s1 + n_keep, dtype=torch.int64, pin_memory=True)
    host = stage.numpy()
    host[:s0], host[s0:s0 + s1] = cand0, cand1
    if keep is not None:
        host[s0 + s1:] = keep
    draws = stage.to(dev, non_blocking=True)
    used = None if keep is None else draws[s0 + s1:]
    return _HardestContrastive.apply(F0.contiguous(), F1.contiguous(), pairs, used, draws[:s0], draws[s0:s0 + s1], float(pos_thresh),
                                     float(neg_thresh))
