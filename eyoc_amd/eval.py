"""Feature-space nearest neighbours with the reference's call surface.

``find_nn_gpu`` / ``pdist`` mirror ``lib/eval.py:18-48`` and ``lib/metrics.py:22-29``; ``find_corr`` and
``random_sample`` mirror ``scripts/test_kitti.py:28-42,54-73`` (twin of ``find_corr`` at
``lib/trainer.py:405-419``).  ``find_correspondences`` is the alias named by the project brief.

The search runs in ``libeyoc_hip.so`` (``eyoc_knn1``): the reference materialises a
``[500, 5000, 32]`` difference tensor per chunk and synchronises after each; here nothing is
materialised and ``nn_max_n`` (a memory knob that never changes the result) is accepted and ignored.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch

from . import _lib

# "GemmL2" is not a reference name: it selects Matcher.match_pair's sqrt(2 - 2 <a,b> + 1e-6) (SC2_PCR.py:296-298)
_DIST = {"SquareL2": 0, "L2": 1, "GemmL2": 2}


def _cuda_f32(t, device=None) -> torch.Tensor:
    """fp32, contiguous, on the GPU (host inputs are uploaded - there is no CPU compute path)."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.EyocError("no GPU visible: the EYOC hot path runs on MI355X only (no CPU fallback)")
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.to(torch.float32).contiguous()


MAX_SEGMENTS = 128


def _segment_chunks(seg_a, seg_b):
    """The library takes at most ``MAX_SEGMENTS`` segments per launch: yield ``(a0, sa, sb, ns)`` per launch, with
    ``sa`` re-based to the chunk's first A row ``a0`` (outputs are per A row) and ``sb`` absolute."""
    nseg = len(seg_a) - 1
    for s0 in range(0, nseg, MAX_SEGMENTS):
        ns = min(MAX_SEGMENTS, nseg - s0)
        a0 = int(seg_a[s0])
        if int(seg_a[s0 + ns]) == a0:
            continue
        sa = (C.c_int32 * (ns + 1))(*[int(v) - a0 for v in seg_a[s0:s0 + ns + 1]])
        sb = (C.c_int32 * (ns + 1))(*[int(v) for v in seg_b[s0:s0 + ns + 1]])
        yield a0, sa, sb, ns


def knn1_segmented(A: torch.Tensor, B: torch.Tensor, seg_a, seg_b, dist_type="SquareL2", return_distance=True):
    """Independent 1-NN problems packed in one launch: rows ``seg_a[s]:seg_a[s+1]`` of ``A`` against rows
    ``seg_b[s]:seg_b[s+1]`` of ``B``.  Returns device tensors ``idx int64 [len(A)]`` (local to the B
    segment) and ``dist f32 [len(A)]``."""
    if dist_type not in _DIST:
        raise NotImplementedError('Not implemented')
    A, B = _cuda_f32(A), _cuda_f32(B, A.device if A.is_cuda else None)
    idx = torch.empty(A.shape[0], dtype=torch.int64, device=A.device)
    # no distances asked for: the library is told so (NULL) - it may then decide most rows by an MFMA score (knn.hip)
    dist = torch.empty(A.shape[0] if return_distance else 0, dtype=torch.float32, device=A.device)
    if A.shape[0] == 0:
        return (idx, dist) if return_distance else idx
    if A.shape[1] != B.shape[1]:
        raise ValueError("feature dimensions differ")
    with torch.cuda.device(A.device):
        for a0, sa, sb, ns in _segment_chunks(seg_a, seg_b):
            _lib.check(_lib.load().eyoc_knn1(_lib.ctx(A.device.index), _lib.ptr(A[a0:]), _lib.ptr(B), A.shape[1], sa, sb, ns,
                                             _DIST[dist_type], _lib.ptr(idx[a0:]), _lib.ptr(dist[a0:]) if return_distance else None,
                                             _lib.stream_ptr()),
                       "eyoc_knn1")
    return (idx, dist) if return_distance else idx


def _mutual_chunks(seg_a, seg_b):
    """``_segment_chunks`` for the mutual search, whose outputs are per A row AND per B row: yield ``(a0, b0, sa, sb, ns)`` per launch
    with both ``sa`` and ``sb`` re-based to the chunk's first rows.  A chunk with an empty side has nothing to search (indices 0, no
    flags - what the outputs are initialised to) and is skipped."""
    nseg = len(seg_a) - 1
    for s0 in range(0, nseg, MAX_SEGMENTS):
        ns = min(MAX_SEGMENTS, nseg - s0)
        a0, b0 = int(seg_a[s0]), int(seg_b[s0])
        if int(seg_a[s0 + ns]) == a0 or int(seg_b[s0 + ns]) == b0:
            continue
        sa = (C.c_int32 * (ns + 1))(*[int(v) - a0 for v in seg_a[s0:s0 + ns + 1]])
        sb = (C.c_int32 * (ns + 1))(*[int(v) - b0 for v in seg_b[s0:s0 + ns + 1]])
        yield a0, b0, sa, sb, ns


def _knn1_mutual_flags(A, B, seg_a, seg_b, dist_type, want_reverse):
    """``eyoc_knn1_mutual`` over every chunk -> ``(A, idx_ab, flags uint8 [len(A)], idx_ba or None)``; ``flags`` as the library writes
    them (bit 0 mutual, bit 1 the row has a neighbour - ``eyoc_mutual_compact``'s fallback reads it)."""
    if dist_type not in _DIST:
        raise NotImplementedError('Not implemented')
    A = _cuda_f32(A)
    B = _cuda_f32(B, A.device)
    if A.shape[1] != B.shape[1]:
        raise ValueError("feature dimensions differ")
    if int(seg_a[-1]) != A.shape[0] or int(seg_b[-1]) != B.shape[0] or len(seg_a) != len(seg_b):
        raise ValueError("seg_a / seg_b must cover A / B with the same number of segments")
    idx_ab = torch.zeros(A.shape[0], dtype=torch.int64, device=A.device)
    flags = torch.zeros(A.shape[0], dtype=torch.uint8, device=A.device)
    idx_ba = torch.zeros(B.shape[0], dtype=torch.int64, device=A.device) if want_reverse else None
    with torch.cuda.device(A.device):
        for a0, b0, sa, sb, ns in _mutual_chunks(seg_a, seg_b):
            _lib.check(_lib.load().eyoc_knn1_mutual(_lib.ctx(A.device.index), _lib.ptr(A[a0:]), _lib.ptr(B[b0:]), A.shape[1], sa, sb, ns,
                                                    _DIST[dist_type], _lib.ptr(idx_ab[a0:]), _lib.ptr(idx_ba[b0:]) if want_reverse else None,
                                                    _lib.ptr(flags[a0:]), _lib.stream_ptr()), "eyoc_knn1_mutual")
    return A, idx_ab, flags, idx_ba


def knn1_mutual_segmented(A, B, seg_a, seg_b, dist_type="SquareL2", return_reverse=False):
    """``knn1_segmented`` with the reciprocity check, per segment, on the device: ``idx_ab int64 [len(A)]`` - exactly
    ``knn1_segmented(A, B)``'s indices -, ``mutual bool [len(A)]`` - row ``i`` has a neighbour ``j = idx_ab[i]``, ``j`` has one among
    the segment's A rows, and that is ``i`` (ties to the lowest index both ways; a row without a neighbour - empty B segment, NaN
    features - reads index 0 and is never mutual) - and with ``return_reverse`` ``idx_ba int64 [len(B)]``, exactly
    ``knn1_segmented(B, A, seg_b, seg_a)``'s.  One library call per 128 segments (``eyoc_knn1_mutual``)."""
    _, idx_ab, flags, idx_ba = _knn1_mutual_flags(A, B, seg_a, seg_b, dist_type, return_reverse)
    mutual = (flags & 1).to(torch.bool)
    return (idx_ab, mutual, idx_ba) if return_reverse else (idx_ab, mutual)


def mutual_compact_device(idx_ab, flags, seg_a, min_keep=0):
    """``eyoc_mutual_compact`` on ``_knn1_mutual_flags``' outputs, nothing read back: ``(rows int64, corr int64, seg_out int32
    [nseg + 1])`` on the device; only the first ``seg_out[-1]`` entries of ``rows`` / ``corr`` (both ``[len(A)]``) mean anything."""
    n, nseg, dev = idx_ab.shape[0], len(seg_a) - 1, idx_ab.device
    rows = torch.empty(n, dtype=torch.int64, device=dev)
    corr = torch.empty(n, dtype=torch.int64, device=dev)
    outs = []
    with torch.cuda.device(dev):
        for s0 in range(0, nseg, MAX_SEGMENTS):
            ns = min(MAX_SEGMENTS, nseg - s0)
            a0 = int(seg_a[s0])
            sa = (C.c_int32 * (ns + 1))(*[int(v) - a0 for v in seg_a[s0:s0 + ns + 1]])
            so = torch.empty(ns + 1, dtype=torch.int32, device=dev)
            _lib.check(_lib.load().eyoc_mutual_compact(_lib.ctx(dev.index), _lib.ptr(idx_ab[a0:]), _lib.ptr(flags[a0:]), sa, ns, int(min_keep),
                                                       _lib.ptr(rows[a0:]), _lib.ptr(corr[a0:]), _lib.ptr(so), _lib.stream_ptr()),
                       "eyoc_mutual_compact")
            outs.append((a0, so))
    if len(outs) == 1:
        return rows, corr, outs[0][1]
    # several launches: every chunk's kept rows sit at the chunk's first A row; move them back to back (device-side, no counts on the host)
    counts = torch.cat([so[1:] - so[:-1] for _, so in outs])
    seg_out = torch.cat((counts.new_zeros(1), torch.cumsum(counts, 0).to(torch.int32)))
    k = torch.arange(n, device=dev)
    src = torch.zeros(n, dtype=torch.int64, device=dev)
    for (a0, so), s0 in zip(outs, range(0, nseg, MAX_SEGMENTS)):
        # output position p in [seg_out[s0], seg_out[s0] + so[-1]) reads the chunk's entry a0 + p - seg_out[s0]
        lo = seg_out[s0].to(torch.int64)
        inside = (k >= lo) & (k < lo + so[-1].to(torch.int64))
        src = torch.where(inside, k - lo + a0, src)
    return rows[src], corr[src], seg_out


_PINNED_SEG: dict = {}


def read_back_segments(seg_out_dev, buf=None):
    """``seg_out`` on the host (a numpy copy): an asynchronous copy into pinned memory and an event wait - this stream only, no device
    synchronisation.  ``buf``: the caller's own pinned ``int32`` staging (the pipeline keeps one per slot); without it a buffer cached
    per (thread, device, length) - the copy and the read of it happen inside this call, so no two callers ever share one in flight."""
    n = seg_out_dev.numel()
    if buf is None:
        key = (threading.get_ident(), seg_out_dev.device.index, n)
        buf = _PINNED_SEG.get(key)
        if buf is None:
            buf = _PINNED_SEG[key] = torch.empty(n, dtype=torch.int32, pin_memory=True)
    buf = buf[:n]
    buf.copy_(seg_out_dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    ev.synchronize()
    return buf.numpy().copy()


def mutual_correspondences(A, B, seg_a, seg_b, dist_type="SquareL2", min_keep=0):
    """The mutual nearest neighbours of every segment, compacted in order: ``rows int64 [m]`` (row inside its A segment), ``corr int64
    [m]`` (its neighbour, inside the B segment) on the device and ``seg_out`` (numpy ``int32 [nseg + 1]``): segment ``s`` owns
    ``[seg_out[s], seg_out[s + 1])``.  A segment with fewer than ``min_keep`` mutual rows keeps all of its rows that have a neighbour
    (Open3D's fallback with ``min_keep = ransac_n``); 0: no fallback.  ``seg_out`` is the one read-back, and the only wait."""
    A, idx_ab, flags, _ = _knn1_mutual_flags(A, B, seg_a, seg_b, dist_type, False)
    with torch.cuda.device(A.device):
        rows, corr, seg_dev = mutual_compact_device(idx_ab, flags, seg_a, min_keep)
        seg_out = read_back_segments(seg_dev)
    m = int(seg_out[-1])
    return rows[:m], corr[:m], seg_out


def gather_rows(F: torch.Tensor, sel: torch.Tensor, G: torch.Tensor | None = None, beta: float = 0.0) -> torch.Tensor:
    """``F[sel]`` in one launch (``eyoc_gather_rows``); with ``G`` ``[len(sel), C]`` the gathered rows are blended
    and re-normalised, ``(F[sel] + beta * G) / |.|`` - the descriptor mode of the synthetic benchmark."""
    F = _cuda_f32(F)
    if sel is not None:                     # (None: every row of ``F`` in place - the blend alone)
        sel = sel.to(F.device, torch.int64).contiguous()
    n = F.shape[0] if sel is None else sel.shape[0]
    c = F.shape[1]
    out = torch.empty((n, c), dtype=torch.float32, device=F.device)
    if G is not None:
        G = _cuda_f32(G, F.device)
        if tuple(G.shape) != (n, c):
            raise ValueError("G must be [len(sel), C]")
    with torch.cuda.device(F.device):
        _lib.check(_lib.load().eyoc_gather_rows(_lib.ctx(F.device.index), _lib.ptr(F), F.stride(0), c, _lib.ptr(sel),
                                                n, _lib.ptr(G), C.c_float(beta), _lib.ptr(out),
                                                _lib.stream_ptr()), "eyoc_gather_rows")
    return out


def dotmax_segmented(A, B, seg_a, seg_b):
    """``(A @ B.T).max(dim=1)`` per segment without the matrix: ``(weight f32 [len(A)], idx int64 [len(A)])`` on the
    device (util/transform_estimation.py:131-133)."""
    A, B = _cuda_f32(A), _cuda_f32(B, A.device if A.is_cuda else None)
    if A.shape[1] != B.shape[1]:
        raise ValueError("feature dimensions differ")
    idx = torch.zeros(A.shape[0], dtype=torch.int64, device=A.device)
    w = torch.full((A.shape[0],), float("nan"), dtype=torch.float32, device=A.device)
    if A.shape[0]:
        with torch.cuda.device(A.device):
            for a0, sa, sb, ns in _segment_chunks(seg_a, seg_b):
                _lib.check(_lib.load().eyoc_dotmax(_lib.ctx(A.device.index), _lib.ptr(A[a0:]), _lib.ptr(B), A.shape[1], sa, sb,
                                                   ns, _lib.ptr(idx[a0:]), _lib.ptr(w[a0:]), _lib.stream_ptr()), "eyoc_dotmax")
    return w, idx


def find_nn_gpu(F0, F1, nn_max_n=-1, return_distance=False, dist_type='SquareL2'):
    """lib/eval.py:18-48.  Returns CPU tensors like the reference: ``inds int64 [N0]`` and, on request,
    ``dists f32 [N0,1]``."""
    F0 = _cuda_f32(F0)
    F1 = _cuda_f32(F1, F0.device)
    if F0.shape[1] != F1.shape[1]:
        raise ValueError("feature dimensions differ")
    if dist_type not in ("SquareL2", "L2"):          # lib/metrics.py:29
        raise NotImplementedError('Not implemented')
    idx, dist = knn1_segmented(F0, F1, [0, F0.shape[0]], [0, F1.shape[0]], dist_type)
    inds = idx.cpu()
    if return_distance:
        return inds, dist.unsqueeze(1).cpu()
    return inds


def pdist(A, B, dist_type='L2'):
    """lib/metrics.py:22-29 - dense ``[n,m]`` distance matrix on the device of ``A``."""
    if dist_type not in ("SquareL2", "L2"):
        raise NotImplementedError('Not implemented')
    A = _cuda_f32(A)
    B = _cuda_f32(B, A.device)
    out = torch.empty((A.shape[0], B.shape[0]), dtype=torch.float32, device=A.device)
    with torch.cuda.device(A.device):
        _lib.check(_lib.load().eyoc_pdist(_lib.ctx(A.device.index), _lib.ptr(A), A.shape[0], _lib.ptr(B), B.shape[0],
                                          A.shape[1], _DIST[dist_type], _lib.ptr(out), _lib.stream_ptr()), "eyoc_pdist")
    return out


def find_corr(xyz0, xyz1, F0, F1, subsample_size=-1, rng=None):
    """scripts/test_kitti.py:28-42.  ``rng`` (a ``numpy.random.Generator`` or ``RandomState``) replaces the
    reference's use of the global ``np.random`` so callers can make the draw reproducible."""
    rng = np.random if rng is None else rng
    subsample = len(F0) > subsample_size
    if subsample_size > 0 and subsample:
        N0 = min(len(F0), subsample_size)
        N1 = min(len(F1), subsample_size)
        inds0 = rng.choice(len(F0), N0, replace=False)
        inds1 = rng.choice(len(F1), N1, replace=False)
        F0, F1 = F0[inds0], F1[inds1]
    nn_inds = find_nn_gpu(F0, F1, nn_max_n=500)
    if subsample_size > 0 and subsample:
        return xyz0[inds0], xyz1[inds1[nn_inds]]
    return xyz0, xyz1[nn_inds]


find_correspondences = find_corr


def random_sample(pcd, feats, N, rng=None):
    """scripts/test_kitti.py:54-73 - exactly ``N`` points (permutation if n > N, with replacement if n < N)."""
    rng = np.random if rng is None else rng
    n1 = pcd.size(0) if isinstance(pcd, torch.Tensor) else pcd.shape[0]
    if n1 == N:
        return pcd, feats
    choice = rng.permutation(n1)[:N] if n1 > N else rng.choice(n1, N)
    return pcd[choice], feats[choice]
