"""Label generation of EYOC's training loop on the GPU: the reference's
``match_and_filter_corr`` (lib/trainer.py:1025-1151) and the non-mutual branch of ``corr_through_registration``
(lib/trainer.py:1195-1218), with the same argument meaning.  Nearest neighbours, ratio weights, top-k and the
filters run in ``libeyoc_hip.so`` (``eyoc_knn2``, ``eyoc_lowe_topk``, ``eyoc_pair_filter``).

The ``*_batched`` functions, ``corr_through_registration`` and ``label_step`` do the same for a whole batch without a per-pair host
loop (``eyoc_lowe_topk_segmented``, ``eyoc_pair_filter_batched``, ``eyoc_posed_nn_grid``): pair for pair the bytes of the functions
above, with a fixed number of host synchronisations whatever the batch size."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .eval import _cuda_f32, _segment_chunks


def knn2_segmented(A, B, seg_a, seg_b):
    """``knn_points(A, B, K=2)`` for independent segments: nearest index (int64, local to the B segment) and the
    two smallest squared distances of every row of ``A``; feature width 4 / 16 / 32 / 64 / 128."""
    A = _cuda_f32(A)
    B = _cuda_f32(B, A.device)
    if A.shape[1] != B.shape[1]:
        raise ValueError("feature dimensions differ")
    idx = torch.zeros(A.shape[0], dtype=torch.int64, device=A.device)
    d1 = torch.full((A.shape[0],), float("inf"), dtype=torch.float32, device=A.device)
    d2 = torch.full((A.shape[0],), float("inf"), dtype=torch.float32, device=A.device)
    if A.shape[0] == 0:
        return idx, d1, d2
    with torch.cuda.device(A.device):
        for a0, sa, sb, ns in _segment_chunks(seg_a, seg_b):      # at most 128 segments per launch
            _lib.check(_lib.load().eyoc_knn2(_lib.ctx(A.device.index), _lib.ptr(A[a0:]), _lib.ptr(B), A.shape[1], sa, sb, ns,
                                             _lib.ptr(idx[a0:]), _lib.ptr(d1[a0:]), _lib.ptr(d2[a0:]), _lib.stream_ptr()),
                       "eyoc_knn2")
    return idx, d1, d2


def lowe_topk(d1, d2, k):
    """calculate_ratio_test + get_topk_matches (lib/trainer.py:993-1016) on the two nearest squared distances:
    ``(idx_source int64 [k], weight f32 [k])``, largest weight first."""
    d1, d2 = _cuda_f32(d1), _cuda_f32(d2)
    k = min(int(k), d1.shape[0])
    idx = torch.empty(k, dtype=torch.int64, device=d1.device)
    w = torch.empty(k, dtype=torch.float32, device=d1.device)
    if k:
        with torch.cuda.device(d1.device):
            _lib.check(_lib.load().eyoc_lowe_topk(_lib.ctx(d1.device.index), _lib.ptr(d1), _lib.ptr(d2), d1.shape[0], k,
                                                  _lib.ptr(idx), _lib.ptr(w), _lib.stream_ptr()), "eyoc_lowe_topk")
    return idx, w


def _pair_filter(mode, P0, P1, i0, i1, T, radius):
    P0 = _cuda_f32(P0)
    P1 = _cuda_f32(P1, P0.device)
    i0 = i0.to(P0.device, torch.int64).contiguous()
    i1 = i1.to(P0.device, torch.int64).contiguous()
    m = i0.shape[0]
    out = torch.empty((m, 2), dtype=torch.int64, device=P0.device)
    n_out = torch.zeros(1, dtype=torch.int32, device=P0.device)
    Td = None if T is None else _cuda_f32(torch.as_tensor(np.asarray(T, np.float32)).reshape(16), P0.device)
    with torch.cuda.device(P0.device):
        _lib.check(_lib.load().eyoc_pair_filter(_lib.ctx(P0.device.index), mode, _lib.ptr(P0), _lib.ptr(P1), _lib.ptr(i0),
                                                _lib.ptr(i1), m, _lib.ptr(Td), C.c_float(radius), _lib.ptr(out),
                                                _lib.ptr(n_out), _lib.stream_ptr()), "eyoc_pair_filter")
    return out[:int(n_out.item())]


def spherical_filter(C0, C1, idx0, idx1, radius):
    """lib/trainer.py:1107-1110: the pairs whose two endpoints are both farther than ``radius`` from their sensor."""
    return _pair_filter(0, C0, C1, idx0, idx1, None, float(radius))


FRAME_TO_YGRID = {0: 1, 1: 1.5, 2: 2, 3: 2.5, 4: 2.5, 5: 2.5}      # lib/trainer.py:1136


def load_dist_sim_map(path):
    """``config/dist_sim_plot/<dataset>_distSimPlot.npz`` as the reference reads it (lib/trainer.py:1128-1132):
    ``{frame_index 0..5: float64 [xlim, ylim]}``."""
    maps = np.load(path, allow_pickle=True)["res"].tolist()
    return {i: np.asarray(maps[i], np.float64) for i in range(6)}


def similarity_filter(C0, C1, idx0, idx1, dist_sim_map, frame_distance, similarity_thresh=0.4):
    """lib/trainer.py:1118-1149 for one pair: keep the index pairs whose (min centre distance, centre-distance gap)
    cell of the distance-similarity table exceeds ``similarity_thresh``.  ``dist_sim_map``: ``{0..5: [xlim, ylim]}``
    (``load_dist_sim_map``); ``frame_distance``: the pair's frame gap (the table slice is ``clamp(gap // 5, 0, 5)``)."""
    frame_index = min(max(0, int(frame_distance) // 5), 5)
    table = np.ascontiguousarray(np.asarray(dist_sim_map[frame_index], np.float64))
    xlim, ylim = table.shape
    P0 = _cuda_f32(C0)
    P1 = _cuda_f32(C1, P0.device)
    i0 = idx0.to(P0.device, torch.int64).contiguous()
    i1 = idx1.to(P0.device, torch.int64).contiguous()
    m = i0.shape[0]
    out = torch.empty((m, 2), dtype=torch.int64, device=P0.device)
    n_out = torch.zeros(1, dtype=torch.int32, device=P0.device)
    td = torch.from_numpy(table).to(P0.device)
    with torch.cuda.device(P0.device):
        _lib.check(_lib.load().eyoc_pair_filter_similarity(
            _lib.ctx(P0.device.index), _lib.ptr(P0), _lib.ptr(P1), _lib.ptr(i0), _lib.ptr(i1), m, _lib.ptr(td), xlim, ylim,
            C.c_float(5.0), C.c_float(FRAME_TO_YGRID[frame_index]), C.c_double(similarity_thresh), _lib.ptr(out), _lib.ptr(n_out),
            _lib.stream_ptr()), "eyoc_pair_filter_similarity")
    return out[:int(n_out.item())]


def match_and_filter_corr(C_batch_0, F_batch_0, C_batch_1, F_batch_1, radius=20, feature_filter="Lowe",
                          spatial_filter="Spherical", frame_distance=None, num_corres=5000, dist_sim_map=None,
                          similarity_thresh=0.4):
    """lib/trainer.py:1025-1151.  Lists of per-cloud ``[n_i,3]`` coordinates and ``[n_i,d]`` features ->
    ``(matches int64 [N,2] on the CPU, with the collate biases; list of per-pair [M_i,2] device tensors)``.
    ``spatial_filter="Similarity"`` needs ``frame_distance`` (one gap per pair) and ``dist_sim_map`` (the reference
    reads it from ``config/dist_sim_plot/<pretraining_dataset>_distSimPlot.npz``: ``load_dist_sim_map``) with
    ``similarity_thresh`` = ``config.similarity_thresh``."""
    if feature_filter not in ("None", "Lowe"):
        raise AssertionError(feature_filter)
    if spatial_filter not in ("Spherical", "None", "Similarity"):
        raise AssertionError(spatial_filter)
    if spatial_filter == "Similarity" and (dist_sim_map is None or frame_distance is None):
        raise ValueError('spatial_filter="Similarity" needs dist_sim_map and frame_distance')
    F0s = [_cuda_f32(f) for f in F_batch_0]
    dev = F0s[0].device
    F1s = [_cuda_f32(f, dev) for f in F_batch_1]
    n0 = [f.shape[0] for f in F0s]
    n1 = [f.shape[0] for f in F1s]
    seg0 = np.concatenate([[0], np.cumsum(n0)])
    seg1 = np.concatenate([[0], np.cumsum(n1)])
    A, B = torch.cat(F0s), torch.cat(F1s)
    i12, d1a, d2a = knn2_segmented(A, B, seg0, seg1)          # both directions, all pairs of the batch in one launch each
    i21, d1b, d2b = knn2_segmented(B, A, seg1, seg0)
    k1, k2 = min(num_corres, min(n0)), min(num_corres, min(n1))
    idx1, idx2 = [], []
    for p in range(len(F0s)):
        a0, a1, b0, b1 = int(seg0[p]), int(seg0[p + 1]), int(seg1[p]), int(seg1[p + 1])
        if feature_filter == "Lowe":
            s12, _ = lowe_topk(d1a[a0:a1], d2a[a0:a1], k1)
            s21, _ = lowe_topk(d1b[b0:b1], d2b[b0:b1], k2)
        else:                                                  # weights = the nearest distance itself (:1072-1073)
            s12 = torch.argsort(-d1a[a0:a1].double(), stable=True)[:k1]
            s21 = torch.argsort(-d1b[b0:b1].double(), stable=True)[:k2]
        t12, t21 = i12[a0:a1][s12], i21[b0:b1][s21]
        idx1.append(torch.cat([s12, t21]))
        idx2.append(torch.cat([t12, s21]))
    matches = torch.cat([torch.stack([a + int(seg0[p]), b + int(seg1[p])], 1) for p, (a, b) in enumerate(zip(idx1, idx2))])
    uncollated = []
    for p in range(len(F0s)):
        if spatial_filter == "None":
            uncollated.append(torch.stack([idx1[p], idx2[p]], 1))
        elif spatial_filter == "Similarity":
            uncollated.append(similarity_filter(C_batch_0[p], C_batch_1[p], idx1[p], idx2[p], dist_sim_map, frame_distance[p],
                                                similarity_thresh))
        else:
            uncollated.append(spherical_filter(C_batch_0[p], C_batch_1[p], idx1[p], idx2[p], radius))
    return matches.cpu(), uncollated


def apply_pose(T, P):
    """``R p + t`` with every fp32 operation rounded separately, left to right (the arithmetic ``eyoc_pair_filter``
    uses for its residual), so the nearest neighbour below and the filter see the same posed points."""
    T = torch.as_tensor(np.asarray(T, np.float32)).to(P.device)
    cols = [((T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]) + T[r, 3] for r in range(3)]
    return torch.stack(cols, 1)


def correspondences_under_pose(pcd0, pcd1, T, n_sample=5000, max_dist=2.0, pos_sel=None, generator=None):
    """lib/trainer.py:1195-1218 for one pair: nearest ``pcd1`` point of every posed ``pcd0`` point, a random subset
    of at most ``n_sample`` of them (``torch.randperm`` like the reference; pass ``pos_sel`` to fix the draw), kept
    where the residual under ``T`` is below ``max_dist``.  Returns ``int64 [M,2]`` on the device."""
    P0 = _cuda_f32(pcd0)
    P1 = _cuda_f32(pcd1, P0.device)
    q = apply_pose(T, P0)
    pad = lambda P: torch.cat([P, torch.zeros((P.shape[0], 1), device=P.device)], 1).contiguous()
    idx, _, _ = knn2_segmented(pad(q), pad(P1), [0, P0.shape[0]], [0, P1.shape[0]])
    if pos_sel is None:
        pos_sel = torch.randperm(P0.shape[0], generator=generator)[:min(P0.shape[0], n_sample)]
    sel = torch.as_tensor(pos_sel).to(P0.device, torch.int64)
    return _pair_filter(1, P0, P1, sel, idx[sel], T, float(max_dist))


# ----------------------------------------------------------------------------------------------------------------------
# The whole batch in one device pass
# ----------------------------------------------------------------------------------------------------------------------
def _seg32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def _offsets(sizes):
    return [0] + [int(v) for v in np.cumsum([int(n) for n in sizes])]


def _upload(t, device):
    """Host tensor -> device through pinned memory on the current stream: the copy is enqueued, the host does not wait for the stream."""
    return t.pin_memory().to(device, non_blocking=True)


def lowe_topk_segmented(d1, d2, seg, k, mode=0, return_weights=False):
    """``lowe_topk`` on every segment ``seg[s]:seg[s+1]`` of ``d1 / d2`` with one ``k`` (at most the shortest segment): ``idx int64
    [nseg, k]`` local to the segment and, with ``return_weights``, ``w f32 [nseg, k]``.  ``mode=1``: weight = ``d1`` (the
    ``feature_filter="None"`` order, a stable descending fp64 argsort).  Three launches and one sort for the batch; row ``s`` is byte
    for byte ``lowe_topk`` on segment ``s`` alone."""
    d1 = _cuda_f32(d1)
    d2 = None if d2 is None else _cuda_f32(d2, d1.device)
    nseg, k = len(seg) - 1, int(k)
    idx = torch.empty((nseg, k), dtype=torch.int64, device=d1.device)
    w = torch.empty((nseg, k), dtype=torch.float32, device=d1.device) if return_weights else None
    with torch.cuda.device(d1.device):
        _lib.check(_lib.load().eyoc_lowe_topk_segmented(_lib.ctx(d1.device.index), _lib.ptr(d1), _lib.ptr(d2), _seg32(seg), nseg, k, int(mode),
                                                        _lib.ptr(idx), _lib.ptr(w), _lib.stream_ptr()), "eyoc_lowe_topk_segmented")
    return (idx, w) if return_weights else idx


def _sim_slices(dist_sim_map, frame_distance):
    """The six table slices back to back (host float64) and every pair's descriptor of the one it reads."""
    tables = [np.ascontiguousarray(np.asarray(dist_sim_map[i], np.float64)) for i in range(6)]
    off = _offsets([t.size for t in tables])
    slices = (_lib.SimSlice * len(frame_distance))()
    for p, gap in enumerate(frame_distance):
        fi = min(max(0, int(gap) // 5), 5)
        slices[p] = _lib.SimSlice(off[fi], tables[fi].shape[0], tables[fi].shape[1], FRAME_TO_YGRID[fi], 0)
    return np.concatenate([t.reshape(-1) for t in tables]), slices


def pair_filter_batched(mode, P0, P1, idx0, idx1, seg_p0, seg_p1, seg_m, T=None, radius=0.0, tables=None, slices=None, thresh=0.4,
                        counts=None):
    """Modes 0 / 1 / 2 of the pair filter for all pairs in one launch per 64 pairs (``eyoc_pair_filter_batched``): packed clouds
    ``P0 / P1`` and packed LOCAL index lists ``idx0 / idx1`` with their host offsets; mode 1 reads ``T f32 [B,4,4]`` on the device,
    mode 2 takes ``tables`` (device float64) and ``slices`` of ``_sim_slices``.  Returns ``(pairs int64 [M,2], counts int32 [B])``
    on the device: the survivors of pair ``b`` are rows ``seg_m[b] : seg_m[b] + counts[b]``.  Nothing is read back here."""
    dev = P0.device
    B = len(seg_m) - 1
    out = torch.empty((int(seg_m[-1]), 2), dtype=torch.int64, device=dev)
    if counts is None:
        counts = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().eyoc_pair_filter_batched(
            _lib.ctx(dev.index), int(mode), _lib.ptr(P0), _lib.ptr(P1), _lib.ptr(idx0), _lib.ptr(idx1), _seg32(seg_p0), _seg32(seg_p1),
            _seg32(seg_m), B, _lib.ptr(T), C.c_float(radius), _lib.ptr(tables), slices, C.c_float(5.0), C.c_double(thresh), _lib.ptr(out),
            _lib.ptr(counts), _lib.stream_ptr()), "eyoc_pair_filter_batched")
    return out, counts


def posed_nn_grid(P0, P1, seg0, seg1, T, max_dist, sel=None, seg_sel=None, return_d2=False, status=None):
    """``eyoc_posed_nn_grid``: for every (selected) row of every pair the row of ``knn2_segmented(pad(apply_pose(T, P0)), pad(P1))``
    local to the pair if its residual is below ``max_dist``, -1 otherwise.  Packed fp32 clouds with host offsets, ``T f32 [B,4,4]`` on
    the device, ``sel int64`` packed local query rows with host offsets ``seg_sel`` (``None``: all rows).  Returns ``(idx int64, d2 f32
    or None, status int32 [B])`` on the device."""
    dev = P0.device
    B = len(seg0) - 1
    nq = int(seg_sel[-1]) if sel is not None else int(seg0[-1])
    idx = torch.empty(nq, dtype=torch.int64, device=dev)
    d2 = torch.empty(nq, dtype=torch.float32, device=dev) if return_d2 else None
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.eyoc_posed_nn_grid_workspace_bytes(B, nq, int(seg1[-1])), dev)
        _lib.check(lib.eyoc_posed_nn_grid(_lib.ctx(dev.index), _lib.ptr(P0), _lib.ptr(P1), _seg32(seg0), _seg32(seg1), B, _lib.ptr(T),
                                          C.c_float(max_dist), _lib.ptr(sel), None if sel is None else _seg32(seg_sel), _lib.ptr(idx),
                                          _lib.ptr(d2), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "eyoc_posed_nn_grid")
    return idx, d2, status


def _pack_clouds(clouds, device=None):
    cs = [_cuda_f32(c, device) for c in clouds]
    return (cs[0] if len(cs) == 1 else torch.cat(cs)), _offsets([c.shape[0] for c in cs])


def match_and_filter_corr_batched(C_batch_0, F_batch_0, C_batch_1, F_batch_1, radius=20, feature_filter="Lowe",
                                  spatial_filter="Spherical", frame_distance=None, num_corres=5000, dist_sim_map=None,
                                  similarity_thresh=0.4):
    """``match_and_filter_corr`` without the per-pair loop: two ``knn2_segmented`` calls, two segmented top-k calls, one batched filter,
    one read-back.  Same arguments; returns ``(matches int64 [N,2] with the collate biases, list of per-pair [M_i,2])`` as DEVICE
    tensors with the values of ``match_and_filter_corr``; the per-pair tensors are views of one buffer."""
    if feature_filter not in ("None", "Lowe"):
        raise AssertionError(feature_filter)
    if spatial_filter not in ("Spherical", "None", "Similarity"):
        raise AssertionError(spatial_filter)
    if spatial_filter == "Similarity" and (dist_sim_map is None or frame_distance is None):
        raise ValueError('spatial_filter="Similarity" needs dist_sim_map and frame_distance')
    F0s = [_cuda_f32(f) for f in F_batch_0]
    dev = F0s[0].device
    F1s = [_cuda_f32(f, dev) for f in F_batch_1]
    B = len(F0s)
    n0, n1 = [f.shape[0] for f in F0s], [f.shape[0] for f in F1s]
    seg0, seg1 = _offsets(n0), _offsets(n1)
    A, Bt = torch.cat(F0s), torch.cat(F1s)
    i12, d1a, d2a = knn2_segmented(A, Bt, seg0, seg1)
    i21, d1b, d2b = knn2_segmented(Bt, A, seg1, seg0)
    k1, k2 = min(num_corres, min(n0)), min(num_corres, min(n1))
    mode = 0 if feature_filter == "Lowe" else 1
    s12 = lowe_topk_segmented(d1a, d2a, seg0, k1, mode)                     # [B, k1], local
    s21 = lowe_topk_segmented(d1b, d2b, seg1, k2, mode)
    bias = _upload(torch.tensor([seg0[:B], seg1[:B]], dtype=torch.int64), dev)     # one small upload: the collate biases
    b0, b1 = bias[0].unsqueeze(1), bias[1].unsqueeze(1)
    t12, t21 = i12[s12 + b0], i21[s21 + b1]
    idx0, idx1 = torch.cat([s12, t21], 1), torch.cat([t12, s21], 1)          # [B, k1 + k2]: lib/trainer.py:1086-1091
    m = k1 + k2
    matches = torch.stack([idx0 + b0, idx1 + b1], 2).reshape(B * m, 2)
    if spatial_filter == "None":
        local = torch.stack([idx0, idx1], 2)
        return matches, [local[p] for p in range(B)]
    P0, p0 = _pack_clouds(C_batch_0, dev)
    P1, p1 = _pack_clouds(C_batch_1, dev)
    if p0 != seg0 or p1 != seg1:
        raise ValueError("coordinates and features of a cloud differ in length")
    seg_m = [m * p for p in range(B + 1)]
    if spatial_filter == "Similarity":
        host_tables, slices = _sim_slices(dist_sim_map, frame_distance)
        out, counts = pair_filter_batched(2, P0, P1, idx0, idx1, seg0, seg1, seg_m, tables=_upload(torch.from_numpy(host_tables), dev),
                                          slices=slices, thresh=similarity_thresh)
    else:
        out, counts = pair_filter_batched(0, P0, P1, idx0, idx1, seg0, seg1, seg_m, radius=float(radius))
    cnt = counts.cpu().tolist()          # HOST SYNCHRONISATION 1 of the label step: how many pairs the spatial filter kept per pair
    return matches, [out[seg_m[p]:seg_m[p] + cnt[p]] for p in range(B)]


def _under_pose_packed(P0, P1, seg0, seg1, T, n_sample, max_dist, pos_sel, generator):
    dev = P0.device
    B = len(seg0) - 1
    n0 = [seg0[p + 1] - seg0[p] for p in range(B)]
    if pos_sel is None:                   # the per-pair loop's draws, in pair order, from the same generator
        pos_sel = [torch.randperm(n, generator=generator)[:min(n, n_sample)] for n in n0]
    sels = [torch.as_tensor(s).to(torch.int64).reshape(-1) for s in pos_sel]
    seg_sel = _offsets([s.shape[0] for s in sels])
    nq = seg_sel[-1]
    # ONE upload: the draws, then per pair (bias0, bias1, number of draws)
    tail = torch.tensor([[seg0[p], seg1[p], seg_sel[p + 1] - seg_sel[p]] for p in range(B)], dtype=torch.int64).reshape(-1)
    if any(s.is_cuda for s in sels):
        up = torch.cat([s.to(dev) for s in sels] + [_upload(tail, dev)])
    else:
        up = _upload(torch.cat(sels + [tail]), dev)
    sel, tail = up[:nq], up[nq:].reshape(B, 3)
    meta = torch.empty(2 * B, dtype=torch.int32, device=dev)                 # status | counts: one read-back for both
    T = T.reshape(B, 16) if T.is_contiguous() else T.contiguous().reshape(B, 16)
    idx, _, _ = posed_nn_grid(P0, P1, seg0, seg1, T, float(max_dist), sel, seg_sel, status=meta[:B])
    out, _ = pair_filter_batched(1, P0, P1, sel, idx, seg0, seg1, seg_sel, T=T, radius=float(max_dist), counts=meta[B:])
    biased = out + torch.repeat_interleave(tail[:, :2], tail[:, 2], dim=0, output_size=nq)
    cnt = meta.cpu().tolist()[B:]        # HOST SYNCHRONISATION 2 of the label step: how many draws of every pair passed the gate
    unc = [out[seg_sel[p]:seg_sel[p] + cnt[p]] for p in range(B)]
    col = torch.cat([biased[seg_sel[p]:seg_sel[p] + cnt[p]] for p in range(B)])
    return unc, col


def correspondences_under_pose_batched(pcd0, pcd1, T, n_sample=5000, max_dist=2.0, pos_sel=None, generator=None):
    """``correspondences_under_pose`` for a batch: lists of per-pair clouds, ``T`` a DEVICE ``[B,4,4]`` fp32 tensor that is never
    sent to the host (where ``Matcher.SC2_PCR_packed`` wrote it).  Default draws: ``torch.randperm(n_b, generator=generator)
    [:n_sample]`` in pair order - the generator consumption of the per-pair loop - or ``pos_sel``, one selection per pair; uploaded
    once.  One grid search (``eyoc_posed_nn_grid``), one mode-1 batched filter, one read-back.  Returns ``(list of per-pair int64
    [M_b,2] views, collated int64 [sum M_b,2] with the biases of lib/trainer.py:1200-1221)`` on the device, each pair the bytes of
    ``correspondences_under_pose``; a pair with a non-finite pose gets an empty list."""
    P0, seg0 = _pack_clouds(pcd0)
    P1, seg1 = _pack_clouds(pcd1, P0.device)
    if not (isinstance(T, torch.Tensor) and T.is_cuda and T.dtype == torch.float32 and T.shape == (len(seg0) - 1, 4, 4)):
        raise ValueError("T must be a device fp32 tensor [B,4,4]")
    return _under_pose_packed(P0, P1, seg0, seg1, T, n_sample, max_dist, pos_sel, generator)


def corr_through_registration(pcd0, pcd1, uncollated_pairs, matcher, n_sample=5000, max_dist=2.0, pos_sel=None, generator=None,
                              on_degenerate="raise"):
    """lib/trainer.py:1153-1224 for the batch: the matched key points are gathered on the device, ``matcher.SC2_PCR_packed`` registers
    all pairs (each truncated to ``matcher.max_points`` like ``SC2_PCR_batch``) and ``correspondences_under_pose_batched`` runs on the
    poses where they lie.  Returns the reference's 5-tuple ``(T_ransac, correspondences, [], fitnesses, uncollated_corr)`` with
    ``T_ransac`` a device ``[B,4,4]`` tensor and ``fitnesses`` per-pair views.  ``on_degenerate="raise"``: a pair below SC2-PCR's
    minimum raises what the per-pair route raises; ``"skip"``: ``eyoc_registration_accept_degenerate`` is set for the call (and
    restored), such a pair keeps a NaN pose and gets an empty list, the others are untouched.  No host synchronisation besides the
    one of ``correspondences_under_pose_batched``."""
    if on_degenerate not in ("raise", "skip"):
        raise ValueError(on_degenerate)
    P0, seg0 = _pack_clouds(pcd0)
    dev = P0.device
    P1, seg1 = _pack_clouds(pcd1, dev)
    B = len(seg0) - 1
    us = [u.to(dev)[:int(matcher.max_points)] for u in uncollated_pairs]
    seg = _offsets([u.shape[0] for u in us])
    tail = torch.tensor([[seg0[p], seg1[p], seg[p + 1] - seg[p]] for p in range(B)], dtype=torch.int64)
    tail = _upload(tail, dev)
    rows = torch.cat(us) + torch.repeat_interleave(tail[:, :2], tail[:, 2], dim=0, output_size=seg[-1])
    src, tgt = P0.index_select(0, rows[:, 0]), P1.index_select(0, rows[:, 1])
    prev = _lib.knob("eyoc_registration_accept_degenerate", 1, device=dev) if on_degenerate == "skip" else None
    try:
        T, fit, n_seed = matcher.SC2_PCR_packed(src, tgt, seg)
    finally:
        if prev is not None:
            _lib.knob("eyoc_registration_accept_degenerate", prev, device=dev)
    unc, col = _under_pose_packed(P0, P1, seg0, seg1, T, n_sample, max_dist, pos_sel, generator)
    return T, col, [], [fit[b, :n_seed[b]] for b in range(B)], unc


def label_step(pcd0, F_batch_0, pcd1, F_batch_1, matcher, use_sc2_filtering=True, radius=20, feature_filter="Lowe",
               spatial_filter="Spherical", frame_distance=None, num_corres=5000, dist_sim_map=None, similarity_thresh=0.4, n_sample=5000,
               max_dist=2.0, generator=None, on_degenerate="raise"):
    """The labeler's output of one training iteration (lib/trainer.py:1295-1313): ``match_and_filter_corr_batched`` and, with
    ``use_sc2_filtering``, ``corr_through_registration``.  Returns ``(pos_pairs, uncollated_pairs, T_ransac, fitnesses)`` on the
    device (``T_ransac`` and ``fitnesses`` are ``None`` without SC2 filtering).  Two host synchronisations for any batch size: the
    counts after the spatial filter and the counts after the gate."""
    matches, uncollated = match_and_filter_corr_batched(pcd0, F_batch_0, pcd1, F_batch_1, radius, feature_filter, spatial_filter,
                                                        frame_distance, num_corres, dist_sim_map, similarity_thresh)
    if not use_sc2_filtering:
        return matches, uncollated, None, None
    T, pos_pairs, _, fitnesses, uncollated_corr = corr_through_registration(pcd0, pcd1, uncollated, matcher, n_sample, max_dist,
                                                                            generator=generator, on_degenerate=on_degenerate)
    return pos_pairs, uncollated_corr, T, fitnesses
