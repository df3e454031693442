"""CPU restatement of the radius-match contract (include/eyoc_hip.h, "Ground-truth matching indices"), numpy fp64.  Imports nothing
from ``eyoc_amd``: it is what the GPU tests compare against, exactly - both sides evaluate the same fp64 expression on the same fp32
inputs, so pairs, order and the bits of d2 must agree without a tolerance.

``brute`` decides over ALL n0 x n1 candidates; ``tree`` takes its candidates from ``cKDTree.query_ball_point`` with a slightly larger
radius and decides them by the same expression (tests/test_matches_host.py compares the two bit for bit).  ``status`` restates the
per-pair status, ``collate`` the shift of ``collate_pair_fn`` (lib/data_loaders.py:48-72).
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

from icp_restatement import _d2, pose

BAD_INIT, RANGE = 2, 8
EDGE_MARGIN = 1.0 + 2.0 ** -20      # cell edge = radius * EDGE_MARGIN in fp64; cells are floor(v / edge), valid in [-2^17, 2^17)

_EMPTY = (np.zeros((0, 2), np.int64), np.zeros(0, np.float64))


def _f32(a):
    return np.asarray(a, np.float32).reshape(-1, 3)


def _T(T):
    return np.eye(4) if T is None else np.asarray(T, np.float64).reshape(4, 4)


def status(src, tgt, T, r) -> int:
    T = _T(T)
    if not np.isfinite(T).all():
        return BAD_INIT
    src, tgt = _f32(src), _f32(tgt)
    if not (np.isfinite(src).all() and np.isfinite(tgt).all()):
        return RANGE
    edge = r * EDGE_MARGIN
    with np.errstate(over="ignore", invalid="ignore"):
        cells = np.concatenate([np.floor(tgt.astype(np.float64) / edge), np.floor(pose(src, T) / edge)])
    return 0 if ((cells >= -2.0 ** 17) & (cells < 2.0 ** 17)).all() else RANGE


def _rows(i, d, j, K):
    """The list of source row ``i``: matches ``j`` with squared distances ``d`` -> ascending by (d2, j), the first K."""
    o = np.lexsort((j, d))
    if K:
        o = o[:K]
    return np.stack([np.full(len(o), i, np.int64), j[o].astype(np.int64)], 1), d[o]


def _gather(rows):
    if not rows:
        return _EMPTY
    return np.concatenate([p for p, _ in rows]), np.concatenate([d for _, d in rows])


def brute(src, tgt, T, r, K=None, block=512):
    """-> ``(pairs int64 [m, 2], d2 f64 [m])`` of one pair, local rows; a pair with a status has none."""
    if status(src, tgt, T, r):
        return _EMPTY
    p, q = pose(_f32(src), _T(T)), _f32(tgt).astype(np.float64)
    if len(p) == 0 or len(q) == 0:
        return _EMPTY
    r2 = r * r
    out = []
    for a in range(0, len(p), block):
        d = _d2(p[a:a + block, None, :], q[None])
        for i in range(d.shape[0]):
            j = np.flatnonzero(d[i] < r2)
            if len(j):
                out.append(_rows(a + i, d[i, j], j, K))
    return _gather(out)


def tree(src, tgt, T, r, K=None):
    """The same decision on the candidates of a KD-tree ball query of radius r (1 + 1e-9)."""
    if status(src, tgt, T, r):
        return _EMPTY
    p, q = pose(_f32(src), _T(T)), _f32(tgt).astype(np.float64)
    if len(p) == 0 or len(q) == 0:
        return _EMPTY
    r2 = r * r
    out = []
    for i, cand in enumerate(cKDTree(q).query_ball_point(p, r * (1 + 1e-9))):
        j = np.asarray(sorted(cand), np.int64)
        if len(j) == 0:
            continue
        d = _d2(p[i][None], q[j])
        keep = d < r2
        if keep.any():
            out.append(_rows(i, d[keep], j[keep], K))
    return _gather(out)


def counts(src, tgt, T, r, K=None):
    """Matches per source row (after K)."""
    pairs, _ = brute(src, tgt, T, r, K)
    return np.bincount(pairs[:, 0], minlength=len(_f32(src)))


def collate(pairs_list, n0, n1):
    """Per-pair local ``[m, 2]`` arrays -> one array with the rows shifted by the running cloud sizes, and the pairs' offsets in it.
    Every pair moves the head, also one without matches."""
    out, seg, s0, s1 = [], [0], 0, 0
    for pr, a, b in zip(pairs_list, n0, n1):
        out.append(np.asarray(pr, np.int64).reshape(-1, 2) + np.array([[s0, s1]], np.int64))
        seg.append(seg[-1] + len(out[-1]))
        s0, s1 = s0 + int(a), s1 + int(b)
    return (np.concatenate(out) if out else np.zeros((0, 2), np.int64)), np.asarray(seg, np.int64)


def overlap_ratio(pcd0, pcd1, T, voxel_size):
    """util/pointcloud.py:42-50 on clouds that are already down-sampled."""
    T = _T(T)
    c01, c10 = counts(pcd0, pcd1, T, voxel_size, 1), counts(pcd1, pcd0, np.linalg.inv(T), voxel_size, 1)
    return max(int(c01.sum()) / len(c01), int(c10.sum()) / len(c10))
