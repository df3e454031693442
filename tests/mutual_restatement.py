"""CPU restatement of the mutual nearest-neighbour contract (include/eyoc_hip.h, ``eyoc_knn1_mutual`` / ``eyoc_mutual_compact``), numpy.
Imports nothing from ``eyoc_amd``: it is what the GPU tests compare against byte for byte.

Everything is read off ONE distance matrix per segment, ``oracle.matching``'s bit-exact ones (``sqdist_rows`` for dist_type 0, ``pdist``
for 1, ``match_pair_distance`` for 2): the kernels' distances are symmetric bit for bit, so the matrix of (B, A) is this one transposed.

  * a candidate ``(i, j)`` is taken iff the kernel's ``v < best`` can succeed for it: a number below +inf in types 0 and 1; in type 2
    also a NaN, which stands below every number (the first one wins);
  * row / column arg-min over the taken candidates, ties to the lowest index; a row (column) without a taken candidate has NO
    neighbour: its index reads 0 and it is never mutual;
  * ``flags[i]``: bit 1 = row ``i`` has a neighbour ``j``, bit 0 = ``j`` has one too and it is ``i``;
  * compaction: per segment the rows with bit 0 in order - or, when there are fewer than ``min_keep`` of them, the rows with bit 1.

The ``defect`` argument plants ONE wrong rule (tests/test_mutual_restatement_host.py watches ``check`` catch each).
"""
from __future__ import annotations

import numpy as np

from oracle import matching as om

DIST = {"SquareL2": 0, "L2": 1, "GemmL2": 2}
DEFECTS = ("reverse_ties_high", "fallback_le", "unordered", "no_neighbour_mutual")


def distance_matrix(A, B, dist_type):
    """``[na, nb]`` fp32, the kernels' values bit for bit (type 2: NaN where the inner product exceeds 1 + 5e-7)."""
    A = np.ascontiguousarray(A, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    if dist_type == 0:
        return om.sqdist_rows(A, B)
    if dist_type == 1:
        return om.pdist(A, B, "L2")
    if dist_type == 2:
        return om.match_pair_distance(A, B)
    raise ValueError(dist_type)


def _argmin_rows(D, dist_type, ties_high=False):
    """-> ``(idx int64 [rows], has bool [rows])`` of the row minima of ``D`` under the candidate rule above."""
    n, m = D.shape
    idx, has = np.zeros(n, np.int64), np.zeros(n, bool)
    if m == 0:
        return idx, has
    with np.errstate(invalid="ignore"):
        key = D.astype(np.float64)
        nan = np.isnan(key)
        taken = (key < np.inf) | (nan if dist_type == 2 else False)
        key = np.where(nan, -1.0, key)                   # type 2: below every distance (those are >= 0)
    key = np.where(taken, key, np.inf)
    has = taken.any(axis=1)
    if ties_high:
        idx = (m - 1 - np.argmin(key[:, ::-1], axis=1)).astype(np.int64)
    else:
        idx = np.argmin(key, axis=1).astype(np.int64)    # first minimum = lowest index
    return np.where(has, idx, 0), has


def segment(A, B, dist_type, defect=None):
    """One segment -> ``(idx_ab int64 [na], idx_ba int64 [nb], flags uint8 [na])``."""
    D = distance_matrix(A, B, dist_type)
    idx_ab, has_a = _argmin_rows(D, dist_type)
    idx_ba, has_b = _argmin_rows(D.T, dist_type, ties_high=defect == "reverse_ties_high")
    if len(B) == 0:
        return idx_ab, idx_ba, np.zeros(len(A), np.uint8)
    j = idx_ab
    mutual = has_a & has_b[j] & (idx_ba[j] == np.arange(len(A)))
    if defect == "no_neighbour_mutual":                  # the index 0 of a row / column without a neighbour taken at face value
        mutual = idx_ba[j] == np.arange(len(A))
    return idx_ab, idx_ba, (mutual.astype(np.uint8) | (has_a.astype(np.uint8) << 1))


def search(A, B, seg_a, seg_b, dist_type, defect=None):
    """All segments -> ``(idx_ab [len(A)], idx_ba [len(B)], flags [len(A)])``, indices local to the segment."""
    A = np.ascontiguousarray(A, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    idx_ab, idx_ba, flags = np.zeros(len(A), np.int64), np.zeros(len(B), np.int64), np.zeros(len(A), np.uint8)
    for s in range(len(seg_a) - 1):
        a0, a1, b0, b1 = int(seg_a[s]), int(seg_a[s + 1]), int(seg_b[s]), int(seg_b[s + 1])
        idx_ab[a0:a1], idx_ba[b0:b1], flags[a0:a1] = segment(A[a0:a1], B[b0:b1], dist_type, defect)
    return idx_ab, idx_ba, flags


def compact(idx_ab, flags, seg_a, min_keep=0, defect=None):
    """-> ``(rows int64 [m], corr int64 [m], seg_out int32 [nseg + 1])``: rows inside their segment, stable."""
    rows, corr, seg_out = [], [], [0]
    for s in range(len(seg_a) - 1):
        a0, a1 = int(seg_a[s]), int(seg_a[s + 1])
        f = flags[a0:a1]
        keep = (f & 1) != 0
        count = int(keep.sum())
        if (count <= min_keep and min_keep > 0) if defect == "fallback_le" else count < min_keep:
            keep = (f & 2) != 0
        r = np.flatnonzero(keep).astype(np.int64)
        if defect == "unordered":
            r = r[::-1]
        rows.append(r)
        corr.append(idx_ab[a0:a1][r])
        seg_out.append(seg_out[-1] + len(r))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)    # noqa: E731
    return cat(rows), cat(corr), np.asarray(seg_out, np.int32)


def check(got, A, B, seg_a, seg_b, dist_type, min_keep=0):
    """``got = (idx_ab, idx_ba, flags, rows, corr, seg_out)`` (numpy) against the restatement, byte for byte; raises ``AssertionError``
    naming the first output that differs."""
    idx_ab, idx_ba, flags = search(A, B, seg_a, seg_b, dist_type)
    rows, corr, seg_out = compact(idx_ab, flags, seg_a, min_keep)
    want = (idx_ab, idx_ba, flags, rows, corr, seg_out)
    for name, g, w in zip(("idx_ab", "idx_ba", "flags", "rows", "corr", "seg_out"), got, want):
        if g is None:
            continue
        g = np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), \
            f"{name} differs from the restatement ({g.dtype}{g.shape} vs {w.dtype}{w.shape})"


def mutual_share(flags):
    return float(((np.asarray(flags) & 1) != 0).mean()) if len(flags) else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs shared by the host and the GPU tests
def unit_rows(seed, n, c):
    """Seeded unit-norm Gaussian rows, fp32."""
    x = np.random.default_rng(seed).normal(size=(n, c)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


SHAPES = ((1, 1), (1, 9), (9, 1), (63, 9), (64, 8), (65, 33), (257, 255), (300, 31), (31, 300))
WIDTHS = (4, 16, 32, 64, 128)
WIDE_SHAPES = ((65, 33), (257, 255))      # the shapes every width runs at


def pair_inputs(na, nb, c, seed=0):
    return unit_rows(1000 * seed + 2 * c + 1, na, c), unit_rows(1000 * seed + 2 * c + 2, nb, c)


def fallback_case(k, c=32, extra=9, seed=5):
    """An exact mutual count: ``k`` source rows EQUAL to ``k`` distinct targets (distance exactly 0, mutual), and ``extra`` further rows
    all nearest to one further target ``t`` at distinct distances (a small step along one direction orthogonal to nothing in particular,
    scaled 1, 2, ... so the nearest of them is the one ``t`` prefers): ``k + 1`` mutual rows.  -> ``(A, B)``, ``len(A) = k + extra``."""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(k + 1, c)).astype(np.float32) * 4.0            # far apart: every planted row stays nearest to its own target
    step = rng.normal(size=c).astype(np.float32)
    step = step / np.linalg.norm(step) * np.float32(0.01)
    rest = np.stack([B[k] + step * np.float32(e + 1) for e in range(extra)])
    return np.concatenate([B[:k], rest]).astype(np.float32), B
