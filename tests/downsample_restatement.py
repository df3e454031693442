"""The contract of ``eyoc_voxel_downsample_batched`` (include/eyoc_hip.h) in numpy fp64, sharing no method with the kernel: no sort of
packed keys, no run heads, no scan.  Cells come from ``np.unique(axis=0)``, re-ordered by first index; the sums are built by adding
the k-th point of every voxel for k = 0, 1, ...: sequential per voxel (the contract's order), vectorised across voxels."""
import numpy as np

RANGE = 8                      # eyoc_amd.icp.RANGE
MAX_CELLS = 1 << 17


def restate_cloud(pts, voxel_size, attrs=None, reverse=False):
    """One cloud: ``pts f32 [n, >= 3]`` -> dict of ``xyz f32 [m, 3]``, ``attrs f32 [m, c]`` (or None), ``first`` / ``count int32 [m]``,
    ``inverse int32 [n]``, ``status``.  ``reverse``: the sums run from the highest point index down (NOT the contract: the order test)."""
    p = np.asarray(pts, np.float32)[:, :3]
    n = p.shape[0]
    a = None if attrs is None else np.asarray(attrs, np.float32).reshape(n, np.shape(attrs)[-1])
    c_attr = 0 if a is None else a.shape[1]
    v = np.float64(voxel_size)

    def result(xyz, att, first, count, inverse, status):
        return dict(xyz=xyz.astype(np.float32).reshape(-1, 3), attrs=None if a is None else att.astype(np.float32).reshape(-1, c_attr),
                    first=first.astype(np.int32), count=count.astype(np.int32), inverse=inverse.astype(np.int32), status=int(status))

    none = np.zeros(0)
    if n == 0:
        return result(none, none, none, none, none, 0)
    refused = result(none, none, none, none, np.full(n, -1), RANGE)
    if not np.isfinite(p).all():
        return refused
    p64 = p.astype(np.float64)
    vmin = p64.min(0) - 0.5 * v
    with np.errstate(over="ignore"):
        if not (np.floor((p64.max(0) - vmin) / v) < MAX_CELLS).all():
            return refused
    cells = np.floor((p64 - vmin) / v).astype(np.int64)
    _, idx, inv, cnt = np.unique(cells, axis=0, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(idx, kind="stable")                # voxels by their lowest point index
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    first, count, inverse = idx[order], cnt[order], rank[np.asarray(inv).ravel()]
    members = np.argsort(inverse, kind="stable")          # points grouped by row, ascending inside a row
    starts = np.concatenate([[0], np.cumsum(count)[:-1]])
    cols = p64 if a is None else np.concatenate([p64, a.astype(np.float64)], 1)
    s = np.zeros((len(count), cols.shape[1]))
    for k in range(int(count.max())):
        live = count > k
        at = starts[live] + (count[live] - 1 - k if reverse else k)
        s[live] = s[live] + cols[members[at]]
    mean = s / count[:, None].astype(np.float64)
    return result(mean[:, :3], mean[:, 3:], first, count, inverse, 0)


def restate_batch(pts, seg, voxel_size, attrs=None, reverse=False):
    """The clouds ``seg[b]:seg[b+1]`` of ``pts`` -> the concatenated outputs, ``seg_out`` (list) and ``status int32 [B]``."""
    pts = np.asarray(pts, np.float32)
    seg = [int(x) for x in seg]
    parts = [restate_cloud(pts[seg[b]:seg[b + 1]], voxel_size, None if attrs is None else np.asarray(attrs)[seg[b]:seg[b + 1]], reverse)
             for b in range(len(seg) - 1)]
    out = {k: np.concatenate([q[k] for q in parts]) for k in ("xyz", "first", "count", "inverse")}
    out["attrs"] = None if attrs is None else np.concatenate([q["attrs"] for q in parts])
    out["seg_out"] = [0] + [int(x) for x in np.cumsum([len(q["count"]) for q in parts])]
    out["status"] = np.array([q["status"] for q in parts], np.int32)
    return out
