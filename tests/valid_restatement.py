"""fp64 numpy restatement of ``eyoc_valid_metrics_batched`` for ONE pair: the metrics of the reference's validation loop
(lib/trainer.py:362-378, lib/metrics.py:13-19) on fp32 inputs, every product and sum in the order the kernel uses and unfused, so that the
integer fields and the sign of ``cos_rre - 1`` can be compared exactly and the float fields to fp64 rounding of the long sums."""
import json

import numpy as np

EMPTY, BAD_INDEX, POSE_NONFINITE = 1, 2, 4


def _apply(T, x):
    """``R x + t`` row by row, ``((T0 x + T1 y) + T2 z) + T3``."""
    ox, oy, oz = x[:, 0], x[:, 1], x[:, 2]
    return [T[i, 0] * ox + T[i, 1] * oy + T[i, 2] * oz + T[i, 3] for i in range(3)]


def hit_distances(p0, p1, idx1, T_gt):
    """``sqrt(|R_gt p0 + t_gt - p1[idx1]|^2 + 1e-6)`` per correspondence (``idx1`` must be valid)."""
    p0, p1, G = np.asarray(p0, np.float64), np.asarray(p1, np.float64), np.asarray(T_gt, np.float64).reshape(4, 4)
    q = p1 if idx1 is None else p1[np.asarray(idx1)]
    g = _apply(G, p0)
    gx, gy, gz = g[0] - q[:, 0], g[1] - q[:, 1], g[2] - q[:, 2]
    return np.sqrt(gx * gx + gy * gy + gz * gz + 1e-6)


def valid_record(p0, p1, idx1, x0, T_est, T_gt, hit_thresh=0.1, max_dist=1.0):
    """-> dict with the fields of ``eyoc_valid_record``."""
    assert np.asarray(T_est).dtype == np.float32 and np.asarray(T_gt).dtype == np.float32
    p0, p1, x0 = (np.asarray(a, np.float32).reshape(-1, 3) for a in (p0, p1, x0))
    E, G = np.asarray(T_est, np.float64).reshape(4, 4), np.asarray(T_gt, np.float64).reshape(4, 4)
    n, n1, nx = len(p0), len(p1), len(x0)
    finite = bool(np.isfinite(E).all())
    status = (EMPTY if n == 0 else 0) | (0 if finite else POSE_NONFINITE)
    nan = float("nan")
    hits = 0
    if n > 0:
        idx = np.arange(n) if idx1 is None else np.asarray(idx1, np.int64)
        bad = (idx < 0) | (idx >= n1)
        if bad.any() or n1 == 0:
            status |= BAD_INDEX
        if n1 > 0:
            hits = int((hit_distances(p0, p1, np.clip(idx, 0, n1 - 1), G) < hit_thresh).sum())
    bad = bool(status & BAD_INDEX)
    rec = {"status": status, "n_corr": n, "n_points": nx, "hits": 0 if bad else hits,
           "hit_ratio": nan if (n == 0 or bad) else hits / n}
    with np.errstate(invalid="ignore", over="ignore"):
        if finite and nx > 0 and n > 0:
            e, g = _apply(E, x0.astype(np.float64)), _apply(G, x0.astype(np.float64))
            ex, ey, ez = e[0] - g[0], e[1] - g[1], e[2] - g[2]
            rec["loss"] = float(np.minimum(np.sqrt(ex * ex + ey * ey + ez * ez), max_dist).sum() / nx)
        else:
            rec["loss"] = nan
        dx, dy, dz = E[0, 3] - G[0, 3], E[1, 3] - G[1, 3], E[2, 3] - G[2, 3]
        rec["rte"] = float(np.sqrt(dx * dx + dy * dy + dz * dz)) if finite else nan
        tr = 0.0
        for i in range(3):
            for j in range(3):
                tr = tr + E[i, j] * G[i, j]
        c = (tr - 1.0) / 2.0
        rec["cos_rre"] = float(c)
        rec["rre"] = float(np.arccos(c)) if (finite and -1.0 <= c <= 1.0) else nan
    return rec


# ---- the fixture g12_valid.npz (tests/golden/make_golden_valid.py): its cases and the bars a record is held to against it

def g12_cases(g):
    """-> [(case index, variant, p0, p1, x0, T_est, T_gt)] of the fixture, inputs regenerated from the seeds."""
    import _inputs_valid as gv
    out = []
    for c, (seed, n, frac, tp) in enumerate(json.loads(str(g["cases"]))):
        for v in (0, 1):
            p0, p1, x0, T_gt = gv.valid_case(seed, n, frac, tp, bool(v))
            out.append((c, v, p0, p1, x0, g[f"T_est{c}"], T_gt))
    return out


def check_against_g12(g, c, v, rec, n):
    """The bars a record - the restatement's or the device's - is held to against the reference's outputs."""
    loss_bar = 4 * float(g["loss_gap"].max()) + 1e-7       # reference (fp32) and restatement each sit within their own rounding of the true value
    assert rec["hits"] == round(float(g["hit_ratio"][c, v]) * n), (c, v)
    assert abs(rec["loss"] - g["loss"][c, v]) <= loss_bar, (c, v, rec["loss"], g["loss"][c, v])
    assert abs(rec["rte"] - g["rte"][c, v]) <= 1e-5, (c, v)
    assert abs(rec["cos_rre"] - g["cos_rre"][c, v]) <= 1e-6, (c, v)
    if v == 1:      # the offset cases only: near the identity acos amplifies 1e-7 into 3e-4 and the cosine's side of 1 is not reproducible
        assert abs(rec["rre"] - g["rre"][c, v]) <= 1e-4, (c, v)
