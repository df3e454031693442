"""FPFH (``eyoc_fpfh_batched``, include/eyoc_hip.h "FPFH descriptors") restated in numpy fp64: a brute-force ``n x n`` sweep, no grid, no
code shared with the kernels.  ``fpfh_rows`` returns, per row, the neighbour list, the 33 counts, ``k``, ``F`` and which rows are
UNDECIDED: rows for which a last-ulp difference between two ``acos`` / ``atan2`` implementations could change a bin or the swap, and
(for ``F``) rows that read the histogram of such a row.  That flag has no other use.

Also here, because the host test and the GPU test must use the very same things: the inputs (``wavy_cloud``, ``cubic_lattice``,
``planar_lattice``), the comparison (``check_against``) and the planted defects of the restatement (``fpfh_rows(defect=...)``)."""
from types import SimpleNamespace

import numpy as np

EPS = 1e-9
BINS = 33
DEFECTS = ("no_d2_guard", "inv_d", "no_self_term", "loose_swap")


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def pair_features(p1, n1, p2, n2, loose_swap=False):
    """Open3D's ComputePairFeatures for row ``(p1, n1)`` against the rows ``(p2, n2) [k, 3]`` -> ``f [k, 3]`` and ``near [k]``: the swap
    decision hangs on less than ``EPS``."""
    k = p2.shape[0]
    f = np.zeros((k, 3))
    d = p2 - p1
    ln = np.sqrt(_dot(d, d))
    ok = ln != 0.0
    n1 = np.broadcast_to(n1, (k, 3)).copy()
    n2 = n2.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        a1, a2 = _dot(n1, d) / ln, _dot(n2, d) / ln
        c1, c2 = np.arccos(np.abs(a1)), np.arccos(np.abs(a2))
        swap = (c1 >= c2) if loose_swap else (c1 > c2)       # NaN compares false: no swap
        gap = np.abs(c1 - c2)
        near = ok & (gap > 0.0) & (gap < EPS)
        f2 = np.where(swap, -a2, a1)
        m1 = np.where(swap[:, None], n2, n1)
        m2 = np.where(swap[:, None], n1, n2)
        d = np.where(swap[:, None], -d, d)
        v = _cross(d, m1)
        vn = np.sqrt(_dot(v, v))
        ok = ok & (vn != 0.0)
        v = v / vn[:, None]
        w = _cross(m1, v)
        f1 = _dot(v, m2)
        f0 = np.arctan2(_dot(w, m2), _dot(m1, m2))
    f[ok, 0], f[ok, 1], f[ok, 2] = f0[ok], f1[ok], f2[ok]
    return f, near


def bin_coordinates(f):
    """``[k, 3]`` features -> the three bin coordinates in units of a bin (before floor and clamp)."""
    return np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) * 0.5, 11.0 * (f[:, 2] + 1.0) * 0.5], 1)


def fpfh_rows(pts, normals, radius, max_nn, defect=None):
    """One cloud: ``pts / normals f32 [n, 3]``.  ``defect``: one of ``DEFECTS`` - a deliberately wrong statement, for the tests that show
    the comparison notices it."""
    assert defect is None or defect in DEFECTS
    x, nr = np.asarray(pts, np.float32).astype(np.float64), np.asarray(normals, np.float32).astype(np.float64)
    n = x.shape[0]
    r2 = float(radius) * float(radius)
    d = x[None, :, :] - x[:, None, :]                      # d[i, j] = x_j - x_i
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    lists, dists = [], []
    k = np.zeros(n, np.int64)
    cnt = np.zeros((n, BINS), np.int64)
    und_hist = np.zeros(n, bool)
    for i in range(n):
        inside = np.flatnonzero(d2[i] < r2)
        order = inside[np.lexsort((inside, d2[i, inside]))][:max_nn]        # by (d2, j)
        nb = order[order != i][:max_nn - 1]
        lists.append(nb)
        dists.append(d2[i, nb])
        k[i] = nb.size
        und_hist[i] = bool((np.abs(d2[i] - r2) < EPS * r2).any())     # a row at the radius: the list itself could differ
        if nb.size == 0:
            continue
        f, near = pair_features(x[i], nr[i], x[nb], nr[nb], loose_swap=defect == "loose_swap")
        t = bin_coordinates(f)
        # only the edges 1..10 separate two bins: below 1 and above 10 the clamp takes everything
        edge = np.rint(t)
        und_hist[i] |= bool(near.any() or ((np.abs(t - edge) < EPS) & (edge >= 1.0) & (edge <= 10.0)).any())
        b = np.clip(np.floor(t), 0, 10).astype(np.int64) + np.array([0, 11, 22])
        np.add.at(cnt[i], b.ravel(), 1)
    S = np.zeros((n, BINS))
    has = k > 0
    S[has] = cnt[has] * (100.0 / k[has])[:, None]
    F = np.zeros((n, BINS))
    und_F = und_hist.copy()
    for i in range(n):
        if k[i] == 0:
            continue
        nb, dd = lists[i], dists[i]
        und_F[i] |= bool(und_hist[nb].any())
        use = np.ones(nb.size, bool) if defect == "no_d2_guard" else dd > 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            T = S[nb[use]] / (np.sqrt(dd[use]) if defect == "inv_d" else dd[use])[:, None]
            W = T.sum(0)
            G = W.reshape(3, 11).sum(1)
            scale = np.where(G != 0.0, 100.0 / G, 0.0)
            F[i] = W * np.repeat(scale, 11) + (0.0 if defect == "no_self_term" else S[i])
    with np.errstate(invalid="ignore"):
        Fn = F / (np.sqrt((F * F).sum(1)) + 1e-6)[:, None]
    return SimpleNamespace(lists=lists, d2=dists, k=k, cnt=cnt, F=F, Fn=Fn, undecided_hist=und_hist, undecided_F=und_F)


def ulp_distance(a, b):
    """Distance in fp32 steps between two float32 arrays (finite, any sign)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def check_against(ref, hist=None, count=None, feat=None, feat_normalized=None, max_undecided=0.01):
    """What the GPU test asserts: at most 1 % of the rows undecided; ``hist`` / ``count`` EXACTLY the restatement's on decided rows;
    ``feat`` (and the normalised rows) within one fp32 step of ``float32(F)`` on rows whose ``F`` is decided - both sides round one fp64
    value once, and the two fp64 values differ by the summation order of at most 127 non-negative terms."""
    n = ref.k.shape[0]
    if n:
        assert ref.undecided_F.mean() <= max_undecided, f"{ref.undecided_F.sum()} of {n} rows undecided"
    dh, dF = ~ref.undecided_hist, ~ref.undecided_F
    if count is not None:
        np.testing.assert_array_equal(np.asarray(count)[dh], ref.k[dh])
    if hist is not None:
        np.testing.assert_array_equal(np.asarray(hist)[dh].astype(np.int64), ref.cnt[dh])
    for got, want in ((feat, ref.F), (feat_normalized, ref.Fn)):
        if got is None:
            continue
        got = np.asarray(got)[:, :BINS]
        assert np.isfinite(got[dF]).all(), "non-finite feature"
        dist = ulp_distance(got[dF], want[dF].astype(np.float32))
        assert dist.max(initial=0) <= 1, f"feature off by {dist.max()} fp32 steps"


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
WAVY = dict(radius=0.45, max_nn=40)


def wavy_cloud(seed, n=700, side=5.6):
    """``n`` random points of the surface ``z = 0.3 sin(x) cos(y)`` over a square, with the surface's unit normal jittered by a few degrees:
    at radius 0.45 a row has between 2 and about 26 neighbours."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, side, (n, 2))
    z = 0.3 * np.sin(xy[:, 0]) * np.cos(xy[:, 1])
    nrm = np.stack([-0.3 * np.cos(xy[:, 0]) * np.cos(xy[:, 1]), 0.3 * np.sin(xy[:, 0]) * np.sin(xy[:, 1]), np.ones(n)], 1)
    nrm += rng.normal(0.0, 0.05, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([xy, z[:, None]], 1).astype(np.float32), nrm.astype(np.float32)


def cubic_lattice(seed, m=6, step=0.25):
    """``m^3`` lattice points (distances tie in large groups) with random unit normals."""
    rng = np.random.default_rng(seed)
    g = np.arange(m, dtype=np.float64) * step
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    nrm = rng.normal(size=pts.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pts.astype(np.float32), nrm.astype(np.float32)


def planar_lattice(m=6, extra_lone=2):
    """An ``m x m`` integer lattice in the plane z = 0 with all normals (0, 0, 1), and ``extra_lone`` points far from everything."""
    g = np.arange(m, dtype=np.float64)
    pts = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.zeros((m, m))], -1).reshape(-1, 3)
    lone = np.array([[1000.0 + 50.0 * i, -500.0, 77.0] for i in range(extra_lone)]).reshape(-1, 3)
    pts = np.concatenate([pts, lone])
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (pts.shape[0], 1))
    return pts.astype(np.float32), nrm.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the end-to-end pair: a scene with corners and edges, and its moved, permuted, thinned copy
# ---------------------------------------------------------------------------------------------------------------------
SCENE = dict(voxel_size=0.3, distance_threshold=0.15, seed=11, drop=0.15)


def _patch(origin, u, v, nu, nv, step):
    a, b = np.meshgrid(np.arange(nu) * step, np.arange(nv) * step, indexing="ij")
    return np.asarray(origin, np.float64) + a.reshape(-1, 1) * np.asarray(u, np.float64) + b.reshape(-1, 1) * np.asarray(v, np.float64)


def corner_scene(seed=SCENE["seed"], step=SCENE["voxel_size"], drop=SCENE["drop"]):
    """A floor, two walls of different size, a box and a ramp around a sensor at the origin (no symmetry maps the scene to itself), one
    point per ``step`` with a little jitter.  -> ``(src f32 [n, 3], tgt f32 [m, 3], T f64 [4, 4])``: ``tgt`` is ``T src`` with ``drop`` of
    the rows removed and the rest permuted.  The motion is small enough that the origin sees every surface from the same side in both
    frames, so normals that point to the origin agree between the two."""
    rng = np.random.default_rng(seed)
    parts = [
        _patch([-2.1, -1.8, -1.2], [1, 0, 0], [0, 1, 0], 14, 12, step),          # floor
        _patch([-2.1, -1.8, -0.9], [0, 1, 0], [0, 0, 1], 12, 7, step),           # wall x = -2.1
        _patch([-1.8, 1.8, -0.9], [1, 0, 0], [0, 0, 1], 10, 5, step),            # wall y = 1.8, shorter and lower
        _patch([0.9, -1.2, -0.9], [0, 1, 0], [0, 0, 1], 3, 3, step),             # box: the face towards the sensor
        _patch([0.9, -1.2, -0.3], [1, 0, 0], [0, 1, 0], 3, 3, step),             # box: top
        _patch([0.9, -0.3, -0.9], [1, 0, 0], [0, 0, 1], 3, 2, step),             # box: side
        _patch([0.6, 0.6, -1.2], [1, 0, 0], [0, 0.8, 0.6], 4, 4, step),          # ramp
    ]
    src = np.concatenate(parts) + rng.normal(0.0, 0.01, (sum(len(p) for p in parts), 3))
    az, tilt = np.deg2rad(17.0), np.deg2rad(4.0)
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(tilt), -np.sin(tilt)], [0, np.sin(tilt), np.cos(tilt)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Rx
    T[:3, 3] = [0.35, -0.25, 0.1]
    src = src.astype(np.float32)
    keep = rng.permutation(len(src))[:int(round(len(src) * (1.0 - drop)))]
    tgt = (src[keep].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return src, tgt, T


def registered(T_est, T_gt, rte_thresh=2.0, rre_thresh=5.0):
    """The reference's criterion (scripts/test_kitti.py:187-206 with the thresholds of its run scripts)."""
    rte = np.linalg.norm(T_est[:3, 3] - T_gt[:3, 3])
    m = T_est[:3, :3].T @ T_gt[:3, :3]
    m[[0, 1, 2], [0, 1, 2]] = np.minimum(1.0, m[[0, 1, 2], [0, 1, 2]])
    rre = np.arccos((np.trace(m) - 1.0) / 2.0)
    return bool(rte < rte_thresh and not np.isnan(rre) and rre < np.pi / 180.0 * rre_thresh), float(rte), float(np.rad2deg(rre))
