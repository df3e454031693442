"""CPU restatement of the two contracts behind point-to-plane ICP (include/eyoc_hip.h, "Normal estimation for a batch of clouds" and
"Point-to-plane ICP for a batch of pairs"), numpy fp64.  Imports nothing from ``eyoc_amd``: it is what the GPU tests compare against.

``normals``: candidates come from ``scipy.spatial.cKDTree`` (a ball a little wider than the radius), the neighbour set is decided by the
contract's expression on those candidates - d = x_j - x_i, d2 = (dx dx + dy dy) + dz dz in fp64, a neighbour iff d2 < fl(radius^2),
ordered by (d2, j), cut to the first ``max_nn`` (0 = all).  ``neighbours_brute`` is the same decision over all n x n candidates.  The
eigenvectors come from ``numpy.linalg.eigh``, not from a Jacobi sweep.

``icp_plane``: ``icp_restatement.evaluate`` for the evaluation, ``numpy.linalg.lstsq`` on the stacked Jacobian for the step (not the
normal equations); only the SINGULAR rule looks at the normal equations, because it is stated on their LDL^T pivots.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.spatial import cKDTree

import icp_restatement as R

CONVERGED, BAD_INIT, FEW, RANGE, SINGULAR = 1, 2, 4, 8, 16
U64 = 2.0 ** -53


# ---- normals

def _d2(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _cut(i, j, d2, n, max_nn):
    """flat candidates (row i, neighbour j, d2, already inside the radius) -> the same arrays ordered by (i, d2, j) and cut per row"""
    o = np.lexsort((j, d2, i))
    i, j, d2 = i[o], j[o], d2[o]
    first = np.searchsorted(i, np.arange(n))
    rank = np.arange(len(i)) - first[i]
    keep = rank < max_nn if max_nn > 0 else np.ones(len(i), bool)
    return i[keep], j[keep], d2[keep]


def neighbours(pts, radius, max_nn):
    """-> (i, j, d2): the neighbour lists of all rows, flat, ordered by (i, d2, j)"""
    x = np.asarray(pts, np.float32).astype(np.float64)
    r2 = radius * radius
    lists = cKDTree(x).query_ball_point(x, radius * (1.0 + 1e-9) + 1e-12, workers=-1)
    i = np.repeat(np.arange(len(x)), [len(l) for l in lists])
    j = np.concatenate([np.asarray(l, np.int64) for l in lists]) if len(x) else np.zeros(0, np.int64)
    d2 = _d2(x[j] - x[i])
    m = d2 < r2
    return _cut(i[m], j[m], d2[m], len(x), max_nn)


def neighbours_brute(pts, radius, max_nn):
    x = np.asarray(pts, np.float32).astype(np.float64)
    d2 = _d2(x[None, :, :] - x[:, None, :])         # [i, j] = |x_j - x_i|^2
    i, j = np.nonzero(d2 < radius * radius)
    return _cut(i, j, d2[i, j], len(x), max_nn)


@dataclass
class Normals:
    normals: np.ndarray     # f64 [n, 3], zero where k < 3
    k: np.ndarray           # int64 [n]
    lam: np.ndarray         # f64 [n, 3]: eigenvalues, descending
    beta: np.ndarray        # f64 [n]: 256 k 2^-53 lam1 / (lam2 - lam3), +inf where lam2 == lam3 (or k < 3)


def normals(pts, radius, max_nn=30) -> Normals:
    """The contract's normals.  ``beta`` bounds the angle between this normal and any other correct evaluation of the contract:
    Davis-Kahan gives sin(angle) <= |E| / (lam2 - lam3) for a perturbation E of the covariance, and two fp64 summations of k terms of
    size <= lam1-ish differ by a few k 2^-53 lam1; 256 is a generous constant over that."""
    x = np.asarray(pts, np.float32).astype(np.float64)
    n = len(x)
    i, j, _ = neighbours(x, radius, max_nn)
    k = np.bincount(i, minlength=n).astype(np.int64)
    d = x[j] - x[i]
    S1 = np.stack([np.bincount(i, d[:, a], n) for a in range(3)], 1)
    S2 = np.stack([np.stack([np.bincount(i, d[:, a] * d[:, b], n) for b in range(3)], 1) for a in range(3)], 1)
    kk = np.maximum(k, 1).astype(np.float64)
    m = S1 / kk[:, None]
    C = S2 / kk[:, None, None] - m[:, :, None] * m[:, None, :]
    w, v = np.linalg.eigh(C)                      # ascending
    nv = v[:, :, 0]
    nv = nv / np.linalg.norm(nv, axis=1, keepdims=True)
    dot = (nv[:, 0] * x[:, 0] + nv[:, 1] * x[:, 1]) + nv[:, 2] * x[:, 2]
    first = np.where(nv[:, 0] != 0, nv[:, 0], np.where(nv[:, 1] != 0, nv[:, 1], nv[:, 2]))
    flip = (dot > 0) | ((dot == 0) & (first < 0))
    nv = np.where(flip[:, None], -nv, nv)
    ok = k >= 3
    nv = np.where(ok[:, None], nv, 0.0)
    lam = w[:, ::-1]
    gap = lam[:, 1] - lam[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = np.where(ok & (gap > 0), 256.0 * k * U64 * lam[:, 0] / gap, np.inf)
    return Normals(nv, k, lam, beta)


# ---- point-to-plane ICP

def jacobian(p, q, n):
    """rows J = (p x n, n) and residuals r = (p - q) . n"""
    return np.concatenate([np.cross(p, n), n], 1), ((p - q) * n).sum(1)


def ldl_pivots(A):
    """LDL^T without pivoting -> (d [6], L)"""
    A = np.array(A, np.float64)
    m = len(A)
    L, d = np.eye(m), np.zeros(m)
    for k in range(m):
        d[k] = A[k, k] - (L[k, :k] ** 2 * d[:k]).sum()
        for i in range(k + 1, m):
            with np.errstate(divide="ignore", invalid="ignore"):
                L[i, k] = (A[i, k] - (L[i, :k] * L[k, :k] * d[:k]).sum()) / d[k]
    return d, L


def singular(A):
    """the contract's rule: a pivot d_k <= 2^-30 A_kk (a NaN pivot counts; pivots after the first failing one mean nothing)"""
    d, _ = ldl_pivots(A)
    for k in range(len(d)):
        if not d[k] > 2.0 ** -30 * A[k, k]:
            return True
    return False


def step_ldl(J, r):
    """the normal equations solved as the kernel does: xi with (J^T J) xi = -J^T r"""
    A, g = J.T @ J, J.T @ r
    d, L = ldl_pivots(A)
    y = np.linalg.solve(L, -g)
    return np.linalg.solve(L.T, y / d)


def step_lstsq(J, r):
    return np.linalg.lstsq(J, -r, rcond=None)[0]


def motion(xi):
    """U = [Rz(gamma) Ry(beta) Rx(alpha) | t]"""
    a, b, g = xi[:3]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    U = np.eye(4)
    U[:3, :3] = Rz @ Ry @ Rx
    U[:3, 3] = xi[3:]
    return U


def icp_plane(src, tgt, tgt_normals, r, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """-> (icp_restatement.Run, closest): ``closest`` is the smallest distance, over the run's convergence tests, of |d fitness| to
    ``relative_fitness`` or of |d rmse| to ``relative_rmse`` (+inf when no test was made) - how far the iteration count is from
    depending on rounding."""
    T = np.eye(4) if init is None else np.array(init, np.float64)
    if not np.isfinite(T).all():
        return R.Run(T, 0.0, 0.0, 0, 0, BAD_INIT, [T]), np.inf
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    nrm = np.asarray(tgt_normals, np.float32).reshape(-1, 3)
    if len(src) == 0 or len(tgt) == 0:
        return R.Run(T, 0.0, 0.0, 0, 0, FEW, [T]), np.inf
    if not (np.isfinite(src).all() and np.isfinite(tgt).all() and np.isfinite(nrm).all()) or R._outside(np.floor(tgt.astype(np.float64) / r)):
        return R.Run(T, 0.0, 0.0, 0, 0, RANGE, [T]), np.inf
    tgt64, nrm64 = tgt.astype(np.float64), nrm.astype(np.float64)
    tree = cKDTree(tgt64)
    traj = [T.copy()]
    res = R.evaluate(src, tgt, T, r, tree)
    status, e, closest = 0, 0, np.inf
    while True:
        hit = res.corr >= 0
        if int(hit.sum()) < 3:
            status |= FEW
        if status or e >= max_iteration:
            break
        J, rr = jacobian(res.p[hit], tgt64[res.corr[hit]], nrm64[res.corr[hit]])
        if singular(J.T @ J):
            status |= SINGULAR
            break
        T = motion(step_lstsq(J, rr)) @ T
        traj.append(T.copy())
        prev, res = res, R.evaluate(src, tgt, T, r, tree)
        e += 1
        df, dr = abs(prev.fitness - res.fitness), abs(prev.inlier_rmse - res.inlier_rmse)
        closest = min(closest, abs(df - relative_fitness), abs(dr - relative_rmse))
        if df < relative_fitness and dr < relative_rmse:
            status |= CONVERGED
    return R.Run(T, res.fitness, res.inlier_rmse, int((res.corr >= 0).sum()), e, status, traj, res), closest
