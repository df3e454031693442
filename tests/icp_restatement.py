"""CPU restatement of the point-to-point ICP contract (include/eyoc_hip.h, "ICP refinement"), numpy fp64.  Imports nothing from
``eyoc_amd``: it is what the GPU tests compare against.

``evaluate``: candidates come from ``scipy.spatial.cKDTree`` (the ``K`` nearest rows by the tree's own arithmetic), the decision is
made by the contract's expression on those candidates - d2 = (px-qx)^2 + (py-qy)^2 + (pz-qz)^2 summed left to right in fp64, the
smallest d2 wins, the lowest row on an exact tie, a correspondence iff d2 < r^2.  ``evaluate_brute`` is the same decision over ALL
N x M candidates (tests/test_icp_host.py compares the two bit for bit).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
from scipy.spatial import cKDTree

CONVERGED, BAD_INIT, FEW, RANGE = 1, 2, 4, 8
K = 4      # candidates per row: the true minimum is among the tree's 4 nearest unless 4 rows sit within rounding of one another


@dataclass
class Eval:
    corr: np.ndarray        # int64 [n]: target row or -1
    d2: np.ndarray          # f64 [n]: d2 of the correspondence, +inf where corr == -1
    fitness: float
    inlier_rmse: float
    margin: np.ndarray      # f64 [n]: min(runner-up d2 - best d2, |best d2 - r^2|): how far the row's decision is from flipping
    p: np.ndarray           # f64 [n, 3]: the posed points


@dataclass
class Run:
    T: np.ndarray
    fitness: float
    inlier_rmse: float
    correspondences: int
    iterations: int
    status: int
    trajectory: list = field(default_factory=list)     # T_0 (= init) ... T_iterations
    last: Eval | None = None


def pose(src, T):
    x = np.asarray(src, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    return np.stack([((T[k, 0] * x[:, 0] + T[k, 1] * x[:, 1]) + T[k, 2] * x[:, 2]) + T[k, 3] for k in range(3)], 1)


def _d2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _decide(p, cand_d2, cand_row, r, n_src):
    """``cand_d2 [n, k]`` (+inf = no candidate), ``cand_row [n, k]`` -> Eval by the contract's order."""
    big = np.iinfo(np.int64).max
    row = np.where(np.isfinite(cand_d2), cand_row, big)
    order = np.lexsort((row, cand_d2), axis=1) if cand_d2.shape[1] > 1 else np.zeros_like(row)
    ar = np.arange(len(p))
    best, best_row = cand_d2[ar, order[:, 0]], row[ar, order[:, 0]]
    second = cand_d2[ar, order[:, 1]] if cand_d2.shape[1] > 1 else np.full(len(p), np.inf)
    r2 = r * r
    hit = best < r2
    n = int(hit.sum())
    with np.errstate(invalid="ignore"):
        margin = np.minimum(np.where(np.isfinite(second), second - best, np.inf), np.abs(best - r2))
    return Eval(np.where(hit, best_row, -1).astype(np.int64), np.where(hit, best, np.inf), n / n_src if n_src else 0.0,
                float(np.sqrt(best[hit].sum() / n)) if n else 0.0, margin, p)


def evaluate(src, tgt, T, r, tree=None):
    tgt64 = np.asarray(tgt, np.float32).astype(np.float64)
    p = pose(src, T)
    if len(p) == 0 or len(tgt64) == 0:
        return Eval(np.full(len(p), -1, np.int64), np.full(len(p), np.inf), 0.0, 0.0, np.full(len(p), np.inf), p)
    tree = cKDTree(tgt64) if tree is None else tree
    k = min(K, len(tgt64))
    _, j = tree.query(p, k=k, workers=-1)
    j = j.reshape(len(p), k)
    return _decide(p, _d2(p[:, None, :], tgt64[j]), j.astype(np.int64), r, len(p))


def evaluate_brute(src, tgt, T, r, block=256):
    tgt64 = np.asarray(tgt, np.float32).astype(np.float64)
    p = pose(src, T)
    d2s, rows = [], []
    for a in range(0, len(p), block):
        d = _d2(p[a:a + block, None, :], tgt64[None])
        o = np.lexsort((np.broadcast_to(np.arange(len(tgt64)), d.shape), d), axis=1)[:, :2]
        d2s.append(np.take_along_axis(d, o, 1))
        rows.append(o)
    return _decide(p, np.concatenate(d2s), np.concatenate(rows).astype(np.int64), r, len(p))


def kabsch(p, q):
    """Umeyama without scaling: the rigid U with U p ~ q (fp64 means, 3 x 3 covariance, reflection fix)."""
    mp, mq = p.mean(0), q.mean(0)
    H = (q - mq).T @ (p - mp)
    U, _, Vt = np.linalg.svd(H)
    D = np.eye(3)
    D[2, 2] = np.sign(np.linalg.det(U) * np.linalg.det(Vt)) or 1.0
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mq - R @ mp
    return T


def _outside(cells):
    return bool(((cells < -2 ** 17) | (cells >= 2 ** 17)).any())


def icp(src, tgt, r, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6) -> Run:
    T = np.eye(4) if init is None else np.array(init, np.float64)
    if not np.isfinite(T).all():
        return Run(T, 0.0, 0.0, 0, 0, BAD_INIT, [T])
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    if len(src) == 0 or len(tgt) == 0:
        return Run(T, 0.0, 0.0, 0, 0, FEW, [T])
    if not (np.isfinite(src).all() and np.isfinite(tgt).all()) or _outside(np.floor(tgt.astype(np.float64) / r)):
        return Run(T, 0.0, 0.0, 0, 0, RANGE, [T])
    tgt64 = tgt.astype(np.float64)
    tree = cKDTree(tgt64)
    traj = [T.copy()]
    res = evaluate(src, tgt, T, r, tree)
    status, e = 0, 0
    while True:
        n = int((res.corr >= 0).sum())
        if n < 3:
            status |= FEW
        if status or e >= max_iteration:
            break
        hit = res.corr >= 0
        T = kabsch(res.p[hit], tgt64[res.corr[hit]]) @ T
        traj.append(T.copy())
        prev, res = res, evaluate(src, tgt, T, r, tree)
        e += 1
        if abs(prev.fitness - res.fitness) < relative_fitness and abs(prev.inlier_rmse - res.inlier_rmse) < relative_rmse:
            status |= CONVERGED
    return Run(T, res.fitness, res.inlier_rmse, int((res.corr >= 0).sum()), e, status, traj, res)


def perturb(T, rng, rot_deg, trans):
    """A RANSAC-grade start: ``T`` turned by ``rot_deg`` about a random axis and shifted by ~``trans`` metres."""
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = np.deg2rad(rot_deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    D[:3, 3] = rng.normal(size=3) * trans / np.sqrt(3)
    return D @ np.asarray(T, np.float64)
