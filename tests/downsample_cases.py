"""Inputs shared by the down-sampling tests (tests/test_downsample_restatement_host.py, tests/test_gpu_downsample*.py)."""
import numpy as np

HUGE_VOXEL = 1.0e7          # every point of order_sensitive() in one voxel
RUN_LENGTHS = (1, 63, 64, 65, 257)


def order_sensitive(n, seed=0):
    """``n`` points (and 3 attribute columns) in ONE voxel at ``HUGE_VOXEL`` whose fp64 sum depends on the order: magnitudes of 1e5 and
    1e-3 mixed, both in +/- pairs, shuffled.  The exact sum is (close to) zero, so what comes out is the rounding of the partial sums:
    a small value added to a partial sum near 1e5 loses its bits below 2^-36, and which ones it loses depends on what came before."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    cols = []
    for _ in range(6):
        half = n // 2
        big = rng.uniform(0.1, 1.0, (half + 1) // 2) * 1.0e5
        small = rng.uniform(0.0, 1.0, half - len(big)) * 1.0e-3
        v = np.concatenate([big, -big, small, -small, rng.uniform(0.0, 1.0, n - 2 * half) * 1.0e-3])
        cols.append(rng.permutation(v))
    a = np.stack(cols, 1).astype(np.float32)
    return np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3:])


def random_clouds(seed, sizes, scale=2.0, offset=(0.0, 0.0, 0.0)):
    """Gaussian clouds of the given sizes (several points per voxel at a voxel of ~0.5), packed, with their segments."""
    rng = np.random.default_rng(seed)
    parts = [(rng.normal(size=(n, 3)) * scale + np.asarray(offset)).astype(np.float32) for n in sizes]
    seg = [0] + [int(v) for v in np.cumsum(sizes)]
    return (np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)), seg


def structured_scene(seed, n, T=None):
    """About ``n`` raw points of a scene FPFH can describe: a floor, two walls and a box, with range noise; ``T``: a pose applied to it."""
    rng = np.random.default_rng(seed)
    k = n // 6
    u = lambda m, lo, hi: rng.uniform(lo, hi, m)
    floor = np.stack([u(2 * k, -3, 3), u(2 * k, -3, 3), np.zeros(2 * k)], 1)
    wall_x = np.stack([np.full(k, 3.0), u(k, -3, 3), u(k, 0, 2)], 1)
    wall_y = np.stack([u(k, -3, 1.5), np.full(k, -3.0), u(k, 0, 1.6)], 1)
    top = np.stack([u(k, 0.5, 1.5), u(k, 0, 1.2), np.full(k, 0.9)], 1)
    side = np.stack([np.full(n - 5 * k, 0.5), u(n - 5 * k, 0, 1.2), u(n - 5 * k, 0, 0.9)], 1)
    p = np.concatenate([floor, wall_x, wall_y, top, side]) + rng.normal(size=(n, 3)) * 0.01
    p = p[rng.permutation(n)]
    if T is not None:
        p = p @ np.asarray(T)[:3, :3].T + np.asarray(T)[:3, 3]
    return p.astype(np.float32)


def small_pose(seed, angle=0.15, shift=0.4):
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= angle / np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = np.linalg.norm(w)
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.normal(size=3) * shift
    return T
