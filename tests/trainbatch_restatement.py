"""fp64 restatement of the training-batch augmentation (``include/eyoc_hip.h``: eyoc_augment_poses, eyoc_voxelize_batched_posed) and of
``draw_augmentation``'s rotation.  Not a test.  Every expression is written element by element with its brackets, on scalars or on whole
columns, so that numpy neither fuses nor re-associates anything: the device's results are compared with these byte for byte."""
import numpy as np

LIM = (1 << 17) - 16          # the key range of the coordinate maps: -LIM <= c < LIM


def rodrigues(axis, theta):
    """R = I + sin(theta) K + (1 - cos(theta)) K^2 for the unit axis, written out."""
    a = np.asarray(axis, np.float64)
    n = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    x, y, z = a[0] / n, a[1] / n, a[2] / n
    c, s = np.cos(np.float64(theta)), np.sin(np.float64(theta))
    t = 1.0 - c
    return np.array([[c + x * x * t, x * y * t - z * s, x * z * t + y * s],
                     [y * x * t + z * s, c + y * y * t, y * z * t - x * s],
                     [z * x * t - y * s, z * y * t + x * s, c + z * z * t]], np.float64)


def cloud_pose(R, mean):
    """T = [R | R (-mean)]: t_k = (R[k][0] (-m_0) + R[k][1] (-m_1)) + R[k][2] (-m_2)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    m = [-np.float64(v) for v in np.asarray(mean, np.float64)[:3]]
    T = np.eye(4)
    for k in range(3):
        T[k, :3] = R[k]
        T[k, 3] = (R[k, 0] * m[0] + R[k, 1] * m[1]) + R[k, 2] * m[2]
    return T


def compose(T0, T1, M2, scale=None):
    """(T_1 M2) inv(T_0) with the rigid inverse, in the header's order; ``scale``: the translation times it (``None``: no product)."""
    T0, T1, M = (np.asarray(a, np.float64).reshape(4, 4) for a in (T0, T1, M2))
    A = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            A[i, j] = (T1[i, 0] * M[0, j] + T1[i, 1] * M[1, j]) + T1[i, 2] * M[2, j]
        A[i, 3] = ((T1[i, 0] * M[0, 3] + T1[i, 1] * M[1, 3]) + T1[i, 2] * M[2, 3]) + T1[i, 3]
    u = [-((T0[0, k] * T0[0, 3] + T0[1, k] * T0[1, 3]) + T0[2, k] * T0[2, 3]) for k in range(3)]
    G = np.eye(4)
    for i in range(3):
        for j in range(3):
            G[i, j] = (A[i, 0] * T0[j, 0] + A[i, 1] * T0[j, 1]) + A[i, 2] * T0[j, 2]
        G[i, 3] = ((A[i, 0] * u[0] + A[i, 1] * u[1]) + A[i, 2] * u[2]) + A[i, 3]
        if scale is not None:
            G[i, 3] = np.float64(scale) * G[i, 3]
    return G


def pose_points(xyz, T, scale=None):
    """p'_k = s (((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3]) for fp32 points -> f64 ``[n,3]``."""
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty((len(p), 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            q = ((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3]
            out[:, k] = q if scale is None else np.float64(scale) * q
    return out


class RangeFault(Exception):
    def __init__(self, cloud):
        super().__init__(f"cloud {cloud}")
        self.cloud = cloud


def quantize_posed(clouds, poses, scales, voxel, batch_base=0, isolate=False):
    """The posed voxeliser: per cloud the first point of every voxel ``floor(p' / voxel)``, ``sel`` ascending, ``float32(p')``.
    -> ``(coords int32 [M,4], sel int64 [M], xyz f32 [M,3], offsets int64 [B+1], faults int32 [B,2])``.  A faulty point (a non-finite
    p', or a finite one with a cell outside the key range) empties its cloud with ``isolate``, else raises ``RangeFault(first cloud)``."""
    C, S, X, off = [], [], [], [0]
    faults = np.zeros((len(clouds), 2), np.int32)
    for b, cloud in enumerate(clouds):
        p = pose_points(cloud, poses[b], None if scales is None else scales[b])
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.floor(p / np.float64(voxel))
            x32 = p.astype(np.float32)
        finite = np.isfinite(p).all(1)
        out = finite & ~((f >= -LIM) & (f < LIM)).all(1)
        faults[b] = int(out.sum()), int((~finite).sum())
        if faults[b].any():
            if not isolate:
                raise RangeFault(b)
            off.append(off[-1])
            continue
        cells = f.astype(np.int64)
        _, first = np.unique(cells, axis=0, return_index=True) if len(cells) else (None, np.zeros(0, np.int64))
        sel = np.sort(first).astype(np.int64)
        C.append(np.concatenate([np.full((len(sel), 1), batch_base + b, np.int64), cells[sel]], 1).astype(np.int32))
        S.append(sel)
        X.append(x32[sel])
        off.append(off[-1] + len(sel))
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)   # noqa: E731
    return cat(C, (0, 4), np.int32), cat(S, (0,), np.int64), cat(X, (0, 3), np.float32), np.asarray(off, np.int64), faults


# ---- G13 (tests/golden/make_golden_trainbatch.py): the inputs are regenerated from the case table
G13_SIZES = (1, 7, 100, 1000, 5000)
G13_RANGES = (360.0, float(np.pi / 4))


def g13_cases():
    """``[(seed, n, rotation_range)]``."""
    return [(100 + 10 * i + j, n, rr) for i, n in enumerate(G13_SIZES) for j, rr in enumerate(G13_RANGES)]


def g13_cloud(seed, n, which):
    """Cloud ``which`` (0 / 1) of a case: fp32, |x| <= 80 m, off-centre."""
    rng = np.random.default_rng([seed, which])
    return (rng.uniform(-60.0, 60.0, size=(n, 3)) + rng.uniform(-20.0, 20.0, size=3)).astype(np.float32)
