"""Inputs shared by tests/test_train_batch_host.py and tests/test_gpu_train_batch.py.  Not a test."""
import numpy as np

HAND_VOXEL = 0.25


def hand_faces():
    """Points whose quotient by 0.25 is exact, under the identity pose and no scale, with the answers written down by hand.
    -> ``(clouds [2] f32 [n,3], coords int32 [M,4], sel int64 [M], xyz f32 [M,3], offsets int64 [3])``; the kept points are
    ``clouds[b][sel]``, except that -0.0 comes out of the pose expression as +0.0 (``1 * -0.0 + 0 * y`` is +0.0 in IEEE arithmetic)."""
    ks = (-3, -1, 0, 1, 2, 7)
    pts, cells, kept = [], [], []

    def add(p, cell, keep=True):
        pts.append(p)
        if keep:
            cells.append(cell)
            kept.append(len(pts) - 1)
    for k in ks:                                      # x = k * 0.25 -> k
        add((np.float32(k * 0.25), 0.1, 0.1), (k, 0, 0))
    for k in ks:                                      # the fp32 number just below -> k - 1
        add((np.nextafter(np.float32(k * 0.25), np.float32(-np.inf)), 0.1, 0.3), (k - 1, 0, 1))
    add((-0.25, 0.6, 0.1), (-1, 2, 0))
    add((-1e-30, 0.85, 0.1), (-1, 3, 0))
    add((-0.0, 1.1, 0.1), (0, 4, 0))
    add((5.05, 5.05, 5.05), (20, 20, 20))             # two points in one voxel: the lower index is kept
    add((5.1, 5.2, 5.24), (20, 20, 20), keep=False)
    add((0.0, 0.1, 0.1), (0, 0, 0), keep=False)       # ... also far apart in the cloud (the voxel of k = 0 above)
    c0 = np.asarray(pts, np.float32)
    assert np.signbit(c0[14, 0]) and c0[13, 0] < 0    # -0.0 and -1e-30 survive the cast to fp32
    c1 = np.asarray([(5.2, 5.01, 5.1), (5.21, 5.01, 5.1)], np.float32)   # the same voxel in another cloud: kept, batch index 1
    coords = np.asarray([(0,) + c for c in cells] + [(1, 20, 20, 20)], np.int32)
    sel = np.asarray(kept + [0], np.int64)
    xyz = np.concatenate([c0[kept], c1[:1]]) + np.float32(0.0)          # (-0.0 + 0.0 = +0.0, every other value unchanged)
    assert not np.signbit(xyz[14, 0]) and np.array_equal(xyz, np.concatenate([c0[kept], c1[:1]]))
    return [c0, c1], coords, sel, xyz, np.asarray([0, len(kept), len(kept) + 1], np.int64)


GENERAL_SIZES = (0, 1, 255, 256, 257, 1025)


def general_clouds(seed=5):
    """Six clouds whose points crowd into a 1.2 m cube some tens of metres from the origin: at 0.3 m many share a voxel."""
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-0.6, 0.6, size=(n, 3)) + rng.uniform(-40.0, 40.0, size=3)).astype(np.float32) for n in GENERAL_SIZES]


def rigid(rng, shift):
    """A random rigid pose with a translation of up to ``shift`` metres per axis."""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.uniform(-shift, shift, 3)
    return T
