"""Where the down-sampling is switched in: the Open3D shim, the overlap ratio and the FPFH registration.  Each is a wiring identity
against tests/downsample_restatement.py or against the same call on clouds down-sampled beforehand; with the switch off the functions
return what a direct call returns."""
import numpy as np
import pytest
import torch

import downsample_cases as DC
import downsample_restatement as DR

pytestmark = pytest.mark.gpu

VOXEL = 0.3


def _down(cloud, voxel=VOXEL):
    return DR.restate_cloud(cloud, voxel)["xyz"]


def test_shim_voxel_down_sample():
    import eyoc_amd.o3d as o3d
    pts, _ = DC.random_clouds(90, [1500], 1.0)
    pcd = o3d.geometry.PointCloud()
    pcd.points = o3d.utility.Vector3dVector(pts)
    out = pcd.voxel_down_sample(VOXEL)
    assert isinstance(out, o3d.geometry.PointCloud) and out is not pcd and not out.has_normals()
    assert out.points.dtype == np.float64 and np.array_equal(out.points, _down(pts).astype(np.float64))
    assert np.array_equal(pcd.points, pts.astype(np.float64))              # the source is left alone

    rng = np.random.default_rng(91)
    nrm = rng.normal(size=(1500, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts2 = pts.copy()
    pts2[:2] = [[40.0, 40.0, 40.0], [40.0, 40.0, 40.0]]                     # a voxel of two points with opposite normals: zero mean
    nrm[1] = -nrm[0].astype(np.float32)
    nrm[0] = nrm[0].astype(np.float32)
    pcd2 = o3d.geometry.PointCloud()
    pcd2.points, pcd2.normals = o3d.utility.Vector3dVector(pts2), o3d.utility.Vector3dVector(nrm)
    out2 = pcd2.voxel_down_sample(VOXEL)
    want = DR.restate_cloud(pts2, VOXEL, nrm.astype(np.float32))
    assert np.array_equal(out2.points, want["xyz"].astype(np.float64)) and out2.has_normals()
    length = np.linalg.norm(out2.normals, axis=1)
    assert length[0] == 0.0 and want["count"][0] == 2
    assert np.all((length == 0.0) | (np.abs(length - 1.0) < 1e-12))
    mean = want["attrs"].astype(np.float64)
    keep = length > 0
    assert np.array_equal(out2.normals[keep], mean[keep] / np.sqrt((mean[keep] ** 2).sum(1, keepdims=True)))


def _pair(seed, n):
    T = DC.small_pose(seed)
    a = DC.structured_scene(seed, n)
    b = DC.structured_scene(seed + 1, n, T)
    return a, b, T


def test_compute_overlap_ratio_downsample():
    import eyoc_amd
    a, b, T = _pair(100, 3000)
    got = eyoc_amd.compute_overlap_ratio(a, b, T, VOXEL, downsample=True)
    want = eyoc_amd.compute_overlap_ratio(_down(a), _down(b), T, VOXEL)
    assert got == want and 0.0 < got <= 1.0
    raw = eyoc_amd.compute_overlap_ratio(a, b, T, VOXEL)
    assert eyoc_amd.compute_overlap_ratio(a, b, T, VOXEL, downsample=False) == raw
    assert float(eyoc_amd.overlap_ratio_batched([a], [b], T[None], VOXEL)[0].item()) == raw


def test_overlap_ratio_batched_downsample():
    import eyoc_amd
    pairs = [_pair(110 + 2 * i, n) for i, n in enumerate((2500, 3000, 1800))]
    A, Bc, T = [p[0] for p in pairs], [p[1] for p in pairs], np.stack([p[2] for p in pairs])
    got = eyoc_amd.overlap_ratio_batched(A, Bc, T, VOXEL, downsample=True)
    want = eyoc_amd.overlap_ratio_batched([_down(a) for a in A], [_down(b) for b in Bc], T, VOXEL)
    assert got.dtype == torch.float64 and got.shape == (3,) and torch.equal(got, want)
    packed_a, packed_b = torch.from_numpy(np.concatenate(A)).cuda(), torch.from_numpy(np.concatenate(Bc)).cuda()
    seg_a, seg_b = [0] + list(np.cumsum([len(a) for a in A])), [0] + list(np.cumsum([len(b) for b in Bc]))
    packed = eyoc_amd.overlap_ratio_batched(packed_a, packed_b, T, VOXEL, seg0=seg_a, seg1=seg_b, downsample=True)
    assert torch.equal(packed, want)
    assert torch.equal(eyoc_amd.overlap_ratio_batched(A, Bc, T, VOXEL, downsample=False), eyoc_amd.overlap_ratio_batched(A, Bc, T, VOXEL))


@pytest.mark.parametrize("backend", ["ransac", "sc2pcr"])
def test_register_fpfh_batched_downsample(backend):
    """A wiring identity: raw scans with ``downsample=True`` give the bytes of the same call on clouds down-sampled beforehand by
    ``voxel_down_sample_batched``.  No recall figure is asserted."""
    import eyoc_amd
    pairs = [_pair(120 + 2 * i, n) for i, n in enumerate((3000, 2900))]
    src, tgt = np.concatenate([p[1] for p in pairs]), np.concatenate([p[0] for p in pairs])
    seg_s, seg_t = [0, 3000, 5900], [0, 3000, 5900]
    kw = dict(voxel_size=VOXEL, distance_threshold=0.45, backend=backend, max_iteration=50000, seed=3)
    got = eyoc_amd.register_fpfh_batched(src, tgt, seg_s, seg_t, downsample=True, **kw)
    ds, seg_ds, st_s = eyoc_amd.voxel_down_sample_batched(src, seg_s, VOXEL)
    dt, seg_dt, st_t = eyoc_amd.voxel_down_sample_batched(tgt, seg_t, VOXEL)
    assert st_s.tolist() == [0, 0] and st_t.tolist() == [0, 0] and 200 < seg_ds[-1] < 5900 // 2
    want = eyoc_amd.register_fpfh_batched(ds, dt, seg_ds, seg_dt, **kw)
    off = eyoc_amd.register_fpfh_batched(ds, dt, seg_ds, seg_dt, downsample=False, **kw)
    assert len(got) == len(want) == 2
    for g, w, o in zip(got, want, off):
        for other in (w, o):
            assert g.transformation.tobytes() == other.transformation.tobytes()
            assert (g.fitness, g.inlier_rmse, g.inliers, g.status) == (other.fitness, other.inlier_rmse, other.inliers, other.status)
        assert g.status == 0


def test_register_fpfh_batched_downsample_refuses_a_bad_scan_alone():
    import eyoc_amd
    from eyoc_amd import icp
    pairs = [_pair(130 + 2 * i, 2000) for i in range(2)]
    src, tgt = np.concatenate([p[1] for p in pairs]), np.concatenate([p[0] for p in pairs])
    src[2500, 0] = np.nan
    kw = dict(voxel_size=VOXEL, distance_threshold=0.45, max_iteration=20000, seed=3)
    out = eyoc_amd.register_fpfh_batched(src, tgt, [0, 2000, 4000], [0, 2000, 4000], downsample=True, **kw)
    alone = eyoc_amd.register_fpfh_batched(src[:2000], tgt[:2000], [0, 2000], [0, 2000], downsample=True, **kw)
    assert out[1].status == icp.RANGE and np.array_equal(out[1].transformation, np.eye(4))
    assert out[0].status == 0 and out[0].transformation.tobytes() == alone[0].transformation.tobytes()
