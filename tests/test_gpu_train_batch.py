"""Training batches from raw scans on the GPU (``eyoc_cloud_centroids``, ``eyoc_augment_poses``, ``eyoc_voxelize_batched_posed``,
``eyoc_amd.trainbatch``) against the fp64 restatement (tests/trainbatch_restatement.py).  Every stage is fed the device's own output of
the stage before it, so the comparisons with the restatement are byte comparisons; the centroid, whose summation order is the kernel's
business, is held to the error bound of ANY summation order against the exact mean instead, and to byte-equal repeatability."""
import math

import numpy as np
import pytest
import torch

import trainbatch_cases as cases
import trainbatch_restatement as R

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _pack(clouds, stride=3):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    host = np.zeros((off[-1], stride), np.float32)
    host[:, :3] = np.concatenate(clouds) if off[-1] else 0
    if stride == 4:
        host[:, 3] = 0.5                     # (the reflectance column: never read)
    return _dev(host), off


def _centroids(clouds, stride=3):
    from eyoc_amd import trainbatch as tb
    packed, off = _pack(clouds, stride)
    return tb.cloud_centroids(packed, off).cpu().numpy()


# ---- 1. centroids
CENTROID_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025, 0)
TILE_SIZES = (4095, 4096, 4097, 8193, 0, 3)      # around the 4096 points one workgroup sums: one, two and three partial sums per cloud


@pytest.mark.parametrize("sizes", [CENTROID_SIZES, TILE_SIZES], ids=["wave_and_workgroup_edges", "tile_edges"])
@pytest.mark.parametrize("stride", [3, 4])
def test_centroids(sizes, stride):
    rng = np.random.default_rng(len(sizes))
    clouds = [(rng.uniform(-60.0, 60.0, size=(n, 3)) + rng.uniform(-20.0, 20.0, size=3)).astype(np.float32) for n in sizes]
    got = _centroids(clouds, stride)
    assert got.shape == (len(sizes), 4) and got.dtype == np.float64
    for b, c in enumerate(clouds):
        n = len(c)
        assert got[b, 3] == n
        if n == 0:
            assert got[b].tobytes() == bytes(32)
            continue
        bound = 2 * n * 2.0 ** -53 * float(np.abs(c).max())
        for k in range(3):
            exact = math.fsum(float(v) for v in c[:, k]) / n
            assert abs(got[b, k] - exact) <= bound, (b, k, got[b, k] - exact, bound)
    # a cloud's 32 bytes: in a second run, at another position, alone
    assert _centroids(clouds, stride).tobytes() == got.tobytes()
    assert _centroids(clouds[::-1], stride)[::-1].tobytes() == got.tobytes()
    for b, c in enumerate(clouds):
        assert _centroids([c], stride).tobytes() == got[b].tobytes(), b


# ---- 2. poses
@pytest.fixture(scope="module")
def general():
    """The six clouds, their centroids and poses as the device computed them (three pairs, scales given), shared and never modified."""
    from eyoc_amd import trainbatch as tb
    clouds = cases.general_clouds()
    packed, off = _pack(clouds)
    cen = tb.cloud_centroids(packed, off)
    rot, _ = tb.draw_augmentation(np.random.RandomState(4), 3)
    rng = np.random.default_rng(8)
    M2 = np.stack([cases.rigid(rng, 300.0) for _ in range(3)])
    scale = rng.uniform(0.8, 1.2, 3)
    pose, T_gt = tb.augment_poses(_dev(rot), cen, _dev(scale), _dev(M2))
    return dict(clouds=clouds, packed=packed, off=off, cen=cen, rot=rot, M2=M2, scale=scale, pose=pose, pose_host=pose.cpu().numpy(),
                T_gt=T_gt.cpu().numpy(), cloud_scale=np.repeat(scale, 2))


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("scaled", [False, True])
def test_poses(general, P, scaled):
    from eyoc_amd import trainbatch as tb
    g = general
    cen = g["cen"].cpu().numpy()
    scale = g["scale"][:P] if scaled else None
    pose, T_gt = tb.augment_poses(_dev(g["rot"][:2 * P]), g["cen"][:2 * P].contiguous(), None if scale is None else _dev(scale), _dev(g["M2"][:P]))
    pose, T_gt = pose.cpu().numpy(), T_gt.cpu().numpy()
    for b in range(P):
        T0, T1 = (R.cloud_pose(g["rot"][2 * b + i], cen[2 * b + i]) for i in (0, 1))
        assert pose[2 * b].tobytes() == T0.tobytes() and pose[2 * b + 1].tobytes() == T1.tobytes(), b
        s = None if scale is None else scale[b]
        assert T_gt[b].tobytes() == R.compose(T0, T1, g["M2"][b], s).tobytes(), b
        want = T1 @ g["M2"][b] @ np.linalg.inv(T0)
        if s is not None:
            want[:3, 3] = s * want[:3, 3]
        np.testing.assert_allclose(T_gt[b], want, rtol=1e-12, atol=1e-10)
    assert np.isfinite(pose[0]).all() and pose[1, :3, 3].tolist() == R.cloud_pose(g["rot"][1], cen[1])[:3, 3].tolist()


# ---- 3. the posed voxeliser on faces known by hand
def _voxelize(clouds, pose, scale, voxel, base=0, isolate=False, packed=None):
    from eyoc_amd import trainbatch as tb
    packed, off = _pack(clouds) if packed is None else packed
    pose = pose if isinstance(pose, torch.Tensor) else _dev(np.stack(pose), np.float64)
    out = tb.voxelize_posed(packed, off, pose, None if scale is None else _dev(scale, np.float64), voxel, base, isolate)
    return [o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out]


def _same(got, want, what=""):
    assert got[0].dtype == np.int32 and got[0].tobytes() == want[0].tobytes(), f"{what}: coords"
    assert got[1].dtype == np.int64 and got[1].tobytes() == want[1].tobytes(), f"{what}: sel"
    assert got[2].dtype == np.float32 and got[2].tobytes() == want[2].tobytes(), f"{what}: xyz"
    assert got[3].tolist() == want[3].tolist(), f"{what}: offsets"


def test_posed_voxeliser_hand_made_faces():
    clouds, coords, sel, xyz, offsets = cases.hand_faces()
    for stride in (3, 4):
        got = _voxelize(clouds, [np.eye(4)] * 2, None, cases.HAND_VOXEL, packed=_pack(clouds, stride))
        _same(got, (coords, sel, xyz, offsets), f"stride {stride}")
    got = _voxelize(clouds, [np.eye(4)] * 2, [1.0, 1.0], cases.HAND_VOXEL, base=7, isolate=True)
    _same(got, (coords + np.asarray([7, 0, 0, 0], np.int32), sel, xyz, offsets), "scale 1, base 7")
    assert not got[4].any()


# ---- 4. the posed voxeliser on clouds that share voxels, under the device's own poses
@pytest.mark.parametrize("base", [0, 1018])
@pytest.mark.parametrize("scaled", [False, True])
def test_posed_voxeliser_general(general, base, scaled):
    g = general
    scale = g["cloud_scale"] if scaled else None
    want = R.quantize_posed(g["clouds"], g["pose_host"], scale, 0.3, base)
    sizes = np.diff(want[3])
    assert sizes[0] == 0 and sizes[1] == 1 and (sizes[2:] < np.asarray(cases.GENERAL_SIZES[2:]) * 0.8).all()   # many share a voxel
    got = _voxelize(g["clouds"], g["pose"], scale, 0.3, base, packed=(g["packed"], g["off"]))
    _same(got, want, "batch of 6")
    assert (got[0][:, 0] >= base).all() and (got[0][:, 0] < base + 6).all()
    for b, c in enumerate(g["clouds"]):               # B = 1: every cloud alone, at its batch index
        if len(c):
            alone = _voxelize([c], g["pose"][b:b + 1].contiguous(), None if scale is None else scale[b:b + 1], 0.3, base + b)
            lo, hi = want[3][b], want[3][b + 1]
            _same(alone, (want[0][lo:hi], want[1][lo:hi], want[2][lo:hi], np.asarray([0, hi - lo])), f"cloud {b} alone")


# ---- 5. faults are counted outcomes
def test_posed_voxeliser_faults(general):
    from eyoc_amd import _lib
    g = general
    bad = [c.copy() for c in g["clouds"]]
    bad[2][17, 1] = np.nan
    bad[4][200] = (1e6, 0.0, 0.0)                     # posed a million metres out: far beyond 2^17 cells of 0.3 m
    clean = R.quantize_posed(g["clouds"], g["pose_host"], None, 0.3, 3)
    want = R.quantize_posed(bad, g["pose_host"], None, 0.3, 3, isolate=True)
    got = _voxelize(bad, g["pose"], None, 0.3, 3, isolate=True)
    _same(got, want, "isolating")
    assert got[4].tolist() == [[0, 0], [0, 0], [0, 1], [0, 0], [1, 0], [0, 0]] and got[4].dtype == np.int32
    off, off_clean = got[3], clean[3]
    assert off[3] == off[2] and off[5] == off[4]
    for b in (1, 3, 5):                               # every other cloud's rows: those of the clean batch
        for k in range(3):
            assert got[k][off[b]:off[b + 1]].tobytes() == clean[k][off_clean[b]:off_clean[b + 1]].tobytes(), (b, k)
    with pytest.raises(_lib.EyocError) as e:
        _voxelize(bad, g["pose"], None, 0.3, 3)
    assert e.value.code == _lib.ERR_RANGE and "cloud 2" in str(e.value)
    bad[2][17, 1] = 0.0                               # the NaN gone: the first faulty cloud is the far one
    with pytest.raises(_lib.EyocError) as e:
        _voxelize(bad, g["pose"], None, 0.3, 3)
    assert e.value.code == _lib.ERR_RANGE and "cloud 4" in str(e.value)
    _same(_voxelize(g["clouds"], g["pose"], None, 0.3, 3), clean, "the clean batch after the failed calls")


# ---- 6. TrainBatch.from_scans, end to end
VOXEL, SEARCH = 0.3, 1.5 * 0.3


@pytest.fixture(scope="module")
def scans():
    """3 pairs of ~2000-point sweeps with their planted relative pose; pair 2's target is shifted by 500 m: no overlap."""
    from eyoc_amd import synthetic as syn
    s0, s1, M2 = [], [], []
    for seed in (1, 2, 3):
        p = syn.make_pair(seed, dist_range=(1.0, 3.0), beams=8, azimuths=250, band=None, keep_raw=True)
        s0.append(p["raw0"])
        s1.append(p["raw1"])
        M2.append(np.asarray(p["T_gt"], np.float64))
    s1[2] = (s1[2] + np.asarray([500.0, 0.0, 0.0], np.float32)).astype(np.float32)
    assert all(1500 <= len(c) <= 2500 for c in s0 + s1)
    return s0, s1, np.stack(M2)


def _batch(scans, n=3, **kw):
    from eyoc_amd import TrainBatch
    s0, s1, M2 = scans
    kw.setdefault("randg", np.random.RandomState(12))
    kw.setdefault("search_voxel_size", SEARCH)
    return TrainBatch.from_scans(s0[:n], s1[:n], M2[:n], VOXEL, frame_distance=(10,) * n, **kw)


@pytest.fixture(scope="module")
def gt_batch(scans):
    return _batch(scans)


def test_from_scans_coordinates_and_poses(scans, gt_batch):
    s0, s1, M2 = scans
    tb = gt_batch
    clouds = [c for pair in zip(s0, s1) for c in pair]
    rot, scale = __import__("eyoc_amd").draw_augmentation(np.random.RandomState(12), 3)
    assert np.array_equal(rot, tb.R) and scale.tolist() == [1.0] * 3
    cen, pose = tb.centroids.cpu().numpy(), tb.pose.cpu().numpy()
    assert cen.tobytes() == _centroids(clouds).tobytes()
    T_gt64 = tb.T_gt64.cpu().numpy()
    for b in range(3):
        T0, T1 = (R.cloud_pose(rot[2 * b + i], cen[2 * b + i]) for i in (0, 1))
        assert pose[2 * b].tobytes() == T0.tobytes() and pose[2 * b + 1].tobytes() == T1.tobytes()
        assert T_gt64[b].tobytes() == R.compose(T0, T1, M2[b]).tobytes()
    assert tb.T_gt.dtype == torch.float32 and tb.T_gt.cpu().numpy().tobytes() == T_gt64.astype(np.float32).tobytes()
    coords, sel, xyz, off, _ = R.quantize_posed(clouds, pose, None, VOXEL)
    for i, (C, X, pcd, seg) in enumerate(((tb.sinput0_C, tb.xyz0, tb.pcd0, tb.seg0), (tb.sinput1_C, tb.xyz1, tb.pcd1, tb.seg1))):
        C, X = C.cpu().numpy(), X.cpu().numpy()
        assert C.dtype == np.int32 and seg[-1] == len(C) == len(X)
        for b in range(3):
            lo, hi = off[2 * b + i], off[2 * b + i + 1]
            want = coords[lo:hi].copy()
            want[:, 0] = b
            assert C[seg[b]:seg[b + 1]].tobytes() == want.tobytes(), (i, b)
            assert X[seg[b]:seg[b + 1]].tobytes() == xyz[lo:hi].tobytes(), (i, b)
            assert pcd[b].cpu().numpy().tobytes() == xyz[lo:hi].tobytes()
            assert tb.len_batch[b][i] == hi - lo
    assert tb.sinput0_F.shape == (len(tb.sinput0_C), 1) and bool((tb.sinput0_F == 1).all()) and bool((tb.sinput1_F == 1).all())
    # a voxel grid of a sweep: a third or more of the raw points go
    assert 300 < tb.len_batch[0][0] < 0.9 * len(s0[0])


def test_from_scans_correspondences_and_dict(scans, gt_batch):
    import eyoc_amd
    tb = gt_batch
    seg0, seg1 = [int(v) for v in tb.seg0], [int(v) for v in tb.seg1]
    corr, seg_m, _ = eyoc_amd.matching_indices_batched(tb.xyz0, tb.xyz1, tb.T_gt64, SEARCH, seg0=seg0, seg1=seg1)
    assert tb.correspondences.dtype == torch.int64 and torch.equal(tb.correspondences, corr) and torch.equal(tb.seg_m, seg_m)
    assert tb.valid.tolist() == [True, True, False]
    counts = torch.diff(tb.seg_m).tolist()
    assert counts[0] > 100 and counts[1] > 100 and counts[2] == 0
    d = tb.as_input_dict()
    assert sorted(d) == sorted(["pcd0", "pcd1", "sinput0_C", "sinput0_F", "sinput1_C", "sinput1_F", "correspondences", "T_gt", "len_batch",
                                "frame_distance"])
    assert len(d["T_gt"]) == 2 and len(d["len_batch"]) == 2 and d["len_batch"] == tb.len_batch[:2]
    assert torch.equal(d["T_gt"][1], tb.T_gt[1]) and d["T_gt"][0].dtype == torch.float32
    assert d["correspondences"].dtype == torch.int32 and len(d["pcd0"]) == 3 and d["frame_distance"] == (10, 10, 10)
    # the planted pose holds under the augmentation: most matched pairs are close under T_gt
    p = tb.xyz0[corr[:, 0]].double() @ tb.T_gt64[0][:3, :3].T + tb.T_gt64[0][:3, 3]
    first = corr[:, 0] < seg0[1]
    assert float((p - tb.xyz1[corr[:, 1]].double())[first].norm(dim=1).max()) < SEARCH


def test_from_scans_labels_and_repeatability(scans, gt_batch):
    import eyoc_amd
    tb = gt_batch
    again = _batch(scans)
    for name in ("sinput0_C", "sinput1_C", "xyz0", "xyz1", "correspondences", "seg_m", "T_gt64", "T_gt", "valid"):
        assert torch.equal(getattr(tb, name), getattr(again, name)), name
    ident = _batch(scans, labels="identity")
    assert torch.equal(ident.sinput0_C, tb.sinput0_C) and torch.equal(ident.T_gt64, tb.T_gt64)
    corr, seg_m, _ = eyoc_amd.matching_indices_batched(ident.xyz0, ident.xyz1, None, SEARCH, seg0=[int(v) for v in ident.seg0],
                                                       seg1=[int(v) for v in ident.seg1])
    assert torch.equal(ident.correspondences, corr) and torch.equal(ident.seg_m, seg_m) and not torch.equal(corr, tb.correspondences)
    none = _batch(scans, labels="none")
    assert none.correspondences.shape == (0, 2) and none.correspondences.dtype == torch.int64
    assert none.valid.tolist() == [True] * 3 and len(none.as_input_dict()["T_gt"]) == 3
    assert torch.equal(none.sinput1_C, tb.sinput1_C)


def test_from_scans_without_rotation_is_the_plain_voxeliser(scans):
    import eyoc_amd
    s0, s1, M2 = scans
    tb = _batch(scans, random_rotation=False, randg=None)
    coords, _, xyz, off = eyoc_amd.sparse_quantize_batch([c for pair in zip(s0, s1) for c in pair], VOXEL)
    coords, xyz = coords.cpu().numpy(), xyz.cpu().numpy()
    for i, (C, X, seg) in enumerate(((tb.sinput0_C, tb.xyz0, tb.seg0), (tb.sinput1_C, tb.xyz1, tb.seg1))):
        C, X = C.cpu().numpy(), X.cpu().numpy()
        for b in range(3):
            lo, hi = off[2 * b + i], off[2 * b + i + 1]
            want = coords[lo:hi].copy()
            want[:, 0] = b
            assert C[seg[b]:seg[b + 1]].tobytes() == want.tobytes() and X[seg[b]:seg[b + 1]].tobytes() == xyz[lo:hi].tobytes()
    assert tb.T_gt64.cpu().numpy().tobytes() == M2.tobytes() and tb.pose is None
    assert tb.valid.tolist() == [True, True, False]


def test_from_scans_scaled_and_isolated(scans):
    """Random scaling: one search per distinct radius, re-assembled in pair order; a NaN point with ``isolate`` costs its pair only."""
    import random
    import eyoc_amd
    s0, s1, M2 = scans
    tb = _batch(scans, random_scale=True, pyrandom=random.Random(1))
    assert len(set(tb.scale.tolist())) == 3
    seg0, seg1 = [int(v) for v in tb.seg0], [int(v) for v in tb.seg1]
    parts = []
    for b in range(3):
        c = eyoc_amd.matching_indices_batched([tb.pcd0[b]], [tb.pcd1[b]], tb.T_gt64[b:b + 1], SEARCH * tb.scale[b], collated=False)[0]
        parts.append(c + torch.tensor([[seg0[b], seg1[b]]], device=c.device))
    assert torch.equal(tb.correspondences, torch.cat(parts)) and tb.seg_m.tolist() == np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    pose = tb.pose.cpu().numpy()
    want = R.quantize_posed([s0[1]], pose[2:3], tb.scale[1:2], VOXEL)
    assert tb.pcd0[1].cpu().numpy().tobytes() == want[2].tobytes()
    broken = [c.copy() for c in s1]
    broken[0][5, 2] = np.nan
    iso = _batch((s0, broken, M2), isolate=True)
    assert iso.valid.tolist() == [False, True, False] and iso.len_batch[0][1] == 0 and iso.faults[1, 1] > 0 and not iso.faults[2:].any()
    assert torch.equal(iso.pcd0[1], _batch(scans).pcd0[1])


# ---- 7. it trains
def test_one_training_iteration(scans):
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    from eyoc_amd.train import forward_train
    tb = _batch(scans, n=2)
    assert tb.valid.tolist() == [True, True]
    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_weights(seed=21).items()})
    model = model.cuda().train()
    F0, F1 = forward_train(model, tb.sinput0).F, forward_train(model, tb.sinput1).F
    assert F0.shape == (len(tb.sinput0_C), 32) and F1.shape == (len(tb.sinput1_C), 32)
    pos, neg = eyoc_amd.contrastive_hardest_negative_loss(F0, F1, tb.correspondences, num_pos=512, num_hn_samples=256,
                                                          rng=np.random.RandomState(0))
    (pos + neg).backward()
    assert math.isfinite(float(pos.detach())) and math.isfinite(float(neg.detach()))
    grad = model.conv1.kernel.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
