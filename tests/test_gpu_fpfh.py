"""FPFH descriptors on the device (csrc/fpfh.hip, eyoc_amd/fpfh.py) against the fp64 restatement of their contract
(tests/fpfh_restatement.py).

Bounds, none of them taken from the kernel's output (``fpfh_restatement.check_against``):
* ``hist`` and ``count`` are EXACTLY the restatement's on decided rows.  A row is undecided when one of its pair features lies within
  1e-9 of a bin edge or of a tie of the swap test (the device's and numpy's ``acos`` / ``atan2`` may differ in the last place), or when
  a neighbour sits within 1e-9 r^2 of the radius; at most 1 % of the rows may be.
* ``feat`` is within one fp32 step of ``float32(F)`` on rows that read no undecided histogram: both sides round one fp64 value once,
  and the fp64 values differ only by the summation order of at most 127 non-negative terms.
Clouds have at most a few hundred rows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fpfh_restatement as R

pytestmark = pytest.mark.gpu

SEEDS = (3, 4)          # tests/test_fpfh_restatement_host.py checks the undecided share of the same inputs
RANGE = 8


@functools.lru_cache(maxsize=None)
def _ref(kind, seed, n, side, radius, max_nn, zero_normals=False):
    """-> (pts, normals, restatement); shared between the tests, never modified"""
    if kind == "wavy":
        pts, nrm = R.wavy_cloud(seed, n, side)
    elif kind == "cubic":
        pts, nrm = R.cubic_lattice(seed, n)
    elif kind == "planar":
        pts, nrm = R.planar_lattice(n)
    else:
        pts, nrm = R.wavy_cloud(seed, n, side)      # "special": a duplicated point and an exact tie of the swap test
        pts = np.concatenate([pts, pts[:1], np.array([[100.0, 0.0, 0.0], [100.25, 0.0, 0.0]], np.float32)])
        nrm = np.concatenate([nrm, nrm[1:2], np.array([[0.6, 0.8, 0.0], [0.6, 0.0, 0.8]], np.float32)])
    if zero_normals:
        nrm = nrm.copy()
        nrm[::7] = 0.0
    for a in (pts, nrm):
        a.setflags(write=False)
    return pts, nrm, R.fpfh_rows(pts, nrm, radius, max_nn)


def _run(clouds, radius, max_nn, normalize=False, pad=False):
    """clouds: [(pts, normals)] -> (feat, hist, count, status) as numpy, and the segments"""
    from eyoc_amd import fpfh
    seg = np.concatenate([[0], np.cumsum([len(p) for p, _ in clouds])]).astype(int)
    pts = np.concatenate([p for p, _ in clouds]).astype(np.float32).reshape(-1, 3)
    nrm = np.concatenate([q for _, q in clouds]).astype(np.float32).reshape(-1, 3)
    feat, hist, count, status = fpfh.compute_fpfh_batched(torch.from_numpy(pts), seg, radius, max_nn, normals=torch.from_numpy(nrm),
                                                          normalize=normalize, pad=pad, return_hist=True)
    torch.cuda.synchronize()
    return feat.cpu().numpy(), hist.cpu().numpy(), count.cpu().numpy(), status.cpu().numpy(), seg


def _check_cloud(ref, out, seg, b, normalized=None):
    feat, hist, count, status, _ = out
    sl = slice(seg[b], seg[b + 1])
    assert status[b] == 0
    R.check_against(ref, hist[sl], count[sl], feat[sl], None if normalized is None else normalized[0][sl])


@pytest.mark.parametrize("seed", SEEDS)
def test_parity_with_the_restatement(seed):
    pts, nrm, ref = _ref("wavy", seed, 700, 5.6, R.WAVY["radius"], R.WAVY["max_nn"])
    assert ref.undecided_F.mean() <= 0.01
    out = _run([(pts, nrm)], **R.WAVY)
    outn = _run([(pts, nrm)], normalize=True, **R.WAVY)
    _check_cloud(ref, out, out[4], 0, outn)
    np.testing.assert_array_equal(out[1], outn[1])
    again = _run([(pts, nrm)], **R.WAVY)
    for a, b in zip(out[:4], again[:4]):
        assert a.tobytes() == b.tobytes()                     # two runs are byte-identical


SIZES = (0, 1, 2, 63, 64, 65, 129)


def _sized(i, n):
    pts, nrm, _ = _ref("wavy", 20 + i, 129, 2.4, 0.45, 24)
    return pts[:n], nrm[:n]


def test_cloud_sizes_around_the_block_and_every_cloud_alone():
    clouds = [_sized(i, n) for i, n in enumerate(SIZES)]
    out = _run(clouds, 0.45, 24)
    seg = out[4]
    for b, (p, q) in enumerate(clouds):
        ref = R.fpfh_rows(p, q, 0.45, 24)
        _check_cloud(ref, out, seg, b)
        if len(p) == 0:
            continue
        alone = _run([(p, q)], 0.45, 24)
        for a, c in zip(out[:3], alone[:3]):
            assert a[seg[b]:seg[b + 1]].tobytes() == c.tobytes()       # alone = in the batch, byte for byte
    assert out[2][seg[1]:seg[2]].tolist() == [0] and not out[0][seg[1]:seg[2]].any()     # a single point: a zero row


def test_65_tiny_clouds_cross_the_chunk():
    pts, nrm, _ = _ref("wavy", 30, 325, 2.0, 0.45, 24)
    clouds = [(pts[5 * i:5 * i + 5] * 0.3, nrm[5 * i:5 * i + 5]) for i in range(65)]       # shrunk: the five rows see each other
    out = _run(clouds, 0.45, 24)
    seg = out[4]
    assert (out[3] == 0).all()
    for b in (0, 1, 63, 64):
        ref = R.fpfh_rows(*clouds[b], 0.45, 24)
        _check_cloud(ref, out, seg, b)
        alone = _run([clouds[b]], 0.45, 24)
        assert out[0][seg[b]:seg[b + 1]].tobytes() == alone[0].tobytes()
    assert out[2].max() >= 1


@pytest.mark.parametrize("max_nn,n,side,radius", [(2, 200, 3.0, 0.45), (128, 300, 1.6, 0.9)])
def test_max_nn_at_both_ends(max_nn, n, side, radius):
    pts, nrm, ref = _ref("wavy", 5, n, side, radius, max_nn)
    assert ref.k.max() == max_nn - 1
    if max_nn == 128:
        x = pts.astype(np.float64)
        assert (((x[:, None] - x[None]) ** 2).sum(-1) < radius * radius).sum(1).max() > 129      # more rows inside than the list takes
    out = _run([(pts, nrm)], radius, max_nn)
    _check_cloud(ref, out, out[4], 0)


def test_lattice_ties_straddle_the_cut():
    """0.25 lattice, radius 0.6: 6 neighbours at 0.25, 12 at 0.354, 8 at 0.433, 6 at 0.5, 24 at 0.559 - a list of 15 ends inside the
    second shell, whose members tie exactly, so the cut is by row index"""
    pts, nrm, ref = _ref("cubic", 3, 6, 0.0, 0.6, 16)
    assert ref.k.max() == 15 and not ref.undecided_hist.any()
    out = _run([(pts, nrm)], 0.6, 16)
    _check_cloud(ref, out, out[4], 0)
    np.testing.assert_array_equal(out[2], ref.k)
    np.testing.assert_array_equal(out[1].astype(np.int64), ref.cnt)


def test_strides_33_and_64_agree():
    pts, nrm, _ = _ref("wavy", SEEDS[0], 700, 5.6, R.WAVY["radius"], R.WAVY["max_nn"])
    for normalize in (False, True):
        a = _run([(pts, nrm)], normalize=normalize, **R.WAVY)[0]
        b = _run([(pts, nrm)], normalize=normalize, pad=True, **R.WAVY)[0]
        assert a.shape == (700, 33) and b.shape == (700, 64)
        assert not b[:, 33:].any() and a.tobytes() == np.ascontiguousarray(b[:, :33]).tobytes()


def test_duplicate_points_and_an_exact_swap_tie():
    pts, nrm, ref = _ref("special", SEEDS[0], 300, 3.6, R.WAVY["radius"], R.WAVY["max_nn"])
    out = _run([(pts, nrm)], **R.WAVY)
    outn = _run([(pts, nrm)], normalize=True, **R.WAVY)
    _check_cloud(ref, out, out[4], 0, outn)
    assert any((d == 0.0).any() for d in ref.d2)


def test_rows_with_zero_normals():
    pts, nrm, ref = _ref("wavy", SEEDS[1], 300, 3.6, R.WAVY["radius"], R.WAVY["max_nn"], True)
    out = _run([(pts, nrm)], **R.WAVY)
    _check_cloud(ref, out, out[4], 0)


def test_bad_clouds_are_isolated():
    good0, good1 = _sized(3, 63), _sized(5, 65)
    base = _run([good0, good1], 0.45, 24)
    p, q = _sized(4, 64)
    nan_pt, nan_nrm, far = p.copy(), q.copy(), p.copy()
    nan_pt[17, 1] = np.nan
    nan_nrm[5, 2] = np.nan
    far[40, 0] = 1.0e6                                       # cell 2.2e6, beyond 2^17
    for bad in ((nan_pt, q), (p, nan_nrm), (far, q)):
        out = _run([good0, bad, good1], 0.45, 24)
        seg = out[4]
        assert out[3].tolist() == [0, RANGE, 0]
        for a in out[:3]:
            assert not a[seg[1]:seg[2]].any()                # zero rows, zero counts
        for a, b in zip(out[:3], base[:3]):
            assert np.concatenate([a[:seg[1]], a[seg[2]:]]).tobytes() == b.tobytes()


def _raw_call(pts, nrm, radius, max_nn, stride, short=0):
    from eyoc_amd import _lib
    lib = _lib.load()
    p, q = torch.from_numpy(np.array(pts)).cuda(), torch.from_numpy(np.array(nrm)).cuda()
    n = p.shape[0]
    seg = (C.c_int32 * 2)(0, n)
    out = torch.full((n, 64), 7.0, dtype=torch.float32, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    need = lib.eyoc_fpfh_workspace_bytes(1, n, max_nn if 2 <= max_nn <= 128 else 16)
    ws = _lib.workspace(need, p.device)
    rc = lib.eyoc_fpfh_batched(_lib.ctx(0), _lib.ptr(p), _lib.ptr(q), seg, 1, float(radius), max_nn, 0, stride, _lib.ptr(out), None, None,
                               _lib.ptr(status), _lib.ptr(ws), need - short, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), status.cpu().numpy()


def test_argument_and_workspace_errors():
    from eyoc_amd import _lib
    pts, nrm = _sized(2, 64)
    for radius, max_nn, stride in ((0.0, 16, 33), (-1.0, 16, 33), (float("nan"), 16, 33), (float("inf"), 16, 33), (0.45, 1, 33), (0.45, 0, 33),
                                   (0.45, 129, 33), (0.45, 16, 32), (0.45, 16, 34)):
        rc, out, status = _raw_call(pts, nrm, radius, max_nn, stride)
        assert rc == _lib.ERR_INVALID and (out == 7.0).all() and status[0] == 77
    assert _lib.load().eyoc_fpfh_workspace_bytes(1, 64, 1) == 0
    rc, out, status = _raw_call(pts, nrm, 0.45, 16, 64, short=1)
    assert rc == _lib.ERR_WORKSPACE and (out == 7.0).all() and status[0] == 77       # nothing written
    rc, out, status = _raw_call(pts, nrm, 0.45, 16, 64)
    assert rc == 0 and status[0] == 0 and not out[:, 33:].any() and out[:, :33].any()


def test_planar_lattice_on_the_device():
    pts, nrm, ref = _ref("planar", 0, 6, 0.0, 1.5, 40)
    out = _run([(pts, nrm)], 1.5, 40)
    want = np.zeros((len(pts), 33), np.float32)
    want[:36, [5, 16, 27]] = 200.0
    np.testing.assert_array_equal(out[0], want)              # exactly 200.0; the lone points: zero rows
    np.testing.assert_array_equal(out[2], ref.k)


def test_python_entry_points_and_the_shim():
    import eyoc_amd
    import eyoc_amd.o3d as o3d
    pts, nrm, _ = _ref("wavy", SEEDS[0], 700, 5.6, R.WAVY["radius"], R.WAVY["max_nn"])
    pts, nrm = np.array(pts), np.array(nrm)          # writable copies: these go to torch as they are
    feat = _run([(pts, nrm)], **R.WAVY)[0]
    one = eyoc_amd.compute_fpfh_feature(pts, normals=nrm, **R.WAVY)
    assert one.is_cuda and one.cpu().numpy().tobytes() == feat.tobytes()
    # normals=None: the estimated normals, whichever way they are handed over
    est, st = eyoc_amd.estimate_normals_batched(torch.from_numpy(pts), [0, 700], 0.6, 30)
    a, sa = eyoc_amd.compute_fpfh_batched(pts, [0, 700], normal_radius=0.6, **R.WAVY)
    b, sb = eyoc_amd.compute_fpfh_batched(pts, [0, 700], normals=est, **R.WAVY)
    assert int(st[0]) == int(sa[0]) == int(sb[0]) == 0 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        eyoc_amd.compute_fpfh_batched(pts, [0, 700], **R.WAVY)
    bad = pts.copy()
    bad[3, 0] = np.inf
    assert int(eyoc_amd.compute_fpfh_batched(bad, [0, 700], normal_radius=0.6, **R.WAVY)[1][0]) == RANGE
    with pytest.raises(eyoc_amd.EyocError):
        eyoc_amd.compute_fpfh_feature(bad, normals=nrm, **R.WAVY)
    # the shim: [33, n] float64 of the same values
    pcd = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(pts))
    with pytest.raises(RuntimeError):
        o3d.pipelines.registration.compute_fpfh_feature(pcd, o3d.geometry.KDTreeSearchParamHybrid(R.WAVY["radius"], R.WAVY["max_nn"]))
    pcd.normals = o3d.utility.Vector3dVector(nrm)
    f = o3d.pipelines.registration.compute_fpfh_feature(pcd, o3d.geometry.KDTreeSearchParamHybrid(R.WAVY["radius"], R.WAVY["max_nn"]))
    assert isinstance(f, o3d.pipelines.registration.Feature) and f.data.dtype == np.float64 and f.data.shape == (33, 700)
    np.testing.assert_array_equal(f.data, feat.T.astype(np.float64))
    pcd.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(0.6, 30))
    np.testing.assert_array_equal(pcd.normals, est.cpu().numpy().astype(np.float64))
    with pytest.raises(NotImplementedError):
        o3d.registration.registration_icp(pcd, pcd, 0.2, np.eye(4), o3d.pipelines.registration.TransformationEstimationPointToPlane())


def _o3d_cloud(o3d, pts, vs):
    pcd = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(pts))
    pcd.estimate_normals(o3d.geometry.KDTreeSearchParamHybrid(2 * vs, 30))
    return pcd, o3d.pipelines.registration.compute_fpfh_feature(pcd, o3d.geometry.KDTreeSearchParamHybrid(5 * vs, 100))


def test_shim_ransac_on_fpfh_features():
    import eyoc_amd.o3d as o3d
    src, tgt, T = R.corner_scene()
    vs, d = R.SCENE["voxel_size"], R.SCENE["distance_threshold"]
    (p0, f0), (p1, f1) = _o3d_cloud(o3d, src, vs), _o3d_cloud(o3d, tgt, vs)
    reg = o3d.pipelines.registration
    res = reg.registration_ransac_based_on_feature_matching(
        p0, p1, f0, f1, False, d, reg.TransformationEstimationPointToPoint(False), 4,
        [reg.CorrespondenceCheckerBasedOnEdgeLength(0.9), reg.CorrespondenceCheckerBasedOnDistance(d)], reg.RANSACConvergenceCriteria(400000, 10000))
    assert res.transformation.shape == (4, 4) and res.fitness > 0.3
    assert R.registered(res.transformation, T)[0]


@pytest.mark.parametrize("backend", ["ransac", "sc2pcr"])
def test_end_to_end_registration_from_raw_points(backend):
    """The scene of fpfh_restatement.corner_scene: on the CPU the restatement's normalised rows, a brute-force nearest neighbour and the
    oracle's RANSAC (400 000 hypotheses, seeds 0 and 1: rte 0.12 / 0.13 m, rre 0.9 / 0.5 degrees) and SC2-PCR (0.02 m, 0.9 degrees)
    register it by the reference's criterion (rte < 2 m, rre < 5 degrees).  The device chain must meet the same criterion."""
    import eyoc_amd
    src, tgt, T = R.corner_scene()
    src2, tgt2, T2 = R.corner_scene(seed=12)
    kw = dict(voxel_size=R.SCENE["voxel_size"], distance_threshold=R.SCENE["distance_threshold"], backend=backend, max_iteration=400000)
    one = eyoc_amd.register_fpfh_batched(src, tgt, [0, len(src)], [0, len(tgt)], seed=0, **kw)
    assert len(one) == 1 and R.registered(one[0].transformation, T)[0], R.registered(one[0].transformation, T)
    both = eyoc_amd.register_fpfh_batched(np.concatenate([src, src2]), np.concatenate([tgt, tgt2]), [0, len(src), len(src) + len(src2)],
                                          [0, len(tgt), len(tgt) + len(tgt2)], seed=0, **kw)
    two = eyoc_amd.register_fpfh_batched(src2, tgt2, [0, len(src2)], [0, len(tgt2)], seed=1, **kw)       # pair b draws with seed + b
    for got, want in zip(both, (one[0], two[0])):
        assert got.transformation.tobytes() == want.transformation.tobytes()
        assert (got.fitness, got.inlier_rmse, got.inliers) == (want.fitness, want.inlier_rmse, want.inliers)
    mutual = eyoc_amd.register_fpfh_batched(src, tgt, [0, len(src)], [0, len(tgt)], seed=0, mutual=True, **kw)
    assert R.registered(mutual[0].transformation, T)[0]


@pytest.mark.parametrize("backend", ["ransac", "sc2pcr"])
def test_failed_pairs_leave_their_neighbours_alone(backend):
    """Four pairs: a good one, one whose source holds a NaN (RANGE), a good one, one without target rows (FEW).  The failed pairs carry
    their status and the identity; a good pair gets the record it gets alone, drawing with seed + its place in the batch."""
    import eyoc_amd
    from eyoc_amd import icp
    src, tgt, _ = R.corner_scene()
    src2, tgt2, _ = R.corner_scene(seed=12)
    bad = src.copy()
    bad[7, 2] = np.nan
    srcs, tgts = [src, bad, src2, src[:50]], [tgt, tgt, tgt2, tgt[:0]]
    seg_s = np.concatenate([[0], np.cumsum([len(a) for a in srcs])])
    seg_t = np.concatenate([[0], np.cumsum([len(a) for a in tgts])])
    kw = dict(voxel_size=R.SCENE["voxel_size"], distance_threshold=R.SCENE["distance_threshold"], backend=backend, max_iteration=100000)
    out = eyoc_amd.register_fpfh_batched(np.concatenate(srcs), np.concatenate(tgts), seg_s, seg_t, seed=5, **kw)
    assert [r.status for r in out] == [0, icp.RANGE, 0, icp.FEW]
    for b in (1, 3):
        assert np.array_equal(out[b].transformation, np.eye(4)) and out[b].fitness == 0.0
    for b in (0, 2):
        alone = eyoc_amd.register_fpfh_batched(srcs[b], tgts[b], [0, len(srcs[b])], [0, len(tgts[b])], seed=5 + b, **kw)[0]
        assert out[b].transformation.tobytes() == alone.transformation.tobytes()
        assert (out[b].fitness, out[b].inlier_rmse, out[b].inliers) == (alone.fitness, alone.inlier_rmse, alone.inliers)
