"""GPU parity of the batched voxeliser + collation (eyoc_voxelize_batched / sparse_quantize_batch / DeviceBatch.from_scans): integer
work, bit-exact against the per-cloud voxeliser and the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def per_cloud(clouds, voxel, batch_base=0):
    """The contract: the concatenation of the single-cloud calls, in cloud order."""
    import eyoc_amd
    coords, sel, xyz, offsets = [], [], [], [0]
    for b, c in enumerate(clouds):
        c = c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c, np.float32)
        cc, ss = eyoc_amd.sparse_quantize(c, voxel, batch_base + b)
        coords.append(cc.cpu().numpy())
        sel.append(ss.cpu().numpy())
        xyz.append(c[sel[-1]][:, :3])
        offsets.append(offsets[-1] + len(ss))
    return np.concatenate(coords), np.concatenate(sel), np.concatenate(xyz), np.asarray(offsets, np.int64)


def check(clouds, voxel, batch_base=0):
    import eyoc_amd
    from oracle import voxelize as ov
    coords, sel, xyz, offsets = eyoc_amd.sparse_quantize_batch(clouds, voxel, batch_base)
    assert coords.dtype == torch.int32 and sel.dtype == torch.int64 and xyz.dtype == torch.float32
    assert offsets.dtype == np.int64 and offsets.shape == (len(clouds) + 1,)
    got = (coords.cpu().numpy(), sel.cpu().numpy(), xyz.cpu().numpy(), offsets)
    for g, r in zip(got, per_cloud(clouds, voxel, batch_base)):
        np.testing.assert_array_equal(g, r)
    for b, c in enumerate(clouds):
        rc, rs = ov.sparse_quantize(np.asarray(c, np.float32), voxel, batch_base + b)
        lo, hi = offsets[b], offsets[b + 1]
        np.testing.assert_array_equal(got[0][lo:hi], rc)
        np.testing.assert_array_equal(got[1][lo:hi], rs)
    return got


@pytest.fixture(scope="module")
def sweeps():
    from eyoc_amd import synthetic as syn
    out = []
    for scene_seed in (5, 6):
        scene = syn.make_scene(np.random.default_rng(scene_seed))
        for k, (x, y, yaw) in enumerate(((0.0, 0.0, 0.0), (9.0, 0.4, 0.1), (-6.0, -0.3, -0.15), (15.0, 0.0, 0.05))):
            out.append(syn.raycast(scene, syn._pose(x, y, yaw), np.random.default_rng([scene_seed, k]), brush_level=1.0,
                                   beams=32, azimuths=1000))
    return out


@pytest.mark.parametrize("batch_base", [0, 5])
def test_batch_equals_per_cloud_calls_on_lidar_sweeps(sweeps, batch_base):
    got = check(sweeps, 0.3, batch_base)
    assert len(sweeps) == 8 and all(len(s) > 10000 for s in sweeps)
    assert np.array_equal(np.unique(got[0][:, 0]), np.arange(8) + batch_base)
    xyzr = [np.concatenate([s, np.full((len(s), 1), 0.5, np.float32)], 1) for s in sweeps[:3]]   # KITTI .bin rows
    got4 = check(xyzr, 0.3, batch_base)
    n3 = got[3][3]
    for a, b in zip(got4[:3], got):
        np.testing.assert_array_equal(a, b[:n3])


def test_device_and_torch_inputs(sweeps):
    import eyoc_amd
    ref = eyoc_amd.sparse_quantize_batch(sweeps[:4], 0.3)
    for clouds in ([torch.from_numpy(s).cuda() for s in sweeps[:4]],
                   [torch.from_numpy(s) for s in sweeps[:2]] + [torch.from_numpy(s).cuda() for s in sweeps[2:4]]):
        got = eyoc_amd.sparse_quantize_batch(clouds, 0.3)
        for a, b in zip(got[:3], ref[:3]):
            assert torch.equal(a, b)
        np.testing.assert_array_equal(got[3], ref[3])


def test_same_scan_twice_is_not_merged(sweeps):
    s = sweeps[0]
    coords, sel, xyz, offsets = check([s, s], 0.3)
    m = offsets[1]
    assert offsets[2] == 2 * m
    np.testing.assert_array_equal(coords[:m, 1:], coords[m:, 1:])
    assert (coords[:m, 0] == 0).all() and (coords[m:, 0] == 1).all()
    np.testing.assert_array_equal(sel[:m], sel[m:])


def test_edge_cases():
    rng = np.random.default_rng(0)
    e = np.zeros((0, 3), np.float32)
    a = rng.uniform(-3, 3, (5000, 3)).astype(np.float32)        # heavy duplication, negative cells
    b = rng.uniform(-40, 40, (7000, 3)).astype(np.float32)
    one = np.array([[0.1, -0.2, 7.0]], np.float32)
    same = np.full((300, 3), 1.05, np.float32) + rng.uniform(0, 0.1, (300, 3)).astype(np.float32)   # one voxel
    border = np.array([[-1e-7, 0.29999, 0.3], [-0.3, 0.3, 0.6], [-0.30001, 0.0, 0.0]], np.float32)
    got = check([e, e, a, e, one, same, b, border, e, e], 0.3)
    np.testing.assert_array_equal(np.diff(got[3])[[0, 1, 3, 8, 9]], 0)
    assert np.diff(got[3])[4] == 1 and np.diff(got[3])[5] == 1 and np.diff(got[3])[7] == 3
    check([a], 0.5)                                               # B = 1
    check([one], 0.3, batch_base=1023)
    big = rng.uniform(-60, 60, (9000, 3)).astype(np.float32)     # clouds straddling scan tiles at odd offsets
    check([big[:2047], big[2047:2049], e, big[2049:6144], big[6144:]], 0.25)
    check([rng.uniform(-20, 20, (n, 3)).astype(np.float32) for n in rng.integers(0, 400, 300)], 0.3, batch_base=100)


def test_all_empty_returns_empty_outputs():
    import eyoc_amd
    e = np.zeros((0, 4), np.float32)
    coords, sel, xyz, offsets = eyoc_amd.sparse_quantize_batch([e, e, e], 0.3)
    assert coords.shape == (0, 4) and sel.shape == (0,) and xyz.shape == (0, 3)
    np.testing.assert_array_equal(offsets, np.zeros(4, np.int64))


def test_point_out_of_range_names_its_cloud():
    import eyoc_amd
    rng = np.random.default_rng(1)
    clouds = [rng.uniform(-10, 10, (500, 3)).astype(np.float32) for _ in range(6)]
    clouds[3][77] = (1e6, 0.0, 0.0)
    clouds[5][3] = (0.0, -1e6, 0.0)
    with pytest.raises(eyoc_amd.EyocError, match="range") as ei:
        eyoc_amd.sparse_quantize_batch(clouds, 0.3)
    assert "cloud 3" in str(ei.value)
    assert ei.value.code == eyoc_amd._lib.ERR_RANGE
    clouds[3][77] = 0.0
    check(clouds[:5], 0.3)                                        # the context is usable after the failure


def test_raw_abi_checks():
    from eyoc_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, B = 4000, 4
    xyz = torch.rand((n, 3), device=dev) * 20
    sel = torch.empty(n, dtype=torch.int32, device=dev)
    coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    i64 = C.POINTER(C.c_int64)
    vox = np.zeros(B + 1, np.int64)

    def call(off, ws, batch_base=0, n_points=n):
        off = np.asarray(off, np.int64)
        return lib.eyoc_voxelize_batched(_lib.ctx(0), _lib.ptr(xyz), 3, off.ctypes.data_as(i64), len(off) - 1, n_points, 0.3,
                                         batch_base, _lib.ptr(sel), _lib.ptr(coords), None, vox.ctypes.data_as(i64), _lib.ptr(ws),
                                         ws.numel(), _lib.stream_ptr())

    need = lib.eyoc_voxelize_batched_workspace_bytes(n, B)
    ok = [0, 1000, 1000, 2500, n]
    assert call(ok, _lib.workspace(need - 256, dev)) == _lib.ERR_WORKSPACE
    assert call([0, 1000, 900, 2500, n], _lib.workspace(need, dev)) == _lib.ERR_INVALID        # not monotone
    assert call([0, 1000, 1000, 2500, n - 1], _lib.workspace(need, dev)) == _lib.ERR_INVALID    # last offset != total
    assert call(ok, _lib.workspace(need, dev), batch_base=1021) == _lib.ERR_RANGE               # batch_base + B > 1024
    assert call(ok, _lib.workspace(need, dev)) == 0
    torch.cuda.synchronize()
    ref = per_cloud([xyz[a:b] for a, b in zip(ok[:-1], ok[1:])], 0.3)
    np.testing.assert_array_equal(vox, ref[3])
    np.testing.assert_array_equal(sel[:vox[-1]].cpu().numpy(), ref[1])
    np.testing.assert_array_equal(coords[:vox[-1]].cpu().numpy(), ref[0])


def test_from_scans_equals_host_voxelised_batch():
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    import eyoc_amd
    dev = torch.device("cuda:0")
    seeds = [21, 22, 23, 24]
    pairs = [syn.make_pair(s, keep_raw=True, beams=32, azimuths=1000, band=None) for s in seeds]
    pairs[3] = syn.make_pair(24, keep_raw=True, beams=8, azimuths=200, band=None)      # small clouds: draws with replacement
    host = DeviceBatch(pairs, seeds, dev, n_points=2000)
    raw = DeviceBatch.from_scans([(p["raw0"], p["raw1"]) for p in pairs], [p["T_gt"] for p in pairs], seeds, dev, voxel_size=0.3,
                                 n_points=2000)
    assert min(host.sizes) < 2000 <= max(host.sizes)
    assert raw.P == host.P and raw.n_points == host.n_points and raw.beta == host.beta
    assert raw.sizes == host.sizes and raw.counts == host.counts
    assert raw.G0 is None and raw.G1 is None and host.G0 is None
    np.testing.assert_array_equal(raw.offsets, host.offsets)
    np.testing.assert_array_equal(raw.seg, host.seg)
    for a, b in zip(raw.T_gt, host.T_gt):
        np.testing.assert_array_equal(a, b)
    for name in ("coords", "feats", "sel0", "sel1", "xyz0", "xyz1"):
        a, b = getattr(raw, name), getattr(host, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, name
        assert torch.equal(a, b), name
    sd = syn.make_weights()
    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    pipe = RegistrationPipeline(model.to(dev).eval(), RegistrationConfig(ransac_max_iteration=20000))
    rec_host = pipe.register(host, seed=3, return_device=True).cpu()
    model.check_range()
    rec_raw = pipe.register(raw, seed=3, return_device=True).cpu()
    model.check_range()
    assert rec_host.shape[0] == 4 and torch.equal(rec_host, rec_raw)          # the [P, 84] result records, byte for byte
    for a, b in zip(pipe.register(host, seed=3), pipe.register(raw, seed=3)):
        np.testing.assert_array_equal(a.transformation, b.transformation)
        assert (a.inliers, a.best_hypothesis, a.survivors) == (b.inliers, b.best_hypothesis, b.survivors)
