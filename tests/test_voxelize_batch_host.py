"""CPU-side checks of the batched voxeliser (eyoc_voxelize_batched / sparse_quantize_batch): workspace sizing, the argument checks
that run before the device is touched, and the host pieces of DeviceBatch.from_scans.  No device compute."""
import numpy as np
import pytest

from eyoc_amd import _lib


def test_batched_workspace_covers_single_cloud_and_grows():
    lib = _lib.load()
    for n in (1, 1000, 123457, 15_000_000):
        single = lib.eyoc_voxelize_workspace_bytes(n)
        sizes = [lib.eyoc_voxelize_batched_workspace_bytes(n, b) for b in (1, 64, 128, 1024)]
        assert sizes[0] >= single
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
    for b in (1, 128, 1024):
        by_n = [lib.eyoc_voxelize_batched_workspace_bytes(n, b) for n in (1000, 100_000, 15_000_000)]
        assert all(a < b for a, b in zip(by_n, by_n[1:]))
    assert lib.eyoc_voxelize_batched_workspace_bytes(1000, 0) == 0
    assert lib.eyoc_voxelize_batched_workspace_bytes(-1, 4) == 0


def test_sparse_quantize_batch_rejects_bad_arguments_before_the_device():
    from eyoc_amd import sparse_quantize_batch
    rng = np.random.default_rng(0)
    c3 = rng.uniform(-5, 5, (100, 3)).astype(np.float32)
    c4 = rng.uniform(-5, 5, (100, 4)).astype(np.float32)
    with pytest.raises(ValueError, match="mixed"):
        sparse_quantize_batch([c3, c4], 0.3)
    with pytest.raises(ValueError, match="batch indices"):
        sparse_quantize_batch([c3] * 1025, 0.3)
    with pytest.raises(ValueError, match="batch indices"):
        sparse_quantize_batch([c3] * 30, 0.3, batch_base=1000)
    with pytest.raises(ValueError, match="voxel_size"):
        sparse_quantize_batch([c3], 0.0)
    with pytest.raises(ValueError, match="voxel_size"):
        sparse_quantize_batch([c3], -0.3)
    with pytest.raises(ValueError, match=r"\[N,3\] or \[N,4\]"):
        sparse_quantize_batch([c3, c3[:, :2]], 0.3)
    with pytest.raises(ValueError, match="no clouds"):
        sparse_quantize_batch([], 0.3)


def test_sample_indices_are_the_batch_draws():
    """The helper both DeviceBatch constructors use: the draws of random_sample as DeviceBatch always made them."""
    from eyoc_amd.harness import sample_indices
    from eyoc_amd.synthetic import subsample_indices
    for seed, i, n in ((3, 0, 31000), (3, 1, 29000), (7, 1, 5000)):
        np.testing.assert_array_equal(sample_indices(seed, i, n, 5000), subsample_indices(seed * 2 + i, n, 5000))
    small = sample_indices(4, 1, 1200, 5000)
    np.testing.assert_array_equal(small, np.random.default_rng(4 * 2 + 1 + 10**6).choice(1200, 5000))
    assert small.max() < 1200


def test_make_pair_keep_raw_adds_the_sweeps_only():
    from eyoc_amd import synthetic as syn
    kw = dict(beams=16, azimuths=400, band=None)
    a = syn.make_pair(11, **kw)
    b = syn.make_pair(11, keep_raw=True, **kw)
    assert "raw0" not in a and set(b) == set(a) | {"raw0", "raw1"}
    for k in ("xyz0", "xyz1", "coords0", "coords1", "feats0", "feats1", "T_gt"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["stats"] == b["stats"]
    for i in (0, 1):
        raw = b[f"raw{i}"]
        assert raw.dtype == np.float32 and len(raw) == b["stats"][f"raw{i}"]
        sel, c = syn.voxelize(raw, 0.3)
        np.testing.assert_array_equal(c, b[f"coords{i}"])
        np.testing.assert_array_equal(raw[sel], b[f"xyz{i}"])


def test_from_scans_refuses_the_descriptor_mode():
    from eyoc_amd.harness import DeviceBatch
    scans = [(np.zeros((10, 3), np.float32), np.zeros((10, 3), np.float32))]
    with pytest.raises(ValueError, match="descriptor"):
        DeviceBatch.from_scans(scans, [np.eye(4)], [0], "cuda:0", descriptor=dict(inlier_ratio=0.3))
