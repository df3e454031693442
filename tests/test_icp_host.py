"""ICP refinement, the part that needs no GPU: the C ABI (symbols, struct sizes), the Open3D shim's defaults and refusals, and the CPU
restatement the GPU tests compare against (tests/icp_restatement.py) checked against an O(N M) brute-force evaluation and hand cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_restatement as R
from eyoc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("eyoc_icp_workspace_bytes", "eyoc_icp_batched", "eyoc_icp_correspondences")


def test_header_declares_and_lib_binds_the_icp_entry_points():
    src = open(os.path.join(ROOT, "include", "eyoc_hip.h")).read()
    assert "added after 111 without a bump, additive only" in src.lower()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.PROTOTYPES
    for name in ("eyoc_icp_params", "eyoc_icp_result"):
        assert re.search(r"\}\s*%s\s*;" % name, code), name
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.eyoc_version() == 111


def test_struct_sizes():
    assert C.sizeof(_lib.IcpParams) == 32
    assert C.sizeof(_lib.IcpResult) == 160
    assert _lib.IcpResult.fitness.offset == 128 and _lib.IcpResult.status.offset == 152


def test_workspace_bytes_is_a_host_function():
    lib = _lib.load()
    a, b = lib.eyoc_icp_workspace_bytes(1, 5000, 5000), lib.eyoc_icp_workspace_bytes(64, 320000, 320000)
    assert 0 < a < b and a % 256 == 0
    assert lib.eyoc_icp_workspace_bytes(0, 10, 10) == 0


def test_shim_defaults_and_refusals():
    import eyoc_amd.o3d as o3d
    c = o3d.pipelines.registration.ICPConvergenceCriteria()
    assert (c.relative_fitness, c.relative_rmse, c.max_iteration) == (1e-6, 1e-6, 30)
    assert o3d.pipelines.registration.ICPConvergenceCriteria(max_iteration=200).max_iteration == 200
    assert o3d.registration.registration_icp is o3d.pipelines.registration.registration_icp
    a = o3d.geometry.PointCloud(np.zeros((4, 3)))
    with pytest.raises(NotImplementedError):
        o3d.pipelines.registration.registration_icp(a, a, 0.2, np.eye(4), o3d.pipelines.registration.TransformationEstimationPointToPoint(True))
    with pytest.raises(NotImplementedError):
        o3d.pipelines.registration.registration_icp(a, a, 0.2, np.eye(4), o3d.pipelines.registration.TransformationEstimationPointToPlane())
    with pytest.raises(TypeError):
        o3d.pipelines.registration.registration_icp(np.zeros((4, 3)), a, 0.2)
    T = np.eye(4)
    T[:3, 3] = (1.0, 2.0, 3.0)
    assert np.array_equal(o3d.geometry.PointCloud(np.ones((2, 3))).transform(T).points, np.array([[2.0, 3.0, 4.0]] * 2))


def test_registration_result_keeps_its_old_constructions():
    from eyoc_amd.registration import RegistrationResult
    r = RegistrationResult(np.eye(4), 0.5, 0.1, 7, 3, 2)
    assert (r.inliers, r.best_hypothesis, r.survivors, r.status, r.iterations, r.correspondence_set) == (7, 3, 2, 0, 0, None)


def test_harness_config_defaults_leave_icp_off():
    from eyoc_amd.harness import RegistrationConfig
    c = RegistrationConfig()
    assert c.icp_refine is False and c.icp_max_correspondence_distance is None and c.icp_max_iteration == 30


def test_no_gpu_means_loud_failure(monkeypatch):
    """Without a visible GPU the ICP entry points raise; there is no CPU path (the restatement lives under tests/ only)."""
    import torch
    import eyoc_amd
    from eyoc_amd import icp
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(eyoc_amd.EyocError):
        icp.registration_icp(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32), 0.2)
    with pytest.raises(eyoc_amd.EyocError):
        icp.icp_batched(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32), [0, 8], [0, 8], 0.2)


def _clouds(seed, n=2000, m=2000):
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-6, 6, (m, 3)).astype(np.float32)
    src = (tgt[rng.integers(0, m, n)] + rng.normal(0, 0.2, (n, 3))).astype(np.float32)
    return src, tgt


def test_restatement_matches_brute_force_bit_for_bit():
    src, tgt = _clouds(0)
    T = R.perturb(np.eye(4), np.random.default_rng(1), 2.0, 0.1)
    for r in (0.3, 0.6):
        a, b = R.evaluate(src, tgt, T, r), R.evaluate_brute(src, tgt, T, r)
        assert 0 < (a.corr >= 0).sum() < len(src)
        np.testing.assert_array_equal(a.corr, b.corr)
        assert a.d2.tobytes() == b.d2.tobytes()
        assert (a.fitness, a.inlier_rmse) == (b.fitness, b.inlier_rmse)
        np.testing.assert_array_equal(a.margin, b.margin)


def test_exact_tie_goes_to_the_lowest_row():
    tgt = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 5]], np.float32)
    e = R.evaluate(np.zeros((1, 3), np.float32), tgt, np.eye(4), 1.5)
    assert e.corr[0] == 0 and e.d2[0] == 1.0 and e.margin[0] == 0.0
    assert R.evaluate(np.zeros((1, 3), np.float32), tgt, np.eye(4), 1.0).corr[0] == -1       # strict gate


def test_identity_on_identical_clouds():
    _, tgt = _clouds(2)
    for it in (0, 30):
        run = R.icp(tgt, tgt, 0.3, np.eye(4), it)
        assert np.array_equal(run.T, np.eye(4)) or np.abs(run.T - np.eye(4)).max() < 1e-14
        assert run.fitness == 1.0 and run.inlier_rmse < 1e-14 and run.correspondences == len(tgt)
    assert R.icp(tgt, tgt, 0.3, np.eye(4), 0).iterations == 0
    run = R.icp(tgt, tgt, 0.3, np.eye(4), 30)
    assert run.iterations == 1 and run.status == R.CONVERGED


def test_small_translation_is_recovered():
    """A pure translation below the gate, with every coordinate exactly representable (multiples of 1/64): recovered to 1e-12."""
    _, tgt = _clouds(3, m=600)
    tgt = (np.round(tgt * 4 * 64) / 64).astype(np.float32)   # spacing far above the gate: every point finds its own partner
    shift = np.array([0.0625, -0.03125, 0.015625])
    src = (tgt.astype(np.float64) - shift).astype(np.float32)
    assert np.array_equal(src.astype(np.float64) + shift, tgt.astype(np.float64))
    run = R.icp(src, tgt, 0.3, np.eye(4), 30)
    want = np.eye(4)
    want[:3, 3] = shift
    assert run.status == R.CONVERGED and run.fitness == 1.0 and run.iterations == 2
    assert np.abs(run.T - want).max() < 1e-12 and run.inlier_rmse < 1e-12


def test_status_paths():
    _, tgt = _clouds(4, m=100)
    assert R.icp(np.zeros((0, 3), np.float32), tgt, 0.3).status == R.FEW
    far = R.icp(tgt[:2], tgt, 0.3, np.eye(4))                # 2 correspondences
    assert far.status & R.FEW and far.correspondences == 2 and far.iterations == 0 and np.array_equal(far.T, np.eye(4))
    bad = np.eye(4)
    bad[0, 3] = np.nan
    assert R.icp(tgt, tgt, 0.3, bad).status == R.BAD_INIT
    nan_pt = tgt.copy()
    nan_pt[5, 1] = np.nan
    assert R.icp(nan_pt, tgt, 0.3).status == R.RANGE and R.icp(tgt, nan_pt, 0.3).status == R.RANGE
    away = tgt.copy()
    away[7] = 1e9
    assert R.icp(tgt, away, 0.3).status == R.RANGE
