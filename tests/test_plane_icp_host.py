"""CPU checks around point-to-plane ICP: the restatement the GPU tests trust (tests/plane_icp_restatement.py) against brute force and
against a second solver, the host side of the new entry points, and the harness option.  No device compute."""
import os
import re

import numpy as np
import pytest

import plane_icp_restatement as PR
from eyoc_amd import icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the restatement imports nothing from the package: its status bits are the package's by this line
assert (PR.CONVERGED, PR.BAD_INIT, PR.FEW, PR.RANGE, PR.SINGULAR) == (icp.CONVERGED, icp.BAD_INIT, icp.FEW, icp.RANGE, icp.SINGULAR)


def _lattice(n, pitch=0.3):
    g = (np.arange(n, dtype=np.float32) - np.float32(n // 2)) * np.float32(pitch)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32(4.0)


@pytest.mark.parametrize("max_nn", [30, 0, 1, 64])
def test_restated_neighbour_sets_equal_brute_force_on_a_cloud(max_nn):
    pts = np.random.default_rng(5).normal(size=(300, 3)).astype(np.float32)
    a, b = PR.neighbours(pts, 1.0, max_nn), PR.neighbours_brute(pts, 1.0, max_nn)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    k = np.bincount(a[0], minlength=300)
    assert k.min() >= 1 and (a[1][np.searchsorted(a[0], np.arange(300))] == np.arange(300)).all()      # a row's first neighbour is itself
    if max_nn == 30:
        assert (k == 30).any() and (k < 30).any()


def test_restated_neighbour_sets_equal_brute_force_on_a_lattice_with_ties_at_the_cut():
    pts = _lattice(6)
    a, b = PR.neighbours(pts, 0.65, 30), PR.neighbours_brute(pts, 0.65, 30)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    # the cut goes through a group of exactly equal d2: entry 30 of a row's uncut list has the d2 of entry 29, and the lower row won
    i, j, d2 = PR.neighbours_brute(pts, 0.65, 0)
    first = np.searchsorted(i, np.arange(len(pts)))
    k = np.bincount(i, minlength=len(pts))
    rows = np.flatnonzero(k > 30)
    tied = [r for r in rows if d2[first[r] + 29] == d2[first[r] + 30]]
    assert len(tied) > 0
    for r in tied[:5]:
        assert j[first[r] + 29] < j[first[r] + 30]
        kept = a[1][a[0] == r]
        assert len(kept) == 30 and kept[-1] == j[first[r] + 29]


def test_restated_normals_of_a_plane_and_the_sign_rule():
    rng = np.random.default_rng(1)
    xy = rng.uniform(-2, 2, size=(400, 2))
    pts = np.concatenate([xy, np.full((400, 1), -1.5)], 1).astype(np.float32)        # the ground under a sensor at the origin
    n = PR.normals(pts, 0.8, 30)
    live = n.k >= 3
    assert live.sum() > 300
    np.testing.assert_allclose(n.normals[live], np.broadcast_to([0.0, 0.0, 1.0], (int(live.sum()), 3)), atol=1e-9)      # n . x <= 0: up
    assert (n.normals[~live] == 0).all()
    assert np.isinf(n.beta[~live]).all() and (n.beta[live] < 1e-9).all()


def test_lstsq_step_equals_the_ldl_step():
    rng = np.random.default_rng(2)
    p = rng.uniform(-20, 20, size=(500, 3))
    nrm = rng.normal(size=(500, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    q = p + rng.normal(size=(500, 3)) * 0.05
    J, r = PR.jacobian(p, q, nrm)
    assert np.linalg.cond(J.T @ J) < 1e4 and not PR.singular(J.T @ J)
    a, b = PR.step_lstsq(J, r), PR.step_ldl(J, r)
    assert np.abs(a - b).max() < 1e-9
    # a plane with one normal leaves three directions free: the rule sees it
    J, r = PR.jacobian(p, q, np.broadcast_to([0.0, 0.0, 1.0], p.shape))
    assert PR.singular(J.T @ J)
    assert PR.singular(np.zeros((6, 6)))
    U = PR.motion(np.array([0.1, -0.2, 0.3, 1.0, 2.0, 3.0]))
    np.testing.assert_allclose(U[:3, :3] @ U[:3, :3].T, np.eye(3), atol=1e-15)
    np.testing.assert_allclose(U[:3, 3], [1.0, 2.0, 3.0])
    assert abs(U[2, 0] + np.sin(-0.2)) < 1e-15            # Rz Ry Rx: R[2][0] = -sin(beta)


def test_struct_and_abi():
    from eyoc_amd import _lib, icp
    lib = _lib.load()
    assert icp.SINGULAR == 16 and PR.SINGULAR == 16
    hdr = open(os.path.join(ROOT, "include", "eyoc_hip.h")).read()
    assert re.search(r"EYOC_ICP_SINGULAR\s*=\s*16\b", hdr)
    for name in ("eyoc_normals_workspace_bytes", "eyoc_normals_batched", "eyoc_icp_plane_workspace_bytes", "eyoc_icp_plane_batched"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    # host functions: no GPU is touched
    assert lib.eyoc_normals_workspace_bytes(0, 100) == 0 and lib.eyoc_normals_workspace_bytes(-1, 100) == 0
    assert lib.eyoc_normals_workspace_bytes(1, -1) == 0
    assert lib.eyoc_icp_plane_workspace_bytes(0, 10, 10) == 0 and lib.eyoc_icp_plane_workspace_bytes(1, -1, 10) == 0
    for n_clouds, total in ((1, 0), (1, 1), (1, 5000), (65, 12345), (1024, 1 << 20)):
        b = lib.eyoc_normals_workspace_bytes(n_clouds, total)
        assert b > 0 and b % 256 == 0
        b = lib.eyoc_icp_plane_workspace_bytes(n_clouds, total, total // 2)
        assert b > 0 and b % 256 == 0
        assert b >= lib.eyoc_icp_workspace_bytes(n_clouds, total, total // 2)        # the larger partials and the normals
    import eyoc_amd
    for name in ("estimate_normals", "estimate_normals_batched", "icp_plane_batched", "registration_icp_point_to_plane"):
        assert getattr(eyoc_amd, name) is getattr(icp, name)


def test_harness_option():
    from eyoc_amd.harness import RegistrationConfig
    cfg = RegistrationConfig()
    assert (cfg.icp_method, cfg.icp_normal_radius, cfg.icp_normal_max_nn) == ("point", None, 30)
    assert RegistrationConfig(icp_method="plane").icp_method == "plane"
    with pytest.raises(ValueError):
        RegistrationConfig(icp_method="bogus")
