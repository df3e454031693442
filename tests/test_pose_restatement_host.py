"""The fp64 restatements of the pose solvers (``tests/pose_restatement.py``) are pinned before the device is held to them: against
the reference's golden vectors and the fp32 oracle, against a second solution method, for scale invariance, and every case family is
checked to be what its name says.  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

import _inputs as gi
import pose_restatement as pr
from oracle import pose as op


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# ----------------------------------------------------------------------------- the goldens and the oracle, at test_oracle_golden's bars
def test_irls_restatement_meets_golden_and_oracle(golden_dir):
    g = _load(golden_dir, "g2_irls.npz")
    for i, (seed, n, frac, use_w, tp) in enumerate(json.loads(str(g["cases"]))):
        p0, p1, _ = gi.corr_case(seed, n, gi.rigid(*tp), frac)
        w = (0.05 + 0.95 * gi._u(seed + 9, n, 1)).astype(np.float32) if use_w else None
        T = pr.irls(p0, p1, w, 20)
        To = op.est_quad_linear_robust(torch.from_numpy(p0), torch.from_numpy(p1), None if w is None else torch.from_numpy(w)).numpy()
        np.testing.assert_allclose(T, g[f"T{i}"], rtol=0, atol=2e-5, err_msg=f"case {i}")
        np.testing.assert_allclose(T, To, rtol=0, atol=2e-5, err_msg=f"case {i} (oracle)")


def test_kabsch_restatement_meets_golden_and_oracle(golden_dir):
    from make_golden_inputs import kabsch_inputs
    from test_oracle_golden import well_conditioned
    g = _load(golden_dir, "g3_kabsch.npz")
    for i, case in enumerate(json.loads(str(g["cases"]))):
        A, B, w = kabsch_inputs(*case)
        T = pr.kabsch_batch(A, B, w)[0]
        To = op.rigid_transform_3d(torch.from_numpy(A), torch.from_numpy(B), None if w is None else torch.from_numpy(w)).numpy()
        ok = well_conditioned(A, B, w)
        assert ok.mean() > 0.9
        np.testing.assert_allclose(T[ok], g[f"T{i}"][ok], rtol=0, atol=5e-4, err_msg=f"case {i} {case}")
        np.testing.assert_allclose(T[ok], To[ok], rtol=0, atol=5e-4, err_msg=f"case {i} {case} (oracle)")
        np.testing.assert_allclose(np.linalg.det(T[:, :3, :3]), 1.0, atol=1e-4)


# ----------------------------------------------------------------------------- IRLS: two solution methods
@pytest.mark.parametrize("name", [c[0] for c in pr.IRLS_CASES])
def test_irls_lstsq_and_normal_equations_agree(name):
    """What licenses the one-ulp bar of the device test: the device solves each step through fp64 normal equations, the restatement by
    ``lstsq``; in float64 the two stay under a hundredth of an fp32 ulp of each other on every case, the clouds 800 m out included
    (measured: under 0.001)."""
    p0, p1, w, iters = pr.irls_case(name)
    T = pr.irls(p0, p1, w, iters)
    assert np.isfinite(T).all()
    if w is not None:
        assert np.linalg.matrix_rank(p0[w != 0].astype(np.float64) - p0[w != 0][0]) >= 2, "three non-collinear rows must carry weight"
    u = pr.parity_ulps(pr.irls_normal_equations(p0, p1, w, iters), T)
    print(f"{name}: lstsq vs normal equations {u:.2e} ulp")
    assert u < 0.01
    if iters == 0:
        np.testing.assert_array_equal(T, np.eye(4))


def test_irls_gather_cases_two_methods_and_layout():
    for seed, n0, n1 in ((31, 700, 400), (32, 90, 60)):
        p0, p1, idx = pr.irls_repeat_case(seed, n0, n1)
        T = pr.irls(p0, p1, None, 20, idx)
        assert pr.parity_ulps(pr.irls_normal_equations(p0, p1, None, 20, idx), T) < 0.01
        np.testing.assert_array_equal(T, pr.irls(p0, p1[idx], None, 20))              # the gather is the only thing idx1 does
        np.testing.assert_allclose(T, pr.T_TRUE, atol=0.01)
    p0, p1, w, iters = pr.irls_case("n65_it20")
    rows, idx = pr.irls_gather_layout(p1, 5, 7)
    assert len(rows) == 72
    np.testing.assert_array_equal(rows[idx], p1)


def _schedule_shift(iters, halve):
    p0, p1, w, it = pr.irls_case(f"sched_it{iters}")
    assert it == iters
    return pr.parity_ulps(pr.irls(p0, p1, w, iters, halve=halve), pr.irls(p0, p1, w, iters))


def test_irls_schedule_is_visible_in_the_cases():
    """An off-by-one in the halving of ``par`` must move the answer by more than the device test's bar of one ulp.  The weights of iteration i
    are made at the end of iteration i - 1, so what a run of k iterations ends on is the ``par`` of iteration k - 2: halving one iteration
    EARLY changes that for k = 6, 11 and 16 (hundreds of ulps); halving one iteration LATE changes only how far the run has converged on
    the same weights, which is less - a few ulps at 10 and 20 iterations."""
    for iters in (6, 11, 16):
        u = _schedule_shift(iters, (4, 9, 14))
        print(f"{iters} iterations, halving at 4, 9, 14: {u:.1f} ulp away")
        assert u > 10
    late = {iters: _schedule_shift(iters, (6, 11, 16)) for iters in (10, 15, 20)}
    print("halving at 6, 11, 16:", {k: round(v, 1) for k, v in late.items()}, "ulp away")
    assert min(late.values()) > 1 and max(late.values()) > 4     # the store of a wrong device adds at most half an ulp either way
    assert _schedule_shift(6, (6, 11, 16)) == 0.0                # six iterations never see par = 0.5
    assert _schedule_shift(5, (4, 9, 14)) == 0.0


# ----------------------------------------------------------------------------- Kabsch: scale invariance of the restatement
@pytest.mark.parametrize("n", pr.SCALE_NS)
def test_kabsch_restatement_is_scale_invariant(n):
    """Weights times 2^e with the 1e-6 of the denominator scaled along (``eps 2^e``) is the unscaled problem exactly, so R and t must not
    move; with the 1e-6 fixed, as the solver has it, tiny weights pull both centroids towards zero - the restatement follows that formula
    and only R's insensitivity to the scale of H is asserted, not any value of t.  Coordinates times 2^k scale t by 2^k."""
    A, B, w = pr.kabsch_scale_case(n)
    T0, H0, s0 = pr.kabsch(A, B, w)
    for e in range(-100, 41, 10):
        we = pr.pow2(w, e)
        assert (we != 0).all() and (np.abs(we) >= np.finfo(np.float32).tiny).all()
        T, H, s = pr.kabsch(A, B, we, eps=np.ldexp(1e-6, e))
        np.testing.assert_allclose(T, T0, rtol=0, atol=1e-12, err_msg=f"weights 2^{e}")
        np.testing.assert_allclose(pr.rotation_from_H(np.ldexp(H0, e))[0], T0[:3, :3], rtol=0, atol=1e-12)
    T1 = pr.kabsch(A, B, None)[0]
    for k in range(-40, 11, 10):
        T = pr.kabsch(pr.pow2(A, k), pr.pow2(B, k), None)[0]
        np.testing.assert_allclose(T[:3, :3], T1[:3, :3], rtol=0, atol=1e-12, err_msg=f"coordinates 2^{k}")
        np.testing.assert_allclose(np.ldexp(T[:3, 3], -k), T1[:3, 3], rtol=0, atol=1e-12 * 40, err_msg=f"coordinates 2^{k}")
    # the scales the device test uses are matrix-parity cases: R is unique at every one of them
    for e in pr.WEIGHT_SCALES:
        T, H, s = pr.kabsch(A, B, pr.pow2(w, e))
        assert s[1] >= 1e-2 * s[0] and np.linalg.det(H) > 0, (e, s)
        ca, cb, _ = pr.kabsch_terms(A, B, pr.pow2(w, e))
        if e <= -54:                                               # den ~ 1e-6: the centroids are gone, t with them
            assert np.abs(ca).max() < 1e-6 and np.abs(T[:3, 3]).max() < 1e-5


# ----------------------------------------------------------------------------- every family is what its name says
@pytest.mark.parametrize("n,bs,kind", pr.KABSCH_SHAPES)
def test_kabsch_shape_cases_are_well_conditioned(n, bs, kind):
    A, B, w = pr.kabsch_shape_case(n, bs, kind)
    assert A.shape == B.shape == (bs, n, 3) and A.dtype == np.float32
    if kind == "zeros":
        assert 0.3 < (w == 0).mean() < 0.7
    elif kind == "uniform":
        assert w.min() >= 0.25 and w.max() <= 1.0
    T, H, s = pr.kabsch_batch(A, B, w)
    for b in range(bs):                                            # every problem, nothing masked
        assert s[b, 1] >= 1e-2 * s[b, 0], (b, s[b])
        assert pr.rotation_is_unique(H[b], s[b])
        np.testing.assert_allclose(T[b, :3, :3], pr._poses(7000 + 13 * n + bs, bs)[b][:3, :3], atol=0.05 if n > 4 else 0.2)


def test_kabsch_threshold_case_keeps_a_unique_rotation():
    A, B, w, wt = pr.kabsch_threshold_case(0.5)
    assert 0.2 < (wt == 0).mean() < 0.5 and (wt[wt != 0] >= 0.5).all() and (w > 0).all()
    T, H, s = pr.kabsch_batch(A, B, wt)
    assert all(pr.rotation_is_unique(H[b], s[b]) for b in range(3))
    assert pr.parity_ulps(pr.kabsch_batch(A, B, w)[0], T) > 100        # the threshold is visible in the answer


def test_kabsch_shape_cases_cover_the_boundaries():
    ns = {c[0] for c in pr.KABSCH_SHAPES}
    assert ns == {3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025}
    for n in ns:
        assert any(c[0] == n and c[1] % 4 for c in pr.KABSCH_SHAPES), n
    for side in (lambda n: n <= 256, lambda n: n > 256):
        assert {c[1] for c in pr.KABSCH_SHAPES if side(c[0])} == {1, 2, 3, 4, 5, 9}
        assert {c[2] for c in pr.KABSCH_SHAPES if side(c[0])} == set(pr.KABSCH_WEIGHTS)


def _geometry_cases():
    return [(f, n) for f in pr.GEOMETRY_FAMILIES for n in pr.GEOMETRY_NS] + [("n1", 1), ("n2", 2)]


@pytest.mark.parametrize("family,n", _geometry_cases())
def test_kabsch_geometry_families_are_what_they_say(family, n):
    A, B, w = pr.kabsch_geometry_case(family, n)
    assert A.shape == B.shape == (n, 3)
    T, H, s = pr.kabsch(A, B, w)
    R = T[:3, :3]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-13)
    assert abs(np.linalg.det(R) - 1) < 1e-13
    hscale = (np.abs(A).max() * np.abs(B).max()) * n
    if family in pr.GEOMETRY_RATIOS:
        (lo2, hi2), (lo3, hi3) = pr.GEOMETRY_RATIOS[family]
        assert s[0] > 1e-3 * hscale
        assert lo2 <= s[1] / s[0] <= hi2 and lo3 <= s[2] / s[0] <= hi3, s / s[0]
    else:                                                           # no spread at all: H is the 1e-6 of the denominator, or nothing
        assert s[0] <= 1e-9 * hscale, s
    if family in ("mirrored", "planar_mirrored"):
        assert np.linalg.det(H) < 0 or s[2] <= 1e-12 * s[0]        # the best orthogonal fit is a reflection (or one costs nothing)
        Ro = np.linalg.svd(H)[2].T @ np.linalg.svd(H)[0].T
        if family == "mirrored":
            assert np.linalg.det(Ro) < 0
    if family == "zero_weights":
        np.testing.assert_array_equal(T, np.eye(4))
    if family == "one_weight":
        assert (w != 0).sum() == 1
    if family == "all_equal":
        assert (A == A[0]).all() and (B == B[0]).all()
    unique = pr.rotation_is_unique(H, s)
    assert unique == (family in ("mirrored", "planar", "planar_mirrored", "octahedron", "square")), (family, s)
