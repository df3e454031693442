"""Pin the CPU oracle against golden vectors produced by the reference's own functions
(tests/golden/make_golden.py).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

import _inputs as gi
from oracle import matching as om
from oracle import pose as op
from oracle import sc2pcr as osc


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# ----------------------------------------------------------------------------- G1
@pytest.mark.parametrize("tag", ["big", "odd", "wide"])
def test_find_nn_matches_reference(golden_dir, tag):
    g = _load(golden_dir, "g1_nn.npz")
    seed, n0, n1 = (int(v) for v in g[f"{tag}_meta"])
    F0, F1 = gi.nn_case(seed, n0, n1)
    inds, d2 = om.find_nn(F0, F1, nn_max_n=500, return_distance=True)
    ref_i, ref_d = g[f"{tag}_inds"].astype(np.int64), g[f"{tag}_d2"]
    # distances agree to fp32 round-off of a 32-term sum
    np.testing.assert_allclose(d2[:, 0], ref_d, rtol=0, atol=4e-6)
    # tie audit: indices may differ only where the runner-up is within round-off of the winner
    diff = np.nonzero(inds != ref_i)[0]
    assert len(diff) <= max(2, n0 // 1000), f"{len(diff)} index mismatches"
    for i in diff:
        D = om.sqdist_rows(F0[i:i + 1], F1)[0]
        assert abs(D[inds[i]] - D[ref_i[i]]) <= 4e-6
    # 'L2' variant
    indsL, dL = om.find_nn(F0, F1, return_distance=True, dist_type="L2")
    np.testing.assert_allclose(dL[:, 0], g[f"{tag}_d_l2"], rtol=0, atol=4e-6)
    assert (indsL != g[f"{tag}_inds_l2"]).sum() <= max(2, n0 // 1000)


def test_pdist_matches_reference(golden_dir):
    g = _load(golden_dir, "g1_nn.npz")
    A, B = gi.nn_case(14, 16, 8)
    np.testing.assert_allclose(om.pdist(A, B, "SquareL2"), g["small_pdist_sq"], atol=2e-6)
    np.testing.assert_allclose(om.pdist(A, B, "L2"), g["small_pdist_l2"], atol=2e-6)


def test_find_nn_tie_goes_to_lowest_index():
    F1 = np.zeros((5, 4), np.float32)
    F1[1] = F1[3] = [1, 0, 0, 0]
    F0 = np.array([[1, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    assert om.find_nn(F0, F1).tolist() == [1, 0]


# ----------------------------------------------------------------------------- G6
def _match_pair_draws(seed, n0, n1, num_node):
    """The rows ``Matcher.match_pair`` samples (SC2_PCR.py:284-289) from the global ``np.random`` seeded by the case."""
    if num_node == "all":
        return np.arange(n0), np.arange(n1)
    rs = np.random.RandomState(seed)
    return rs.choice(n0, num_node), rs.choice(n1, num_node)


def test_match_pair_matches_reference(golden_dir):
    """oracle.match_pair_indices vs the reference's own Matcher.match_pair (golden g6): unit-norm descriptors, exact
    ties, descriptors that are not unit-norm (NaN rows) and the with-replacement resampling.  The reference sums the
    32 products inside sgemm; indices may differ from the oracle's FMA chain only where two candidates' distances
    are within rounding - those rows are audited one by one."""
    g = _load(golden_dir, "g6_match.npz")
    n_nan_rows = 0
    for i, (kind, seed, n0, n1, num_node) in enumerate(json.loads(str(g["cases"]))):
        F0, F1 = gi.match_pair_case(kind, seed, n0, n1)
        s_sel, t_sel = _match_pair_draws(seed, n0, n1, num_node)
        np.testing.assert_array_equal(g[f"src{i}"], s_sel)                 # the draw itself is reproduced
        A, B = F0[s_sel], F1[t_sel]
        idx = om.match_pair_indices(A, B)
        ref_local = g[f"tgt{i}"].astype(np.int64)                           # = t_sel[argmin]: original target row
        got = t_sel[idx]
        diff = np.nonzero(got != ref_local)[0]
        assert len(diff) <= max(2, len(A) // 500), f"case {i}: {len(diff)} index mismatches"
        D = om.match_pair_distance(A[diff], B) if len(diff) else None
        for r, row in enumerate(diff):
            cand = np.nonzero(t_sel == ref_local[row])[0]                   # the reference's pick, in local numbering
            d_ref, d_got = D[r, cand[0]], D[r, idx[row]]
            if np.isnan(d_got):      # a NaN row: the reference must have picked a (near-)NaN candidate too
                assert np.isnan(d_ref) or om.dot_rows(A[row:row + 1], B[cand[:1]])[0, 0] > 1.0 - 1e-5
            else:
                assert abs(float(d_ref) - float(d_got)) <= 2e-4 * max(1.0, float(d_got)), f"case {i} row {row}"
        n_nan_rows += int(np.isnan(om.match_pair_distance(A[:256], B)).any(axis=1).sum())
        if kind == "ties":           # exact duplicates: never the third copy; the second only where the first was nudged
            assert (idx < n1 // 3 + 200).all()
    assert n_nan_rows > 0, "the raw cases must exercise the NaN rule"


def test_match_pair_nan_and_tie_rules():
    A = np.array([[1.0, 0, 0, 0], [2.0, 0, 0, 0], [0.5, 0, 0, 0]], np.float32)
    B = np.array([[0.2, 0, 0, 0], [1.0, 0, 0, 0], [1.0, 0, 0, 0], [3.0, 0, 0, 0]], np.float32)
    # row 0: S = .2, 1, 1, 3 -> w < 0 only for S = 3: NaN at index 3 wins;  row 1: S = .4, 2, 2, 6: first NaN = 1;
    # row 2: S = .1, .5, .5, 1.5: NaN at 3
    assert om.match_pair_indices(A, B).tolist() == [3, 1, 3]
    assert om.match_pair_indices(A, B[:3]).tolist() == [1, 1, 1]           # ties -> lowest index
    t = torch.sqrt(2 - 2 * (torch.from_numpy(A) @ torch.from_numpy(B).T) + 1e-6).argmin(dim=1)
    assert t.tolist() == [3, 1, 3]                                          # torch.argmin's NaN rule, as assumed


def test_fmaf_emulation_is_correctly_rounded():
    from fractions import Fraction
    rng = np.random.default_rng(5)
    n = 3000
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)).astype(np.float32)
    c[:50] = -(a[:50].astype(np.float64) * b[:50]).astype(np.float32)       # cancellation
    r = om.fmaf(a, b, c)
    for i in range(n):
        ex = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(ex))
        cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - ex), int(x.view(np.uint32)) & 1))
        assert best == r[i]


# ----------------------------------------------------------------------------- G2
def test_irls_matches_reference(golden_dir):
    g = _load(golden_dir, "g2_irls.npz")
    cases = json.loads(str(g["cases"]))
    for i, (seed, n, frac, use_w, tp) in enumerate(cases):
        p0, p1, _ = gi.corr_case(seed, n, gi.rigid(*tp), frac)
        w = None
        if use_w:
            w = torch.from_numpy((0.05 + 0.95 * gi._u(seed + 9, n, 1)).astype(np.float32))
        T = op.est_quad_linear_robust(torch.from_numpy(p0), torch.from_numpy(p1), w).numpy()
        np.testing.assert_allclose(T, g[f"T{i}"], rtol=0, atol=2e-5, err_msg=f"case {i}")


# ----------------------------------------------------------------------------- G3
def well_conditioned(A, B, w, tol=1e-3):
    """Kabsch is ill-posed when the (weighted, centred) points are nearly collinear: the second
    singular value of H vanishes and round-off decides the rotation about the line.  Such batch
    elements (one 3-point case in the fixture) are excluded from element-wise comparison."""
    w = np.ones(A.shape[:2], np.float32) if w is None else w
    ws = w.sum(1, keepdims=True)[:, :, None] + 1e-6
    Am = A - (A * w[:, :, None]).sum(1, keepdims=True) / ws
    Bm = B - (B * w[:, :, None]).sum(1, keepdims=True) / ws
    H = np.einsum("bni,bnj->bij", Am, w[:, :, None] * Bm).astype(np.float64)
    s = np.linalg.svd(H, compute_uv=False)
    return s[:, 1] > tol * s[:, 0]


def test_kabsch_matches_reference(golden_dir):
    from make_golden_inputs import kabsch_inputs
    g = _load(golden_dir, "g3_kabsch.npz")
    cases = json.loads(str(g["cases"]))
    for i, case in enumerate(cases):
        A, B, w = kabsch_inputs(*case)
        T = op.rigid_transform_3d(torch.from_numpy(A), torch.from_numpy(B),
                                  None if w is None else torch.from_numpy(w)).numpy()
        ok = well_conditioned(A, B, w)
        assert ok.mean() > 0.9
        np.testing.assert_allclose(T[ok], g[f"T{i}"][ok], rtol=0, atol=5e-4, err_msg=f"case {i} {case}")
        R = T[:, :3, :3]
        np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-4)


# ----------------------------------------------------------------------------- G4
def test_sc2pcr_matches_reference(golden_dir):
    g = _load(golden_dir, "g4_sc2pcr.npz")
    cases = json.loads(str(g["cases"]))
    cfg = json.loads(str(g["cfg"]))
    assert cfg == osc.KITTI_CFG
    m = osc.Matcher(**cfg)
    for i, (seed, n, frac, tp) in enumerate(cases):
        p0, p1, _ = gi.corr_case(seed, n, gi.rigid(*tp), frac, noise=0.03)
        T, fit = m.SC2_PCR(torch.from_numpy(p0)[None], torch.from_numpy(p1)[None])
        np.testing.assert_allclose(T[0].numpy(), g[f"T{i}"], rtol=0, atol=2e-4, err_msg=f"case {i}")
        assert float(fit.max()) == pytest.approx(float(g[f"fitmax{i}"]), abs=2)
        # and the recovered pose is the planted one
        np.testing.assert_allclose(T[0].numpy(), gi.rigid(*tp), atol=0.05)


def test_leading_eigenvector_matches_reference(golden_dir):
    g = _load(golden_dir, "g4_sc2pcr.npz")
    M = gi._u(45, 256, 256)
    M = ((M + M.T) * 0.5).astype(np.float32)
    np.fill_diagonal(M, 0)
    v = osc.Matcher(**osc.KITTI_CFG).cal_leading_eigenvector(torch.from_numpy(M)[None])[0].numpy()
    np.testing.assert_allclose(v, g["eig_vec"], atol=1e-6)


# ----------------------------------------------------------------------------- G5
def test_se3_helpers_match_reference(golden_dir):
    g = _load(golden_dir, "g5_se3.npz")
    pts = ((gi._u(51, 3, 40, 3) - 0.5) * 10).astype(np.float32)
    R = np.stack([gi.rot_zyx(*((gi._u(52 + b, 3) - 0.5) * 2)) for b in range(3)]).astype(np.float32)
    t = ((gi._u(55, 3, 3, 1) - 0.5) * 5).astype(np.float32)
    T = op.integrate_trans(torch.from_numpy(R), torch.from_numpy(t))
    np.testing.assert_array_equal(T.numpy(), g["T"])
    np.testing.assert_allclose(op.transform(torch.from_numpy(pts), T).numpy(), g["warped"], atol=1e-6)
    np.testing.assert_allclose(op.transform(torch.from_numpy(pts[0]), T[0]).numpy(), g["warped0"], atol=1e-6)


# ----------------------------------------------------------------------------- G6 (hand-computed)
def _product_metrics():
    import eyoc_amd.metrics as pm      # numpy only: importable (and checked) without a GPU
    return pm


@pytest.mark.parametrize("which", ["oracle", "product"])
def test_metrics_hand_cases(which):
    """scripts/test_kitti.py:187-211 on hand-computed cases - the oracle's twin AND eyoc_amd.metrics (the copy the
    harness and bench report with)."""
    op = globals()["op"] if which == "oracle" else _product_metrics()
    T = np.eye(4, dtype=np.float32)
    assert op.registration_errors(T, T) == (0.0, 0.0, True)
    a = np.deg2rad(3.0)
    Tr = np.eye(4, dtype=np.float32)
    Tr[:3, :3] = gi.rot_zyx(0, 0, a)
    Tr[:3, 3] = (1.0, 0.0, 0.0)
    rte, rre, ok = op.registration_errors(Tr, T)
    assert rte == pytest.approx(1.0) and rre == pytest.approx(a, abs=2e-4) and ok
    Tr[:3, 3] = (2.5, 0, 0)
    assert op.registration_errors(Tr, T)[2] is False          # RTE >= 2 m
    Tr[:3, :3] = gi.rot_zyx(0, 0, np.deg2rad(6.0))
    Tr[:3, 3] = 0
    assert op.registration_errors(Tr, T)[2] is False          # RRE >= 5 deg
    # the diagonal clamp keeps arccos finite when round-off pushes the trace above 3
    Tb = np.eye(4, dtype=np.float32)
    Tb[:3, :3] *= np.float32(1.0000002)
    assert not np.isnan(op.registration_errors(Tb, T)[1])
    d = op.evaluate_nn_dist(np.zeros((2, 3)), np.array([[3.0, 4.0, 0.0], [0, 0, 0]]), np.eye(4))
    np.testing.assert_allclose(d, [np.sqrt(25 + 1e-6), 1e-3], rtol=1e-6)


def test_loss_helpers_match_reference_when_present(golden_dir):
    """oracle.loss.pdist / pair_hash against lib.metrics.pdist and util.misc._hash of the reference: their outputs on seeded
    inputs are stored in g11_host.npz (tests/golden/make_golden.py).  The squared distances bit for bit on rows whose sums are
    exact in any order; everything else within a few ulps - the reference's own bits depend on the CPU (summation order of the
    32 terms, and torch's vectorised fp32 sqrt, which is not correctly rounded), and the stored run was on another one."""
    from oracle import loss as ol
    g = _load(golden_dir, "g11_host.npz")
    A, B, pairs = gi.loss_helper_case(31)
    E0, E1 = gi.exact_rows_case(34)
    np.testing.assert_array_equal(ol.pdist(torch.from_numpy(E0), torch.from_numpy(E1), "SquareL2").numpy(), g["pdist_exact_SquareL2"])
    np.testing.assert_allclose(ol.pdist(torch.from_numpy(E0), torch.from_numpy(E1), "L2").numpy(), g["pdist_exact_L2"], rtol=1e-6, atol=0)
    for t in ("L2", "SquareL2"):
        np.testing.assert_allclose(ol.pdist(torch.from_numpy(A), torch.from_numpy(B), t).numpy(), g[f"pdist_{t}"], rtol=1e-6, atol=0)
    np.testing.assert_array_equal(ol.pair_hash(pairs, 5000), g["hash_array"])
    np.testing.assert_array_equal(ol.pair_hash([pairs[:, 0], pairs[:, 1]], 5000), g["hash_list"])


# ----------------------------------------------------------------------------- G7: hardest-contrastive loss (lib/trainer.py:935-991)
def _loss_cases(golden_dir):
    g = _load(golden_dir, "g7_loss.npz")
    return g, json.loads(str(g["cases"]))


@pytest.mark.parametrize("i", [0, 1, 2])
def test_oracle_loss_matches_reference_values_and_gradients(golden_dir, i):
    """oracle/loss.py against the reference's own ``contrastive_hardest_negative_loss`` run on the same seeded inputs with
    the global ``np.random`` seeded the same way: both loss terms (case 1: the reference's NaN mean over no negatives) and the
    gradients of ``pos + neg`` with respect to both descriptor sets."""
    from oracle import loss as ol
    g, cases = _loss_cases(golden_dir)
    seed, n0, n1, npairs, num_pos, nhn = cases[i]
    F0n, F1n, pairs = gi.loss_case(seed, n0, n1, npairs)
    F0, F1 = torch.from_numpy(F0n).requires_grad_(True), torch.from_numpy(F1n).requires_grad_(True)
    pos, neg = ol.contrastive_hardest_negative_loss(F0, F1, pairs, num_pos=num_pos, num_hn_samples=nhn, rng=np.random.RandomState(seed))
    (pos + neg).backward()
    np.testing.assert_allclose(float(pos.detach()), float(g[f"pos{i}"]), rtol=1e-6)
    np.testing.assert_allclose(float(neg.detach()), float(g[f"neg{i}"]), rtol=1e-6, equal_nan=True)
    for got, want in ((F0.grad.numpy(), g[f"gF0_{i}"]), (F1.grad.numpy(), g[f"gF1_{i}"])):
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * np.abs(want).max())


# ----------------------------------------------------------------------------- G8: ratio test + top-k (lib/trainer.py:993-1016)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_oracle_ratio_test_and_topk_match_reference(golden_dir, i):
    """The fixture's inputs are what ``knn_points(K = 2)`` hands the trainer (and must be what oracle.labels.knn2 computes
    from the seeded descriptors); weights bit-exact against ``calculate_ratio_test`` on the cosines of :1066-1070, top-k
    against ``get_topk_matches`` (``torch.topk`` leaves the order of equal weights open: compared as the same multiset of
    weights in the same order, and the same (source, target) pairs wherever the weight is unique)."""
    from oracle import labels as olb
    g = _load(golden_dir, "g8_labels.npz")
    seed, n0, n1, k = json.loads(str(g["cases"]))[i]
    F0, F1 = gi.nn_case(seed, n0, n1)
    idx, d1, d2 = olb.knn2(F0, F1)
    np.testing.assert_array_equal(idx, g[f"idx{i}"])
    np.testing.assert_array_equal(d1, g[f"d1_{i}"])
    np.testing.assert_array_equal(d2, g[f"d2_{i}"])
    w = olb.lowe_weights(d1, d2)
    np.testing.assert_array_equal(w, g[f"w{i}"])
    src, tgt, top = olb.topk_matches(w, idx, k)
    assert len(src) == min(k, n0)
    np.testing.assert_array_equal(top, g[f"top{i}"])
    vals, counts = np.unique(top, return_counts=True)
    uniq = counts[np.searchsorted(vals, top)] == 1
    assert uniq.mean() > 0.99
    np.testing.assert_array_equal(src[uniq], g[f"src{i}"][uniq])
    np.testing.assert_array_equal(tgt[uniq], g[f"tgt{i}"][uniq])


# ----------------------------------------------------------------------------- G10: match_and_filter_corr (lib/trainer.py:1025-1151)
def same_rows_up_to_topk_ties(got, want, what=""):
    """``torch.topk`` leaves the order of equal weights open: the same rows, and in the same places except where neighbours of equal
    weight swapped (a handful of rows)."""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    key = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))]
    np.testing.assert_array_equal(key(got), key(want), err_msg=what)
    assert (got != want).any(1).mean() < 0.01, what


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_oracle_match_and_filter_corr_matches_reference(golden_dir, i):
    """oracle.labels.match_and_filter_corr against the reference's own method run on a batch of three pairs (G10: the method
    unmodified; its two pytorch3d calls given bodies for the fixture only - a list-to-padded-tensor holder and STORED K = 2
    neighbours): the collated matches with their biases, and the per-pair survivors of the spherical / similarity / no filter."""
    from oracle import labels as olb
    g = _load(golden_dir, "g10_match_filter.npz")
    ff, sf, fd = json.loads(str(g["cases"]))[i]
    C0s, F0s, C1s, F1s = gi.label_batch_case(101)
    m, unc = olb.match_and_filter_corr(C0s, F0s, C1s, F1s, 20, ff, sf, frame_distance=fd, dist_sim_map=gi.dist_sim_table(), similarity_thresh=0.3)
    same_rows_up_to_topk_ties(m, g[f"matches{i}"], "matches")
    assert len(unc) == 3
    for p, u in enumerate(unc):
        same_rows_up_to_topk_ties(u, g[f"unc{i}_{p}"], f"pair {p}")
        if sf != "None":
            assert 0 < len(u) < 1800


# ----------------------------------------------------------------------------- G9: find_corr / random_sample / apply_transform / evaluate_nn_dist
@pytest.mark.parametrize("i", [0, 1, 2])
def test_oracle_find_corr_matches_reference(golden_dir, i):
    """scripts/test_kitti.py:28-42 with the global ``np.random`` seeded: the rows drawn and their nearest neighbours (points
    are index-coded).  Mismatches only at fp32 near-ties of the NN, as for G1."""
    g = _load(golden_dir, "g9_eval.npz")
    seed, n0, n1, sub = json.loads(str(g["cases"]))[i]
    F0, F1 = gi.nn_case(seed, n0, n1)
    x0 = np.zeros((n0, 3), np.float32); x0[:, 0] = np.arange(n0)
    x1 = np.zeros((n1, 3), np.float32); x1[:, 0] = np.arange(n1)
    a, b = om.find_corr(x0, x1, F0, F1, subsample_size=sub, rng=np.random.RandomState(seed))
    np.testing.assert_array_equal(a[:, 0].astype(np.int32), g[f"corr0_{i}"])
    got, want = b[:, 0].astype(np.int32), g[f"corr1_{i}"]
    diff = np.nonzero(got != want)[0]
    assert len(diff) <= max(1, len(got) // 1000)
    rows = a[:, 0].astype(np.int64)
    for r in diff:
        D = om.sqdist_rows(F0[rows[r]:rows[r] + 1], F1)[0]
        assert abs(D[got[r]] - D[want[r]]) <= 4e-6


@pytest.mark.parametrize("which", ["oracle", "product"])
def test_random_sample_and_nn_dist_match_reference(golden_dir, which):
    g = _load(golden_dir, "g9_eval.npz")
    if which == "oracle":
        sample = lambda p, f, N, s: om.random_sample(p, f, N, np.random.RandomState(s))
        applyT, nn_dist = op.apply_transform, op.evaluate_nn_dist
    else:
        import importlib.util
        spec = importlib.util.spec_from_file_location("_eyoc_metrics", os.path.join(os.path.dirname(golden_dir), "..", "eyoc_amd", "metrics.py"))
        pm = importlib.util.module_from_spec(spec); spec.loader.exec_module(pm)
        sample = None                                   # eyoc_amd.eval.random_sample needs the GPU package: tests/test_gpu_goldens.py
        applyT, nn_dist = pm.apply_transform, pm.evaluate_nn_dist
    if sample is not None:
        for j, (n, N) in enumerate(((1000, 300), (200, 500), (64, 64))):
            pts = np.zeros((n, 3), np.float32); pts[:, 0] = np.arange(n)
            feats = np.arange(n * 4, dtype=np.float32).reshape(n, 4)
            p, f = sample(pts, feats, N, 100 + j)
            np.testing.assert_array_equal(p[:, 0].astype(np.int32), g[f"rs_p{j}"])
            np.testing.assert_array_equal(f, g[f"rs_f{j}"])
    T = g["T"]
    pts = ((gi._u(95, 500, 3) - 0.5) * 60).astype(np.float32)
    tgt = (pts @ T[:3, :3].T + T[:3, 3] + 0.05 * gi._normal(96, 500, 3)).astype(np.float32)
    np.testing.assert_allclose(np.asarray(applyT(pts, T)), g["applied"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(np.asarray(nn_dist(pts, tgt, T)), g["nn_dist"], rtol=2e-5, atol=2e-6)
