"""GPU parity of the pose solvers of ``csrc/pose.hip`` - ``eyoc_kabsch_batched``, ``eyoc_irls_quad``, ``eyoc_irls_quad_batched`` - against their
fp64 restatements (``tests/pose_restatement.py``, pinned on the host by ``tests/test_pose_restatement_host.py``), at the shapes where the
kernels change path: the 256-point switch between the wave and the block Kabsch kernel, batches that are no multiple of the wave
kernel's four problems, the 1024-row sweep of the IRLS workgroup, both sides of every halving of ``par``.

Bars (derived, not tuned: both sides compute in float64 and the device rounds once, when it stores T):
  matrix parity      ``|T - T_ref| <= 2^-23 max(1, |T_ref|)`` per entry, "one ulp" below
  degenerate H       R a proper rotation (``|R R^T - I|``, ``|det R - 1| <= 4 2^-23``), ``t = cb - R ca`` with the restatement's centroids, and
                     ``tr(R_ref H) - tr(R H) <= 2^-24 sum |H_ij|`` - what storing R in fp32 can cost and nothing more

Realised on an MI355X (maximum over the cases of each test, in units of its bar, i.e. fp32 ulps for the parities):
  Kabsch shapes            0.46 ulp                      weight threshold wrapper   0.24 ulp
  Kabsch weights 2^e       0.42 ulp (e = 40 ... -100)    Kabsch coordinates 2^k     0.40 ulp (k = 10 ... -40)
  IRLS single / batched    0.32 / 0.32 ulp (n sweep 0.31, iteration sweep 0.30, 800 m out 0.32)
  Kabsch geometry, as parity / objective / orthogonality / det / t, each over its bound:
    mirrored 0.24 / 0.20 / 0.11 / 0.11 / 0.26     planar 0.27 / 0.05 / 0.04 / 0.00 / 0.29     planar, mirrored 0.17 / 0.05 / 0.04 / 0.00 / 0.10
    octahedron 0.13 / 0 / 0 / 0 / 0.13            square 0.13 / 0 / 0 / 0 / 0.13
    near-collinear 1e-3 - / 0.02 / 0.05 / 0.03 / 0.24     1e-5 - / 0.00 / 0.14 / 0.02 / 0.13     collinear - / 0.00 / 0.11 / 0.10 / 0.09
    all equal - / 0.21 / 0.15 / 0.10 / 0.26       one weight - / 0.10 / 0.09 / 0.04 / 0.20    n = 1 - / 0.09 / 0.08 / 0.01 / 0.07
    n = 2 - / 0.24 / 0.10 / 0.05 / 0.13           no weight: the identity, exactly
With the absolute ``1e-30`` that ``jacobi_eig3`` used to carry in its convergence test the scale tests failed - and only they: weights 2^-54
(20 points: 94 ulp), 2^-60 (2e5 and 75 ulp), 2^-66 and 2^-100 (1.8e6 and 4.4e5 ulp, a rotation 0.2 off) and coordinates 2^-40 (1.7e6 and
4.9e5 ulp)."""
import functools

import numpy as np
import pytest
import torch

import pose_restatement as pr

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kabsch_abi(A, B, w):
    """``eyoc_kabsch_batched`` on ``[bs,n,3]`` inputs into a buffer of bs + 1 transforms filled with NaN: the last one must stay NaN."""
    from eyoc_amd import _lib
    bs, n = A.shape[:2]
    a, b, wd = _dev(A), _dev(B), _dev(w)
    T = torch.full((bs + 1, 16), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().eyoc_kabsch_batched(_lib.ctx(0), _lib.ptr(a), _lib.ptr(b), _lib.ptr(wd), bs, n, _lib.ptr(T), _lib.stream_ptr()),
               "eyoc_kabsch_batched")
    torch.cuda.synchronize()
    out = T.cpu().numpy()
    assert np.isnan(out[bs]).all(), "the kernel wrote past its last problem"
    out = out[:bs].reshape(bs, 4, 4)
    np.testing.assert_array_equal(out[:, 3], np.tile(np.float32([0, 0, 0, 1]), (bs, 1)))
    return out


# ----------------------------------------------------------------------------- Kabsch
@pytest.mark.parametrize("n,bs,kind", pr.KABSCH_SHAPES)
def test_kabsch_shapes(n, bs, kind):
    import eyoc_amd
    A, B, w = pr.kabsch_shape_case(n, bs, kind)
    T = _kabsch_abi(A, B, w)
    T_ref = pr.kabsch_batch(A, B, w)[0]
    ulps = [pr.parity_ulps(T[b], T_ref[b]) for b in range(bs)]
    print(f"kabsch n={n} bs={bs} {kind}: max {max(ulps):.3f} ulp")
    assert max(ulps) <= 1.0, ulps
    Tw = eyoc_amd.rigid_transform_3d(_dev(A), _dev(B), _dev(w))           # the wrapper is that call
    assert Tw.is_cuda and Tw.shape == (bs, 4, 4)
    np.testing.assert_array_equal(Tw.cpu().numpy(), T)


def _geometry_cases():
    return [(f, n) for f in pr.GEOMETRY_FAMILIES for n in pr.GEOMETRY_NS] + [("n1", 1), ("n2", 2)]


@pytest.mark.parametrize("family,n", _geometry_cases())
def test_kabsch_geometry(family, n):
    A, B, w = pr.kabsch_geometry_case(family, n)
    T = _kabsch_abi(A[None], B[None], None if w is None else w[None])[0]
    assert np.isfinite(T).all()
    T_ref, H, s = pr.kabsch(A, B, w)
    fig = pr.rotation_checks(T, A, B, w)
    unique = pr.rotation_is_unique(H, s)
    if unique:
        fig["parity"] = pr.parity_ulps(T, T_ref)
    print(f"kabsch {family} n={n}: " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()) + " (each over its bound)")
    assert max(fig.values()) <= 1.0, fig
    if family == "zero_weights":
        np.testing.assert_array_equal(T, np.eye(4, dtype=np.float32))


@pytest.mark.parametrize("e", pr.WEIGHT_SCALES)
@pytest.mark.parametrize("n", pr.SCALE_NS)
def test_kabsch_weight_scale(n, e):
    A, B, w = pr.kabsch_scale_case(n)
    we = pr.pow2(w, e)
    T = _kabsch_abi(A[None], B[None], we[None])[0]
    u = pr.parity_ulps(T, pr.kabsch(A, B, we)[0])
    print(f"kabsch n={n}, weights 2^{e}: {u:.3f} ulp")
    assert u <= 1.0


@pytest.mark.parametrize("k", pr.COORD_SCALES)
@pytest.mark.parametrize("n", pr.SCALE_NS)
def test_kabsch_coordinate_scale(n, k):
    A, B, _ = pr.kabsch_scale_case(n)
    Ak, Bk = pr.pow2(A, k), pr.pow2(B, k)
    T = _kabsch_abi(Ak[None], Bk[None], None)[0].astype(np.float64)
    T_ref = pr.kabsch(Ak, Bk, None)[0]
    T[:3, 3], T_ref[:3, 3] = np.ldexp(T[:3, 3], -k), np.ldexp(T_ref[:3, 3], -k)      # translations at the scale of the unscaled problem
    u = pr.parity_ulps(T, T_ref)
    print(f"kabsch n={n}, coordinates 2^{k}: {u:.3f} ulp")
    assert u <= 1.0


@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_rigid_transform_3d_weight_threshold(where):
    import eyoc_amd
    A, B, w, wt = pr.kabsch_threshold_case(0.5)
    put = (lambda a: torch.from_numpy(a.copy())) if where == "cpu" else _dev
    wc = put(w)
    T = eyoc_amd.rigid_transform_3d(put(A), put(B), wc, weight_threshold=0.5)
    assert T.is_cuda == (where == "cuda") and T.shape == (3, 4, 4) and T.dtype == torch.float32
    np.testing.assert_array_equal(wc.cpu().numpy(), wt)                  # the caller's weights, thresholded in place
    T_ref = pr.kabsch_batch(A, B, wt)[0]
    u = max(pr.parity_ulps(T[b].cpu().numpy(), T_ref[b]) for b in range(3))
    print(f"rigid_transform_3d, threshold 0.5, {where}: {u:.3f} ulp")
    assert u <= 1.0


# ----------------------------------------------------------------------------- IRLS
@functools.lru_cache(maxsize=None)
def _irls_ref(name):
    p0, p1, w, iters = pr.irls_case(name)
    T = pr.irls(p0, p1, w, iters)
    T.setflags(write=False)
    return T


@pytest.mark.parametrize("name", [c[0] for c in pr.IRLS_CASES])
def test_irls_single(name):
    import eyoc_amd
    p0, p1, w, iters = pr.irls_case(name)
    T = eyoc_amd.est_quad_linear_robust(_dev(p0), _dev(p1), _dev(w), iters=iters)
    assert T.is_cuda and T.shape == (4, 4)
    T = T.cpu().numpy()
    np.testing.assert_array_equal(T[3], np.float32([0, 0, 0, 1]))
    u = pr.parity_ulps(T, _irls_ref(name))
    print(f"irls {name}: {u:.3f} ulp")
    assert u <= 1.0


@pytest.mark.parametrize("iters", sorted({c[2] for c in pr.IRLS_CASES}))
def test_irls_batched_ragged(iters):
    """Every case of this iteration count in ONE call, as a gather: each pair's p1 segment holds its partners shuffled among unmatched rows (so
    it is longer than the p0 segment), an empty pair sits between live ones, and - at 20 iterations - two pairs have more correspondences
    than target rows, so their ``idx1`` repeats."""
    import eyoc_amd
    P0, P1, I1, W, refs, names = [], [], [], [], [], []
    for k, c in enumerate(c for c in pr.IRLS_CASES if c[2] == iters):
        p0, p1, w, _ = pr.irls_case(c[0])
        rows, idx = pr.irls_gather_layout(p1, 40 + k, 5 + 3 * k)
        P0.append(p0); P1.append(rows); I1.append(idx); W.append(np.ones(len(p0), np.float32) if w is None else w)     # (no weight = weight 1)
        refs.append(_irls_ref(c[0])); names.append(c[0])
    if iters == 20:
        for seed, n0, n1 in ((31, 700, 400), (32, 90, 60)):
            p0, p1, idx = pr.irls_repeat_case(seed, n0, n1)
            P0.append(p0); P1.append(p1); I1.append(idx); W.append(np.ones(n0, np.float32))
            refs.append(pr.irls(p0, p1, None, 20, idx)); names.append(f"repeat_{n0}_over_{n1}")
    empty = (np.zeros((0, 3), np.float32), np.float32([[1, 2, 3], [4, 5, 6]]), np.zeros(0, np.int64), np.zeros(0, np.float32))
    for lst, e in zip((P0, P1, I1, W), empty):                       # an empty pair (with target rows of its own) after the first live one
        lst.insert(1, e)
    refs.insert(1, None); names.insert(1, "empty")
    seg = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)     # noqa: E731
    assert all(len(a) > len(b) for a, b, nm in zip(P1, P0, names) if not nm.startswith("repeat"))      # the p1 side is the longer one
    T = eyoc_amd.est_quad_linear_robust_batched(_dev(np.concatenate(P0)), _dev(np.concatenate(P1)), seg(P0), seg(P1),
                                                idx1=_dev(np.concatenate(I1)), weight=_dev(np.concatenate(W)), iters=iters)
    assert T.is_cuda and T.shape == (len(refs), 4, 4)
    T = T.cpu().numpy()
    assert np.isnan(T[1]).all()
    worst = 0.0
    for b, (name, ref) in enumerate(zip(names, refs)):
        if ref is None:
            continue
        u = pr.parity_ulps(T[b], ref)
        worst = max(worst, u)
        assert u <= 1.0, (name, u)
    print(f"irls batched, {iters} iterations, {len(refs)} pairs: max {worst:.3f} ulp")
