"""fp64 numpy restatements of the two pose solvers of ``csrc/pose.hip`` and the seeded cases the host and the GPU tests share.

``kabsch`` is ``rigid_transform_3d`` (scripts/SC2_PCR/common.py:7-45) and ``irls`` is ``est_quad_linear_robust``
(util/transform_estimation.py:89-116, after ``oracle/pose.py``): fp32 inputs widened exactly, every sum in float64, the 3x3
factorisation by ``numpy.linalg.svd`` and the 3n x 6 system by ``numpy.linalg.lstsq`` - neither method is the device's (Jacobi on
H^T H; 6x6 normal equations), so an error in the kernels' algebra cannot hide on both sides.

The bars of the GPU tests are stated here once (``ULP``, ``parity_ulps``, ``rotation_checks``): both sides compute in float64, so
the only fp32 rounding is the final store of T."""
import numpy as np

import _inputs as gi

ULP = 2.0 ** -23
T_TRUE = gi.rigid(0.02, -0.01, 0.12, 1.5, -0.4, 0.1)          # a small-angle pose: what the IRLS solver is for


def _f64(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x.astype(np.float64)


# ----------------------------------------------------------------------------- weighted Kabsch
def kabsch_terms(A, B, w=None, eps=1e-6):
    """-> ``ca [3], cb [3], H [3,3]`` of one problem: ``den = sum w + eps``, weighted centroids, ``H = sum w (a - ca)(b - cb)^T``."""
    A, B = _f64(A), _f64(B)
    w = np.ones(len(A)) if w is None else _f64(w).reshape(-1)
    den = w.sum() + eps
    ca, cb = (A * w[:, None]).sum(0) / den, (B * w[:, None]).sum(0) / den
    H = (A - ca).T @ (w[:, None] * (B - cb))
    return ca, cb, H


def rotation_from_H(H):
    """``H = U S V^T`` -> ``R = V diag(1, 1, det(V U^T)) U^T``, and S."""
    U, s, Vh = np.linalg.svd(H)
    V = Vh.T
    d = np.linalg.det(V @ U.T)
    return V @ np.diag([1.0, 1.0, d]) @ U.T, s


def kabsch(A, B, w=None, eps=1e-6):
    """One problem ``A, B f32 [n,3]``, ``w f32 [n]`` -> ``T f64 [4,4]`` with ``B ~ R A + t``, H and its singular values."""
    ca, cb, H = kabsch_terms(A, B, w, eps)
    R, s = rotation_from_H(H)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = cb - R @ ca
    return T, H, s


def kabsch_batch(A, B, w=None):
    """-> ``T f64 [bs,4,4]``, ``H [bs,3,3]``, ``s [bs,3]``."""
    out = [kabsch(A[b], B[b], None if w is None else w[b]) for b in range(len(A))]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def rotation_is_unique(H, s):
    """Where a matrix comparison means something: the second singular value carries the rotation about the first axis, and when the
    best orthogonal fit is a reflection the flipped axis must be the smallest one by a margin."""
    return bool(s[1] > 1e-2 * s[0] and (np.linalg.det(H) >= 0 or s[1] - s[2] > 1e-2 * s[0]))


# ----------------------------------------------------------------------------- IRLS small-angle solver
def _solve_lstsq(A, b):
    return np.linalg.lstsq(A, b, rcond=None)[0]


def _solve_normal(A, b):
    return np.linalg.solve(A.T @ A, A.T @ b)


def irls(p0, p1, w0, iters, idx1=None, solve=_solve_lstsq, halve=None):
    """``est_quad_linear_robust`` in float64 -> ``T f64 [4,4]``.  Row i pairs with ``p1[idx1[i]]`` (``p1[i]`` without ``idx1``); the rows of
    the linearised residual are ``[0, z, -y, 1, 0, 0]``, ``[-z, 0, x, 0, 1, 0]``, ``[y, -x, 0, 0, 0, 1]`` scaled by the weight; ``par`` halves
    at iterations 5, 10 and 15 and the weights of an iteration are ``par / (|r| + par)`` from the end of the one before."""
    cur, q = _f64(p0), _f64(p1)
    if idx1 is not None:
        q = q[np.asarray(idx1, np.int64)]
    n = len(cur)
    w = np.ones(n) if w0 is None else _f64(w0).reshape(-1)
    T, par = np.eye(4), 1.0
    o, l = np.zeros(n), np.ones(n)
    for i in range(iters):
        if (i > 0 and i % 5 == 0) if halve is None else i in halve:      # ``halve``: another schedule, for tests of the tests
            par /= 2.0
        x, y, z = cur[:, 0], cur[:, 1], cur[:, 2]
        A = np.concatenate([np.stack([o, z, -y, l, o, o], 1), np.stack([-z, o, x, o, l, o], 1), np.stack([y, -x, o, o, o, l], 1)])
        b = np.concatenate([q[:, 0] - x, q[:, 1] - y, q[:, 2] - z])
        w3 = np.tile(w, 3)
        sol = solve(A * w3[:, None], b * w3)
        Ti = np.eye(4)
        Ti[:3, :3] = gi.rot_zyx(sol[0], sol[1], sol[2])           # Euler Z . Y . X
        Ti[:3, 3] = sol[3:]
        cur = cur @ Ti[:3, :3].T + Ti[:3, 3]
        w = par / (np.linalg.norm(cur - q, axis=1) + par)
        T = Ti @ T
    return T


def irls_normal_equations(p0, p1, w0, iters, idx1=None):
    """The same loop, each step through the 6x6 normal equations in float64 (the device's method, numpy's solver)."""
    return irls(p0, p1, w0, iters, idx1, solve=_solve_normal)


# ----------------------------------------------------------------------------- the bars
def parity_ulps(T, T_ref):
    """max over entries of ``|T - T_ref| / (2^-23 max(1, |T_ref|))``: at most 1 when T is T_ref stored in fp32."""
    T, T_ref = np.asarray(T, np.float64), np.asarray(T_ref, np.float64)
    return float((np.abs(T - T_ref) / (ULP * np.maximum(1.0, np.abs(T_ref)))).max())


def rotation_checks(T, A, B, w):
    """The checks that hold whatever the geometry, for one problem -> dict of the realised figures over their bounds (each <= 1 passes):
    ``orth`` ``|R R^T - I| / (4 2^-23)``, ``det`` ``|det R - 1| / (4 2^-23)``, ``objective`` ``(tr(R_ref H) - tr(R H)) / (2^-24 sum |H_ij|)``
    - the first-order effect of storing R in fp32 -, and ``t`` ``|t - (cb - R ca)|`` over ``2^-23 max(1, |t|) + 2^-24 sum |ca_j|`` (t's own
    store, and R's store carried through ``R ca``).  H = 0 has no objective to miss: its figure is 0."""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    ca, cb, H = kabsch_terms(A, B, w)
    R_ref, _ = rotation_from_H(H)
    hsum = np.abs(H).sum()
    deficit = np.trace(R_ref @ H) - np.trace(R @ H)
    t_ref = cb - R @ ca
    return {"orth": float(np.abs(R @ R.T - np.eye(3)).max() / (4 * ULP)),
            "det": float(abs(np.linalg.det(R) - 1.0) / (4 * ULP)),
            "objective": float(deficit / (0.5 * ULP * hsum)) if hsum > 0 else 0.0,
            "t": float((np.abs(t - t_ref) / (ULP * np.maximum(1.0, np.abs(t_ref)) + 0.5 * ULP * np.abs(ca).sum())).max())}


# ----------------------------------------------------------------------------- Kabsch cases
KABSCH_WEIGHTS = ("none", "uniform", "zeros")
_NS = (3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)          # around a wave, around the 256-point kernel switch, block strides
_BS = (1, 2, 3, 5, 9)
# (n, bs, weights): every n with a batch that is no multiple of 4 (the wave kernel's early return), every batch size and every kind of
# weights on each side of n = 256; three points carry no weights (zeros among three would leave a line)
KABSCH_SHAPES = tuple((n, _BS[i % 5], KABSCH_WEIGHTS[i % 3]) for i, n in enumerate(_NS)) + ((256, 4, "uniform"), (257, 4, "zeros"))


def _poses(seed, bs):
    return [gi.rigid(*((gi._u(seed + 100 + b, 6) - 0.5) * np.array([0.6, 0.6, 2.0, 20, 20, 2]))) for b in range(bs)]


def _weights(seed, bs, n, kind):
    if kind == "none":
        return None
    w = 0.25 + 0.75 * gi._u(seed + 2, bs, n)
    if kind == "zeros":
        w[gi._u(seed + 3, bs, n) < 0.5] = 0.0
    return w.astype(np.float32)


def kabsch_shape_case(n, bs, kind, noise=0.05):
    """``A, B f32 [bs,n,3]``, ``w f32 [bs,n]`` or None: a 40 m box, a planted pose per problem, noise 0.05."""
    seed = 7000 + 13 * n + bs
    A = (gi._u(seed, bs, n, 3) - 0.5) * 40.0
    B = np.stack([A[b] @ T[:3, :3].T + T[:3, 3] for b, T in enumerate(_poses(seed, bs))]) + noise * gi._normal(seed + 1, bs, n, 3)
    return A.astype(np.float32), B.astype(np.float32), _weights(seed, bs, n, kind)


def kabsch_threshold_case(threshold=0.5):
    """Three problems of 65 points with weights U(0.25, 1) -> ``A, B, w`` and ``w`` with every entry under the threshold zeroed."""
    A, B, w = kabsch_shape_case(65, 3, "uniform")
    return A, B, w, np.where(w < np.float32(threshold), np.float32(0), w)


GEOMETRY_FAMILIES = ("mirrored", "planar", "planar_mirrored", "octahedron", "square", "near_collinear_1e-3", "near_collinear_1e-5",
                     "collinear", "all_equal", "zero_weights", "one_weight")
GEOMETRY_NS = (64, 320)                                               # the wave kernel and the block kernel
# the singular-value ratios a family must show (s2 / s1 and s3 / s1 as (low, high)); None = H is (numerically) zero
GEOMETRY_RATIOS = {"mirrored": ((0.3, 0.7), (0.08, 0.3)), "planar": ((0.3, 1.0), (0.0, 1e-12)), "planar_mirrored": ((0.3, 1.0), (0.0, 1e-12)),
                   "octahedron": ((1 - 1e-9, 1.0), (1 - 1e-9, 1.0)), "square": ((1 - 1e-9, 1.0), (0.0, 1e-12)),
                   "near_collinear_1e-3": ((3e-4, 3e-3), (0.0, 3e-3)), "near_collinear_1e-5": ((3e-6, 3e-5), (0.0, 3e-5)),
                   "collinear": ((0.0, 1e-12), (0.0, 1e-12)), "n2": ((0.0, 1e-12), (0.0, 1e-12))}


def _cycle(vertices, n):
    """n points: whole rounds of the vertices, the rest at their centre (no pull on the centroid, nothing added to H)."""
    v = np.asarray(vertices, np.float64)
    out = np.zeros((n, 3))
    k = (n // len(v)) * len(v)
    out[:k] = np.tile(v, (n // len(v), 1))
    return out


def kabsch_geometry_case(family, n):
    """One problem ``A, B f32 [n,3]``, ``w f32 [n]`` or None of a named degenerate (or merely special) geometry."""
    seed = 8000 + 17 * n + 101 * (GEOMETRY_FAMILIES + ("n1", "n2")).index(family)
    T = gi.rigid(0.2, -0.15, 0.7, 6.0, -3.0, 1.0)
    A = (gi._u(seed, n, 3) - 0.5) * 40.0
    w, noise, post = _weights(seed, 1, n, "uniform")[0], 0.05, None
    if family == "mirrored":
        A *= np.array([1.0, 0.7, 0.4])                               # distinct spreads: the axis to flip is the smallest by a margin
        post = 2
    elif family in ("planar", "planar_mirrored"):
        A[:, 2], noise = 0.0, 0.0
        post = 0 if family == "planar_mirrored" else None
    elif family == "octahedron":
        A, w, noise = _cycle([[8, 0, 0], [-8, 0, 0], [0, 8, 0], [0, -8, 0], [0, 0, 8], [0, 0, -8]], n), None, 0.0
        T = gi.rigid(0, 0, np.pi / 2, 4.0, -2.0, 1.0)                # a quarter turn and whole metres: B is exact
    elif family == "square":
        A, w, noise = _cycle([[8, 8, 0], [-8, 8, 0], [-8, -8, 0], [8, -8, 0]], n), None, 0.0
        T = gi.rigid(0, 0, np.pi / 2, 4.0, -2.0, 1.0)
    elif family.startswith("near_collinear"):
        # a singular value of H is a weighted variance: s2 / s1 = (spread across the line / spread along it)^2
        A[:, 1:] *= np.sqrt(float(family.split("_")[-1]))
        A, noise = A @ gi.rot_zyx(0.3, 0.5, -0.4).T, 0.0
    elif family == "collinear":
        A = np.round(A[:, :1] * 4) / 4 * np.array([[1.0, 2.0, -2.0]])
        T, noise = gi.rigid(0, 0, np.pi / 2, 4.0, -2.0, 1.0), 0.0
    elif family == "all_equal":
        A[:], noise = A[0], 0.0
    elif family == "zero_weights":
        w[:] = 0.0
    elif family == "one_weight":
        w[:] = 0.0
        w[n // 3] = 0.75
    elif family not in ("n1", "n2"):
        raise ValueError(family)
    R = np.round(T[:3, :3]) if noise == 0.0 and abs(T[0, 0]) < 1e-9 else T[:3, :3]       # the quarter turn without cos(pi/2)'s 6e-17
    B = A @ R.T + T[:3, 3] + noise * gi._normal(seed + 1, n, 3)
    if post is not None:
        B[:, post] = -B[:, post]
    return A.astype(np.float32), B.astype(np.float32), w


WEIGHT_SCALES = (40, 20, 0, -20, -40, -54, -60, -66, -100)
COORD_SCALES = (10, 0, -20, -40)
SCALE_NS = (20, 300)


def kabsch_scale_case(n):
    """One problem for the scale family: 40 m box, noise 0.05, weights U(0.25, 1) (to be multiplied by 2^e: exact, and normal in fp32
    down to e = -100)."""
    A, B, w = kabsch_shape_case(n, 1, "uniform")
    return A[0], B[0], w[0]


def pow2(x, k):
    """``x * 2^k`` exactly, in x's own type."""
    return np.ldexp(x, k).astype(x.dtype)


# ----------------------------------------------------------------------------- IRLS cases
IRLS_WEIGHTS = ("none", "uniform", "signed")
_IRLS_NS = (3, 4, 63, 64, 65, 1023, 1024, 1025, 2049)              # around a wave, around the 1024-row sweep, several sweeps
_IRLS_ITERS = (0, 1, 4, 5, 6, 10, 11, 15, 16, 20)                  # both sides of every halving of par


def _irls_cases():
    """(name, n, iters, inlier fraction, weights, far): the n sweep at 20 and 6 iterations, the iteration sweep at n = 1025, and clouds 800 m
    from the origin.  Three or four rows cannot have outliers and a pose: those keep every row an inlier."""
    out, k = [], 0
    for iters in (20, 6):
        for n in _IRLS_NS:
            out.append((f"n{n}_it{iters}", n, iters, 1.0 if n < 63 or k % 2 == 0 else 0.4, IRLS_WEIGHTS[k % 3], False))
            k += 1
    for iters in _IRLS_ITERS:
        out.append((f"sched_it{iters}", 1025, iters, 0.4 if k % 2 else 1.0, IRLS_WEIGHTS[k % 3], False))
        k += 1
    for n in (65, 1025):
        out.append((f"far_n{n}", n, 20, 0.4, IRLS_WEIGHTS[k % 3], True))
        k += 1
    return tuple(out)


IRLS_CASES = _irls_cases()


def irls_case(name):
    """-> ``p0, p1 f32 [n,3]``, ``w0 f32 [n]`` or None, iters."""
    i = [c[0] for c in IRLS_CASES].index(name)
    _, n, iters, frac, kind, far = IRLS_CASES[i]
    seed = 9000 + 10 * i
    p0, p1, _ = gi.corr_case(seed, n, T_TRUE, frac)
    if far:                                                          # fp32 coordinates 800 m out: 6e-5 m apart, the solver stays fp64
        off = np.array([560.0, -560.0, 80.0])
        p0 = (p0.astype(np.float64) + off).astype(np.float32)
        p1 = (p1.astype(np.float64) + T_TRUE[:3, :3] @ off).astype(np.float32)
    w = None
    if kind == "uniform":
        w = (0.05 + 0.95 * gi._u(seed + 9, n)).astype(np.float32)
    elif kind == "signed":                                           # pose_estimation's weight is a maximal inner product: any sign, only w^2 enters
        w = (2.0 * gi._u(seed + 9, n) - 1.0).astype(np.float32)
        if n > 4:
            w[gi._u(seed + 8, n) < 0.25] = 0.0
            w[:3] = (0.9, -0.8, 0.7)                                 # three rows that always count
    return p0, p1, w, iters


def irls_gather_layout(p1, seed, extra):
    """A p1 segment longer than the correspondence list: the rows of ``p1`` shuffled among ``extra`` unmatched ones -> ``p1_seg, idx1`` with
    ``p1_seg[idx1] == p1``."""
    n = len(p1)
    rng = np.random.default_rng(seed)
    rows = np.concatenate([p1, rng.uniform(-30, 30, (extra, 3)).astype(np.float32)])
    perm = rng.permutation(n + extra)
    idx1 = np.argsort(perm)[:n]
    return rows[perm], idx1.astype(np.int64)


def irls_repeat_case(seed, n0, n1):
    """More correspondences than target rows, so ``idx1`` repeats: ``p0 [n0,3]`` are noisy pre-images of ``p1[idx1]`` -> ``p0, p1, idx1``."""
    rng = np.random.default_rng(seed)
    p1 = rng.uniform(-30, 30, (n1, 3))
    idx1 = rng.integers(0, n1, n0)
    Tinv = np.linalg.inv(T_TRUE)
    p0 = p1[idx1] @ Tinv[:3, :3].T + Tinv[:3, 3] + 0.02 * rng.standard_normal((n0, 3))
    assert len(np.unique(idx1)) < n0
    return p0.astype(np.float32), p1.astype(np.float32), idx1.astype(np.int64)
