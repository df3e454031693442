"""SC2-PCR stage by stage in fp64, and one checker per stage of ``csrc/sc2pcr.hip``.  TEST INFRASTRUCTURE, numpy; imports nothing
from ``eyoc_amd`` (torch and ``oracle`` only inside the three functions that run the fp32 oracle).

Written from ``oracle/sc2pcr.py`` and the reference lines it cites (scripts/SC2_PCR/SC2_PCR.py:307-384 ``SC2_PCR``, :170-196
``cal_leading_eigenvector``, :33-59 ``pick_seeds``, :61-168 ``cal_seed_trans``, :238-278 ``post_refinement``;
scripts/SC2_PCR/common.py:7-45 ``rigid_transform_3d``), not from the kernels.  Coordinates are fp32 values and exact in fp64; the
thresholds are the fp32 parameters the library call receives.

A *dump* is a dict of numpy arrays named like the workspace buffers of ``eyoc_sc2pcr`` (``include/eyoc_hip.h``,
``eyoc_sc2pcr_workspace_layout``): ``src tgt v dom score rank seeds hard tight ptr_h col_h val_h cnt blk_dense knn seed_h Ts fitness
T`` plus ``ctl`` (a dict: ``converged iters best_seed best_fitness norm dense``), the plan's integers ``n words n_seed k1 k2
csr_cap`` and ``params``.  Bit matrices are ``uint64 [n, words]``, bit b of word w = column 64 w + b.

Every checker takes the dump's OWN output of the previous stage as its input, so each comparison is exact or has a derivable band
and a near-tie in one stage cannot cascade into the next.  The band of a length comparison: three coordinate differences at
relative 2^-24 each, one rounded product and two fused multiply-adds, a correctly rounded root, one rounded difference - below
7 * 2^-24 * the longer length; 8 is used.  A checker raises ``AssertionError`` and returns a dict of the quantities it realised.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -24
BAND = 8 * U

KITTI = dict(inlier_threshold=0.6, d_thre=0.1, ratio=0.2, nms_radius=0.6, num_iterations=20, k1=30, k2=20)
TDM = dict(inlier_threshold=0.10, d_thre=0.1, ratio=0.1, nms_radius=0.10, num_iterations=10, k1=30, k2=20)   # 3DMatch-like

STAGES = ("masks", "csr", "eigenvector", "nms", "seeds", "second_order", "local", "poses", "fitness", "final")

# caps on what a band may leave undecided (conditions on the inputs: a checker that excuses more than this hides failures)
CAP_MASK_UNDECIDED = 2e-4      # of n^2, per matrix
CAP_NMS_ROWS = 1e-3            # of n
CAP_FRAGILE = 0.01             # of n_seed
CAP_ILL = 0.01                 # of n_seed
MIN_SINGLE_FITNESS = 0.95      # of n_seed: fitness interval is one integer


def f32(x):
    return float(np.float32(x))


def plan(n, p):
    """The integers of the library's plan (make_plan): words, n_seed = int(ratio n), k1 = k2 = 4 when k1 > n, csr_cap."""
    k1, k2 = (4, 4) if p["k1"] > n else (p["k1"], p["k2"])
    return dict(n=n, words=(n + 63) // 64, n_seed=int(n * p["ratio"]), k1=k1, k2=k2, csr_cap=n * n // 4 + 64)


# ----------------------------------------------------------------------------- inputs of the stage tests
def _corr(gi, seed, n, frac, noise):
    return gi.corr_case(seed, n, gi.rigid(0.02, -0.01, 0.1, 4.0, 0.3, -0.2), frac, noise=noise)[:2]


def case_input(name, gi, golden=None):
    """-> (src f32 [n,3], tgt f32 [n,3], params).  ``gi`` = tests/golden/_inputs.py; ``golden`` = the loaded g4_sc2pcr.npz (golden*)."""
    import json
    if name.startswith("golden"):
        seed, n, frac, tp = json.loads(str(golden["cases"]))[int(name[6:])]
        p0, p1, _ = gi.corr_case(seed, n, gi.rigid(*tp), frac, noise=0.03)
        return p0, p1, dict(KITTI)
    if name == "exact":            # thousands of equal counts and equal scores: every tie rule at once
        return (*_corr(gi, 730, 3000, 0.6, 0.0), dict(KITTI))
    if name == "dup":              # what match_pair's resampling produces: 37 % duplicated rows, cross lengths of exactly 0, equal v
        p0, p1 = _corr(gi, 731, 5000, 0.25, 0.03)
        sel = np.random.default_rng(1).choice(5000, 8000)
        return p0[sel], p1[sel], dict(KITTI)
    if name == "n20":              # k1 > n: k1 = k2 = 4
        return (*gi.corr_case(81, 20, gi.rigid(0.01, 0.0, 0.08, 3.0, 0.2, 0.0), 1.0, noise=0.01)[:2], dict(KITTI))
    if name == "n65":
        return (*_corr(gi, 732, 65, 0.5, 0.01), dict(KITTI))
    if name == "n777":
        return (*_corr(gi, 733, 777, 0.4, 0.02), dict(KITTI))
    if name == "n4097":            # 65 words
        return (*_corr(gi, 734, 4097, 0.2, 0.03), dict(KITTI))
    if name == "n8193":            # 129 words: the 64-words-per-wave dense count kernel
        return (*_corr(gi, 735, 8193, 0.15, 0.03), dict(KITTI))
    if name == "tdm":              # inlier_threshold = 0.10: the 0.10 m refinement branch.  Noise 0.01: at 0.03 the inliers' residuals
        # (~0.05 m) are dense around the 0.10 m threshold and 7 % of the seeds have one inside its band - found with the fp32 oracle alone
        return (*_corr(gi, 736, 2000, 0.3, 0.01), dict(TDM))
    if name == "scaled":           # coordinates x 1e4 WITH the three lengths of the parameter set: wide bands, same geometry
        p0, p1 = _corr(gi, 737, 2000, 0.3, 0.03)
        s = np.float32(1.0e4)
        return p0 * s, p1 * s, dict(KITTI, d_thre=0.1 * 1e4, nms_radius=0.6 * 1e4, inlier_threshold=0.6 * 1e4)
    raise KeyError(name)


GPU_CASES = ("golden0", "golden1", "golden2", "golden3", "exact", "dup", "n20", "n65", "n777", "n4097", "n8193", "tdm", "scaled")
HOST_CASES = ("golden0", "golden1", "golden2", "golden3", "exact", "n20", "n65", "n777", "tdm", "scaled")      # n <= 3000


# ----------------------------------------------------------------------------- bits
def pack_bits(B, words):
    by = np.packbits(np.asarray(B, bool), axis=1, bitorder="little")
    out = np.zeros((B.shape[0], words * 8), np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8")


def unpack_bits(W, n=None):
    B = np.unpackbits(np.ascontiguousarray(W).view(np.uint8), axis=1, bitorder="little")
    return (B if n is None else B[:, :n]).astype(bool)


def popcount(W):
    return np.bitwise_count(W)


def _rows_per_chunk(n, budget=1 << 21):
    return max(1, budget // max(n, 1))


def _lens(P, r0, r1):
    d = P[r0:r1, None, :] - P[None, :, :]
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


# ----------------------------------------------------------------------------- the restatement of an input (cached by the tests)
class FirstOrder:
    """fp64 first-order stage of one input: both masks, which of their entries lie inside the band, the soft matrix
    ``max(0, 1 - c^2 / d^2)`` as a sparse fp64 matrix (its support is c < d), and the power iterates (every one kept)."""

    def __init__(self, src, tgt, p):
        self.src, self.tgt, self.p = np.asarray(src, np.float64), np.asarray(tgt, np.float64), p
        n = self.n = len(src)
        self.words = (n + 63) // 64
        d = self.d = f32(p["d_thre"])
        dh = self.dh = f32(np.float32(0.5) * np.float32(p["d_thre"]))
        H, T, UH, UT, rows, cols, vals = [], [], [], [], [], [], []
        step = _rows_per_chunk(n)
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            ls, lt = _lens(self.src, r0, r1), _lens(self.tgt, r0, r1)
            c = np.abs(ls - lt)
            band = BAND * np.maximum(ls, lt)
            hb = c < d
            H.append(pack_bits(hb, self.words)); T.append(pack_bits(c < dh, self.words))
            UH.append(pack_bits(np.abs(c - d) <= band, self.words)); UT.append(pack_bits(np.abs(c - dh) <= band, self.words))
            i, j = np.nonzero(hb)
            rows.append(i + r0); cols.append(j); vals.append(1.0 - c[i, j] ** 2 / d ** 2)
        self.hard, self.tight, self.und_hard, self.und_tight = (np.concatenate(x) for x in (H, T, UH, UT))
        self.M = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
        self._it = None

    def iterates(self):
        """-> (list v_0 .. v_K with K = num_iterations, iters): SC2_PCR.py:170-196 - from all-ones, v <- M v / (|M v| + 1e-6), stop
        after the sweep whose result is allclose (torch defaults) to the previous one; ``iters`` = sweeps the loop applies.  The
        iterates beyond it are kept too, so that an implementation that stops one sweep later has something to be compared with."""
        if self._it is None:
            self._it = power_iterates64(self.M, int(self.p["num_iterations"]))
        return self._it


def power_iterates64(M, K):
    v = np.ones(M.shape[0])
    its, iters = [v], None
    for k in range(1, K + 1):
        y = M @ v
        nv = y / (np.sqrt((y * y).sum()) + 1e-6)
        if iters is None and np.all(np.abs(nv - v) <= 1e-8 + 1e-5 * np.abs(v)):
            iters = k
        its.append(nv)
        v = nv
    return its, K if iters is None else iters


def cross_of_pairs(src, tgt, i, j):
    """fp64 cross length and its band for index pairs."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    ls = np.sqrt(((src[i] - src[j]) ** 2).sum(-1))
    lt = np.sqrt(((tgt[i] - tgt[j]) ** 2).sum(-1))
    return np.abs(ls - lt), BAND * np.maximum(ls, lt)


def kabsch64(ca, cb, H):
    """common.py:7-45 from centroids and cross-covariance: R = V diag(1, 1, det(V U^T)) U^T, t = cb - R ca (batched) -> R, t, singular values."""
    Uu, S, Vh = np.linalg.svd(H)
    V, Ut = np.swapaxes(Vh, -1, -2), np.swapaxes(Uu, -1, -2)
    D = np.zeros_like(H)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = np.linalg.det(V @ Ut)
    R = V @ D @ Ut
    return R, cb - np.einsum("...ij,...j->...i", R, ca), S


def kabsch_terms64(A, B, w):
    """Weighted centroids (1e-6 in the denominator) and H = (A - ca)^T diag(w) (B - cb), batched over the leading axis."""
    den = w.sum(-1)[..., None] + 1e-6
    ca = (A * w[..., None]).sum(-2) / den
    cb = (B * w[..., None]).sum(-2) / den
    H = np.einsum("...ni,...nj->...ij", A - ca[..., None, :], w[..., None] * (B - cb[..., None, :]))
    return ca, cb, H


def local_stage64(src, tgt, knn, p, k2):
    """SC2_PCR.py:61-168 up to the weighted Kabsch terms, from the seeds' k1 neighbours: local hard matrix, its first row times the
    matrix, stable top-k2, soft matrix with zero diagonal, power iteration, w / (sum w + 1e-6).
    -> (seed_h f64 [S, 15] = centroid a, centroid b, H row-major;  fragile bool [S]: a local cross length within its band of d).
    The reference iterates the whole batch of seeds until ALL of them are allclose (one ``torch.allclose`` over [S, k2]); a seed
    that stops on its own, as the device's do, is within the 1e-5 of allclose of that."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    d = f32(p["d_thre"])
    S, k1 = knn.shape
    s1, t1 = src[knn], tgt[knn]                                                   # [S, k1, 3]
    loc = lambda P: np.sqrt(((P[:, :, None, :] - P[:, None, :, :]) ** 2).sum(-1))
    ls, lt = loc(s1), loc(t1)
    c = np.abs(ls - lt)
    fragile = (np.abs(c - d) <= BAND * np.maximum(ls, lt)).any((1, 2))
    hard = (c < d).astype(np.float64)
    sc2 = np.einsum("sa,saj->sj", hard[:, 0, :], hard)
    nn2 = np.argsort(-sc2, axis=1, kind="stable")[:, :k2]
    s2, t2 = np.take_along_axis(s1, nn2[..., None], 1), np.take_along_axis(t1, nn2[..., None], 1)
    c2 = np.abs(loc(s2) - loc(t2))
    soft = np.maximum(1.0 - c2 ** 2 / d ** 2, 0.0)
    ar = np.arange(k2)
    soft[:, ar, ar] = 0.0
    v = np.ones((S, k2))
    for _ in range(int(p["num_iterations"])):
        y = np.einsum("sab,sb->sa", soft, v)
        last, v = v, y / (np.sqrt((y * y).sum(1, keepdims=True)) + 1e-6)
        if np.all(np.abs(v - last) <= 1e-8 + 1e-5 * np.abs(last)):
            break
    w = v / (v.sum(1, keepdims=True) + 1e-6)
    ca, cb, H = kabsch_terms64(s2, t2, w)
    return np.concatenate([ca, cb, H.reshape(S, 9)], 1), fragile


def oracle_seed_h(src, tgt, knn, p, k2):
    """The local stage of the fp32 torch oracle on GIVEN neighbour lists -> seed_h f64 [S, 15] holding its fp32 values."""
    import torch
    from oracle import sc2pcr as osc
    from oracle.pose import kabsch_terms
    m = osc.Matcher(d_thre=p["d_thre"], num_iterations=p["num_iterations"])
    ts, tt = torch.from_numpy(np.asarray(src, np.float32))[None], torch.from_numpy(np.asarray(tgt, np.float32))[None]
    s2, t2, w = m.local_consensus(torch.from_numpy(np.asarray(knn, np.int64))[None], ts, tt, k2)
    cA, cB, H = kabsch_terms(s2.reshape(-1, k2, 3), t2.reshape(-1, k2, 3), w)
    return torch.cat([cA[:, 0], cB[:, 0], H.reshape(-1, 9)], 1).numpy().astype(np.float64)


def seed_h_error(got, want):
    """max |a - b| / max |b| for the three groups of seed_h (centroid a, centroid b, H) -> the largest of the three."""
    e = 0.0
    for sl in (slice(0, 3), slice(3, 6), slice(6, 15)):
        if want[:, sl].size:
            e = max(e, float(np.abs(got[:, sl] - want[:, sl]).max() / max(np.abs(want[:, sl]).max(), 1e-300)))
    return e


def refine64(T, src, tgt, p, it_num=20):
    """SC2_PCR.py:238-278: inliers under 0.10 m (inlier_threshold == 0.10) or 1.2 m, Cauchy weights, Kabsch; stop when the count repeats."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    thr = f32(0.10) if np.float32(p["inlier_threshold"]) == np.float32(0.10) else f32(1.2)
    T = np.array(T, np.float64)
    prev = 0
    for _ in range(it_num):
        dist = np.sqrt((((src @ T[:3, :3].T + T[:3, 3]) - tgt) ** 2).sum(1))
        inl = dist < thr
        if abs(int(inl.sum()) - prev) < 1:
            break
        prev = int(inl.sum())
        ca, cb, H = kabsch_terms64(src[inl], tgt[inl], 1.0 / (1.0 + (dist[inl] / thr) ** 2))
        R, t, _ = kabsch64(ca, cb, H)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
    return T


def second_order_counts(hard, tight, seed):
    """popcount(tight[seed] & tight[j]) * hard[seed][j] for every j (int64 [64 words]); only the hard row's set bits are visited."""
    cand = np.nonzero(unpack_bits(hard[seed:seed + 1])[0])[0]
    out = np.zeros(hard.shape[1] * 64, np.int64)
    out[cand] = popcount(tight[seed][None, :] & tight[cand]).sum(1)
    return out


def chain64(src, tgt, p, fo=None):
    """All stages in fp64, each fed by the one before (``Matcher.SC2_PCR``) -> (T [4,4], seed-wise fitness, v)."""
    fo = fo or FirstOrder(src, tgt, p)
    n, P = fo.n, plan(fo.n, p)
    its, it = fo.iterates()
    v = its[it]
    dom, R, step = np.zeros(n, bool), f32(p["nms_radius"]), _rows_per_chunk(n)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        dom[r0:r1] = ((v[None, :] > v[r0:r1, None]) & (_lens(fo.src, r0, r1) < R)).any(1)
    seeds = np.argsort(-np.where(dom, 0.0, v), kind="stable")[:P["n_seed"]]
    knn = np.stack([np.argsort(-second_order_counts(fo.hard, fo.tight, int(sd))[:n], kind="stable")[:P["k1"]] for sd in seeds])
    h, _ = local_stage64(src, tgt, knn, p, P["k2"])
    Rs, ts, _ = kabsch64(h[:, 0:3], h[:, 3:6], h[:, 6:15].reshape(-1, 3, 3))
    r = np.sqrt(((np.einsum("sij,nj->sni", Rs, fo.src) + ts[:, None, :] - fo.tgt[None]) ** 2).sum(-1))
    fitness = (r < f32(p["inlier_threshold"])).sum(1)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rs[np.argmax(fitness)], ts[np.argmax(fitness)]
    return refine64(T, src, tgt, p), fitness, v


# ----------------------------------------------------------------------------- the checkers
def check_masks(D, fo):
    n, words = D["n"], D["words"]
    stats = {}
    for name, ref, und, in (("hard", fo.hard, fo.und_hard), ("tight", fo.tight, fo.und_tight)):
        dev = D[name]
        assert dev.shape == (n, words) and dev.dtype == np.uint64, f"masks: {name} shape {dev.shape}"
        B = unpack_bits(dev)
        assert not B[:, n:].any(), f"masks: {name} has bits set at columns >= n"
        B = B[:, :n]
        assert B.diagonal().all(), f"masks: {name} diagonal not set"
        asym = np.argwhere(B != B.T)
        assert len(asym) == 0, f"masks: {name} not symmetric at {asym[:4].tolist()}"
        wrong = (dev ^ ref) & ~und
        if wrong.any():
            ij = np.argwhere(unpack_bits(wrong))
            raise AssertionError(f"masks: {name} differs from the fp64 decision outside the band at {len(ij)} entries, first {ij[:4].tolist()}")
        frac = float(popcount(und).sum()) / (n * n)
        assert frac <= CAP_MASK_UNDECIDED, f"masks: {name} undecided fraction {frac:.2e} above the cap"
        stats[f"undecided_{name}"] = frac
    return stats


def check_csr(D):
    n, hard, ctl = D["n"], D["hard"], D["ctl"]
    deg = popcount(hard).sum(1).astype(np.int64)
    nnz = int(deg.sum())
    assert bool(ctl["dense"]) == (nnz > D["csr_cap"]), f"csr: dense {ctl['dense']} but nnz {nnz}, cap {D['csr_cap']}"
    if ctl["dense"]:
        return dict(nnz=nnz, dense=1)
    ptr = np.concatenate([[0], np.cumsum(deg)])
    assert np.array_equal(D["ptr_h"][:n + 1], ptr), "csr: ptr_h is not the exclusive scan of the row popcounts"
    i, j = np.nonzero(unpack_bits(hard, n))                 # row-major: columns ascending within a row - the order the kernel promises
    assert np.array_equal(D["col_h"][:nnz].astype(np.int64), j), "csr: col_h is not the ascending column list of the hard rows"
    d = f32(D["params"]["d_thre"])
    worst = 0.0
    for a in range(0, nnz, 1 << 21):
        b = min(nnz, a + (1 << 21))
        c, band = cross_of_pairs(D["src"], D["tgt"], i[a:b], j[a:b])
        want = np.maximum(0.0, 1.0 - c * c / (d * d))
        tol = 2.0 * c * band / (d * d) + 4 * U
        err = np.abs(D["val_h"][a:b].astype(np.float64) - want)
        bad = np.nonzero(err > tol)[0]
        assert len(bad) == 0, f"csr: val_h off at entry {a + bad[0]}: {D['val_h'][a + bad[0]]} vs {want[bad[0]]} (tol {tol[bad[0]]:.2e})"
        worst = max(worst, float((err / tol).max()))
    return dict(nnz=nnz, dense=0, val_err_over_tol=worst)


def check_eigenvector(D, fo, tol):
    ctl, K = D["ctl"], int(D["params"]["num_iterations"])
    its, iters64 = fo.iterates()
    it = int(ctl["iters"])
    assert 1 <= it <= K and abs(it - iters64) <= 1, f"eigenvector: {it} sweeps, fp64 takes {iters64} (of at most {K})"
    assert ctl["converged"] in (0, 1), "eigenvector: converged flag"
    if it < K:
        assert ctl["converged"] == 1, f"eigenvector: stopped after {it} of {K} sweeps without converged"
    want = its[it]
    err = float(np.abs(D["v"].astype(np.float64) - want).max() / np.abs(want).max())
    assert err <= tol, f"eigenvector: v differs from fp64 iterate {it} by {err:.2e} (relative to max |v|), tolerance {tol:.2e}"
    return dict(iters=it, iters64=iters64, v_err=err)


def check_nms(D):
    n, R = D["n"], f32(D["params"]["nms_radius"])
    src, v = np.asarray(D["src"], np.float64), D["v"].astype(np.float64)
    sure, maybe = np.zeros(n, bool), np.zeros(n, bool)
    step = _rows_per_chunk(n)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        L = _lens(src, r0, r1)
        gt = v[None, :] > v[r0:r1, None]
        sure[r0:r1] = (gt & (L < R - BAND * L)).any(1)
        maybe[r0:r1] = (gt & (L < R + BAND * L)).any(1)
    dom = D["dom"] != 0
    bad = np.nonzero((sure & ~dom) | (~maybe & dom))[0]
    assert len(bad) == 0, f"nms: dom wrong for {len(bad)} rows, first {bad[:4].tolist()}"
    und = int((maybe & ~sure).sum())
    assert und <= CAP_NMS_ROWS * n, f"nms: {und} rows with only in-band dominators"
    want = np.where(dom, np.float32(0), D["v"])
    assert np.array_equal(D["score"].view(np.uint32), want.view(np.uint32)), "nms: score is not (dom ? 0 : v)"
    return dict(nms_undecided_rows=und, survivors=int((~dom).sum()))


def check_seeds(D):
    n, n_seed = D["n"], D["n_seed"]
    order = np.argsort(-D["score"].astype(np.float64), kind="stable")
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    bad = np.nonzero(D["rank"] != rank)[0]
    assert len(bad) == 0, f"seeds: rank wrong at {bad[:4].tolist()}"
    bad = np.nonzero(D["seeds"][:n_seed] != order[:n_seed])[0]
    assert len(bad) == 0, f"seeds: seed list wrong at positions {bad[:4].tolist()}"
    return dict(zero_score_seeds=int((D["score"][order[:n_seed]] == 0).sum()))


def check_second_order(D):
    n, hard, tight = D["n"], D["hard"], D["tight"]
    k1 = plan(n, D["params"])["k1"]
    assert D["knn"].shape[1] == k1, f"second_order: {D['knn'].shape[1]} neighbours per seed, the parameters ask for {k1}"
    ties = 0
    for s, seed in enumerate(D["seeds"][:D["n_seed"]]):
        cnt = second_order_counts(hard, tight, int(seed))
        srt = np.argsort(-cnt[:n], kind="stable")
        want = srt[:k1]
        assert np.array_equal(D["knn"][s], want), f"second_order: knn of seed {s} (row {seed}) is {D['knn'][s].tolist()}, stable top-k1 is {want.tolist()}"
        ties += int(k1 < n and cnt[srt[k1]] == cnt[srt[k1 - 1]])
        if D["blk_dense"][s >> 6]:
            assert np.array_equal(D["cnt"][s].astype(np.int64), cnt), f"second_order: cnt row of seed {s} differs from the counts"
    return dict(seeds_with_tie_at_k1=ties)


def check_local(D):
    """The tolerance is ``tolerance()`` of the fp32 oracle's own error on the SAME neighbour lists (the stage's input, taken from the dump)."""
    S = D["n_seed"]
    knn = D["knn"][:S].astype(np.int64)
    want, fragile = local_stage64(D["src"], D["tgt"], knn, D["params"], D["k2"])
    assert fragile.sum() <= CAP_FRAGILE * S, f"local: {int(fragile.sum())} fragile seeds of {S}"
    ok = ~fragile
    oracle_err = seed_h_error(oracle_seed_h(D["src"], D["tgt"], knn, D["params"], D["k2"])[ok], want[ok])
    err = seed_h_error(D["seed_h"][:S][ok, :15], want[ok])
    assert err <= tolerance(oracle_err), (f"local: seed_h differs from fp64 by {err:.2e} (per group, relative to its max), the fp32 oracle "
                                          f"by {oracle_err:.2e}: tolerance {tolerance(oracle_err):.2e}")
    return dict(fragile=int(fragile.sum()), seed_h_err=err, oracle_seed_h_err=oracle_err)


def check_poses(D):
    S = D["n_seed"]
    h = D["seed_h"][:S]
    R, t, sv = kabsch64(h[:, 0:3], h[:, 3:6], h[:, 6:15].reshape(S, 3, 3))
    Ts = D["Ts"][:S].astype(np.float64).reshape(S, 4, 4)
    det = np.linalg.det(Ts[:, :3, :3])
    bad = np.nonzero(~(np.abs(det - 1.0) <= 1e-6))[0]
    assert len(bad) == 0, f"poses: det R = {det[bad[0]]} for seed {bad[0]}"
    assert np.array_equal(Ts[:, 3], np.tile([0.0, 0, 0, 1], (S, 1))), "poses: last row is not (0, 0, 0, 1)"
    well = sv[:, 1] > 1e-3 * sv[:, 0]
    assert (~well).sum() <= CAP_ILL * S, f"poses: {int((~well).sum())} ill-conditioned seeds of {S}"
    eR = np.abs(Ts[:, :3, :3] - R).max((1, 2))
    et = np.abs(Ts[:, :3, 3] - t).max(1) / np.maximum(1.0, np.abs(t).max(1))
    bad = np.nonzero(well & ((eR > 4 * U) | (et > 4 * U)))[0]
    assert len(bad) == 0, f"poses: seed {bad[0]} rotation off by {eR[bad[0]]:.2e}, translation by {et[bad[0]]:.2e} (relative), bound {4 * U:.2e}"
    return dict(ill_conditioned=int((~well).sum()), R_err=float(eR[well].max(initial=0)), t_err=float(et[well].max(initial=0)))


def check_fitness(D):
    S, n = D["n_seed"], D["n"]
    thr = f32(D["params"]["inlier_threshold"])
    src, tgt = np.asarray(D["src"], np.float64), np.asarray(D["tgt"], np.float64)
    Ts = D["Ts"][:S].astype(np.float64).reshape(S, 4, 4)
    l1 = np.abs(src).sum(1) + np.abs(tgt).sum(1)
    lo, hi = np.zeros(S, np.int64), np.zeros(S, np.int64)
    step = _rows_per_chunk(n)
    for a in range(0, S, step):
        b = min(S, a + step)
        r = np.sqrt(((np.einsum("sij,nj->sni", Ts[a:b, :3, :3], src) + Ts[a:b, None, :3, 3] - tgt[None]) ** 2).sum(-1))
        band = BAND * (l1[None, :] + np.abs(Ts[a:b, :3, 3]).sum(1)[:, None])
        lo[a:b], hi[a:b] = (r < thr - band).sum(1), (r < thr + band).sum(1)
    f = D["fitness"][:S].astype(np.float64)
    bad = np.nonzero((f < lo) | (f > hi) | (f != np.round(f)))[0]
    assert len(bad) == 0, f"fitness: seed {bad[0]} has {f[bad[0]]}, fp64 interval [{lo[bad[0]]}, {hi[bad[0]]}]"
    single = float((lo == hi).mean())
    assert single >= MIN_SINGLE_FITNESS, f"fitness: only {single:.3f} of the seeds have a one-integer interval"
    return dict(single_interval=single)


def check_final(D):
    S = D["n_seed"]
    f = D["fitness"][:S]
    best = int(np.argmax(f))
    assert int(D["ctl"]["best_seed"]) == best, f"final: best_seed {D['ctl']['best_seed']}, first maximum is {best}"
    assert float(D["ctl"]["best_fitness"]) == float(f[best]), "final: best_fitness"
    T0 = np.eye(4)
    T0[:3] = D["Ts"][best].astype(np.float64).reshape(4, 4)[:3]
    want = refine64(T0, D["src"], D["tgt"], D["params"])
    err = float(np.abs(np.asarray(D["T"], np.float64).reshape(4, 4) - want).max())
    assert err <= 1e-4, f"final: T differs from the fp64 refinement of the device's best hypothesis by {err:.2e}"
    return dict(T_err=err)


def run_all(D, fo, tol_v):
    """Every checker on one dump -> {stage: stats dict, or the AssertionError's text}."""
    fns = dict(masks=lambda: check_masks(D, fo), csr=lambda: check_csr(D), eigenvector=lambda: check_eigenvector(D, fo, tol_v),
               nms=lambda: check_nms(D), seeds=lambda: check_seeds(D), second_order=lambda: check_second_order(D),
               local=lambda: check_local(D), poses=lambda: check_poses(D), fitness=lambda: check_fitness(D),
               final=lambda: check_final(D))
    out = {}
    for st in STAGES:
        try:
            out[st] = fns[st]()
        except AssertionError as e:
            out[st] = str(e)
    return out


def failed(res):
    return [st for st in STAGES if isinstance(res[st], str)]


def oracle_v_error(fo, src, tgt, p):
    """The fp32 torch oracle's leading eigenvector against the fp64 iterate of the same number: max |a - b| / max |b|."""
    import torch
    from oracle import sc2pcr as osc
    m = osc.Matcher(d_thre=p["d_thre"], num_iterations=p["num_iterations"])
    ts, tt = torch.from_numpy(np.asarray(src, np.float32))[None], torch.from_numpy(np.asarray(tgt, np.float32))[None]
    cross = torch.abs(osc.pairwise_len(ts) - osc.pairwise_len(tt))
    v = m.cal_leading_eigenvector(torch.clamp(1.0 - cross ** 2 / m.d_thre ** 2, min=0))[0].numpy().astype(np.float64)
    want = fo.iterates()[0][m._sweeps]
    return float(np.abs(v - want).max() / np.abs(want).max())


def tolerance(oracle_err):
    """What the device gets for a quantity whose error depends on the input's spectral gap: 4 x the fp32 oracle's own error against
    fp64 (two independent fp32 evaluation orders can sit on opposite sides of the fp64 value, times two for the data-dependent
    summation order), never less than 16 * 2^-24."""
    return max(4.0 * oracle_err, 16 * U)


# ----------------------------------------------------------------------------- a dump from the workspace bytes
def dump_from_workspace(ws, L, src, tgt, p, fitness, T):
    """``ws`` uint8 [>= L.total] = one pair's workspace slice copied back; ``L`` = eyoc_sc2pcr_layout (attributes)."""
    n, words, S, k1 = L.n, L.words, L.n_seed, L.k1
    take = lambda off, dtype, count: np.frombuffer(ws, dtype, int(count), int(off)).copy()
    c = take(L.off_ctl, np.int32, 8)
    ctl = dict(converged=int(c[0]), iters=int(c[1]), best_seed=int(c[2]), best_fitness=float(c[3:4].view(np.float32)[0]),
               norm=float(c[4:5].view(np.float32)[0]), dense=int(c[5]))
    ptr = take(L.off_ptr_h, np.int32, n + 1)
    nnz = 0 if ctl["dense"] else int(ptr[n])
    return dict(src=np.asarray(src, np.float32), tgt=np.asarray(tgt, np.float32), params=p, n=n, words=words, n_seed=S, k1=k1, k2=L.k2,
                csr_cap=int(L.csr_cap), ctl=ctl, v=take(L.off_v, np.float32, n), score=take(L.off_score, np.float32, n),
                seeds=take(L.off_seeds, np.int32, S), hard=take(L.off_hard, np.uint64, n * words).reshape(n, words),
                tight=take(L.off_tight, np.uint64, n * words).reshape(n, words), knn=take(L.off_knn, np.int32, S * k1).reshape(S, k1),
                Ts=take(L.off_Ts, np.float32, S * 16).reshape(S, 16), dom=take(L.off_dom, np.int32, n),
                rank=take(L.off_rank, np.int32, n), ptr_h=ptr, col_h=take(L.off_col_h, np.uint16, nnz),
                val_h=take(L.off_val_h, np.float32, nnz), cnt=take(L.off_cnt, np.uint16, S * words * 64).reshape(S, words * 64),
                blk_dense=take(L.off_blk_dense, np.uint8, (S + 63) // 64), seed_h=take(L.off_seed_h, np.float64, S * 16).reshape(S, 16),
                fitness=np.asarray(fitness, np.float32)[:S].copy(), T=np.asarray(T, np.float32).reshape(4, 4).copy())


# buffers of a dump that two runs of the same pair must agree on byte for byte (y is scratch; seed_h column 15 is never written)
DUMP_BUFFERS = ("v", "score", "seeds", "hard", "tight", "knn", "Ts", "dom", "rank", "ptr_h", "col_h", "val_h", "cnt", "blk_dense",
                "fitness", "T")


def dumps_equal(A, B):
    """-> names of the buffers (and ctl fields) in which two dumps differ, byte for byte."""
    out = [k for k in DUMP_BUFFERS if A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    if A["seed_h"][:, :15].tobytes() != B["seed_h"][:, :15].tobytes():
        out.append("seed_h")
    out += ["ctl." + k for k in A["ctl"] if np.float32(A["ctl"][k]).tobytes() != np.float32(B["ctl"][k]).tobytes()]
    return out


# ----------------------------------------------------------------------------- a dump from the fp32 torch oracle
def dump_from_oracle(src, tgt, p, matcher_cls=None):
    """Runs ``oracle.sc2pcr.Matcher`` (fp32 torch, CPU) with its ``taps`` and packs what it recorded into the device's format.  The
    format defines ``Ts`` as the fp32 storage of an fp64 solve of ``seed_h``, so that is what the dump holds (the oracle's own fp32
    SVD cannot meet a 4 * 2^-24 bound); fitness, arg-max and refinement then follow from those ``Ts`` in the oracle's fp32 arithmetic."""
    import torch
    from oracle import sc2pcr as osc
    n = len(src)
    P = plan(n, p)
    words, S, k1 = P["words"], P["n_seed"], P["k1"]
    m = (matcher_cls or osc.Matcher)(inlier_threshold=p["inlier_threshold"], num_node="all", use_mutual=False, d_thre=p["d_thre"],
                                     num_iterations=p["num_iterations"], ratio=p["ratio"], nms_radius=p["nms_radius"],
                                     max_points=16384, k1=p["k1"], k2=p["k2"])
    m.taps = t = {}
    ts, tt = torch.from_numpy(np.asarray(src, np.float32))[None], torch.from_numpy(np.asarray(tgt, np.float32))[None]
    m.SC2_PCR(ts, tt)
    hard_b = t["hard"].numpy().astype(bool)
    hard, tight = pack_bits(hard_b, words), pack_bits(t["tight"].numpy().astype(bool), words)
    deg = hard_b.sum(1)
    nnz = int(deg.sum())
    dense = int(nnz > P["csr_cap"])
    i, j = np.nonzero(hard_b)
    seed_h = np.zeros((S, 16))
    seed_h[:, :15] = t["seed_h"].numpy().astype(np.float64)
    R, tr, _ = kabsch64(seed_h[:, 0:3], seed_h[:, 3:6], seed_h[:, 6:15].reshape(S, 3, 3))
    Ts = np.tile(np.eye(4, dtype=np.float32), (S, 1, 1))
    Ts[:, :3, :3], Ts[:, :3, 3] = R, tr
    Tt = torch.from_numpy(Ts)
    pred = torch.einsum("snm,mk->snk", Tt[:, :3, :3], ts[0].T) + Tt[:, :3, 3:4]
    fit = (torch.norm(pred.permute(0, 2, 1) - tt, dim=-1) < p["inlier_threshold"]).float().sum(-1).numpy()
    best = int(np.argmax(fit))
    T = m.post_refinement(Tt[best][None], ts, tt, 20)[0].numpy()
    score = t["score"].numpy()
    order = np.argsort(-score.astype(np.float64), kind="stable")
    rank = np.empty(n, np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    cnt = np.zeros((S, words * 64), np.uint16)
    cnt[:, :n] = t["sc2"].numpy().astype(np.uint16)
    return dict(src=np.asarray(src, np.float32), tgt=np.asarray(tgt, np.float32), params=p, n=n, words=words, n_seed=S, k1=k1, k2=P["k2"],
                csr_cap=P["csr_cap"],
                ctl=dict(converged=int(t["converged"]), iters=int(t["iters"]), best_seed=best, best_fitness=float(fit[best]), norm=0.0,
                         dense=dense),
                v=t["v"].numpy().copy(), score=score.copy(), seeds=t["seeds"].numpy().astype(np.int32), hard=hard, tight=tight,
                knn=t["knn"].numpy().astype(np.int32), Ts=Ts.reshape(S, 16), dom=t["dom"].numpy().astype(np.int32), rank=rank,
                ptr_h=np.concatenate([[0], np.cumsum(deg)]).astype(np.int32),
                col_h=(np.zeros(0, np.uint16) if dense else j.astype(np.uint16)),
                val_h=(np.zeros(0, np.float32) if dense else t["soft"].numpy()[i, j].copy()), cnt=cnt,
                blk_dense=np.ones((S + 63) // 64, np.uint8), seed_h=seed_h, fitness=fit.astype(np.float32), T=T)
