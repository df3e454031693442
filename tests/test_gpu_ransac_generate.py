"""The two forms of the RANSAC hypothesis generator (eyoc_ransac_select_generate: 0 the exact round-6 k_generate, 1 k_generate_q on
16-bit records with banded edge checks) must give the same result records byte for byte - k_fit re-evaluates the exact edge
expression on whatever either form hands it - and both must agree with oracle/ransac.py.  Also here: the packing kernel of the kNN
pre-filter (knn_pack_targets_mfma) against a numpy restatement of its arithmetic, bit for bit.

The survivor lists themselves live at internal offsets of the workspace and their order depends on atomics; a test reaches them
through the records only (``survivors`` is their length, the winner and its count come out of them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _inputs as gi
from test_ransac_prefilter_host import _edge_family

pytestmark = pytest.mark.gpu

LDS_RECORDS_Q = 12000          # eyoc_amd/csrc/ransac.hip: more correspondences than this in a pair and the launch takes the exact form from global memory
T0 = gi.rigid(0.02, -0.01, 0.12, 4.0, -1.0, 0.3)


def _lib():
    from eyoc_amd import _lib as L
    return L, L.load()


def _batch(cases):
    """``cases``: (p0, p1) per pair, identity correspondences -> (src, tgt, corr, seg)."""
    seg = [0]
    for p0, _ in cases:
        seg.append(seg[-1] + len(p0))
    s = torch.from_numpy(np.concatenate([c[0] for c in cases]).astype(np.float32))
    t = torch.from_numpy(np.concatenate([c[1] for c in cases]).astype(np.float32))
    corr = torch.cat([torch.arange(len(c[0])) for c in cases])
    return s, t, corr, seg


def _both_forms(cases, thr, H, seed, edge_sim=0.9):
    """Result records ``[P, 84] uint8`` under form 0 and form 1."""
    from eyoc_amd import registration as reg
    L, lib = _lib()
    s, t, corr, seg = _batch(cases)
    out = {}
    prev = L.knob("eyoc_ransac_select_generate", -1)
    assert prev == 1, "the compact form is the default"
    try:
        for form in (0, 1):
            L.knob("eyoc_ransac_select_generate", form)
            out[form] = reg.ransac_batched_from_correspondences(s, t, corr, seg, seg, thr, H, seed=seed, edge_similarity=edge_sim).cpu().numpy()
    finally:
        L.knob("eyoc_ransac_select_generate", prev)
    np.testing.assert_array_equal(out[1], out[0], err_msg="compact against exact generate")
    return out[1]


def _against_oracle(rec_bytes, p0, p1, thr, H, seed, edge_sim=0.9, winner=True, inliers=True):
    """``winner=False`` for clouds of EXACT inliers: thousands of hypotheses tie on the count there and an RMSE of ~1e-15 decides, which
    the oracle's SVD and the device's Jacobi sweeps need not agree on (the two forms of the generator still must, byte for byte).
    ``inliers=False`` where only DEGENERATE samples survive (edge_similarity 1: both edge lengths equal to the last bit - repeated
    indices): their rotation is not determined, so neither is the count; the number of survivors is."""
    from eyoc_amd import registration as reg
    from oracle import ransac as orn
    res = reg.decode_ransac_result(torch.from_numpy(rec_bytes), len(p0))
    ref = orn.ransac(p0, p1, np.arange(len(p0)), thr, H, seed=seed, edge_similarity=edge_sim)
    assert res.survivors == ref["survivors"]
    if ref["survivors"] == 0:
        assert res.best_hypothesis == -1 and res.inliers == 0
        return res
    if not inliers:
        return res
    assert res.inliers == ref["inliers"]
    if not winner:
        return res
    assert res.best_hypothesis == ref["best_h"]
    assert res.inlier_rmse == pytest.approx(ref["rmse"], rel=1e-5)
    np.testing.assert_allclose(res.transformation, ref["T"], atol=1e-5)
    return res


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 600])
def test_small_pairs(n):
    p0, p1, _ = gi.corr_case(1000 + n, n, T0, 1.0 if n < 63 else 0.5, noise=0.03)
    H = 1 << 17 if n >= 63 else 1 << 12
    rec = _both_forms([(p0, p1)], 0.3, H, seed=7)
    res = _against_oracle(rec[0], p0, p1, 0.3, H, 7)
    assert res.survivors > 0


@pytest.mark.parametrize("n", [LDS_RECORDS_Q - 1, LDS_RECORDS_Q, LDS_RECORDS_Q + 1])
def test_around_the_lds_capacity_of_the_compact_records(n):
    """One below and at the capacity: 16-bit records in LDS, one workgroup per CU; one above: the global-memory fallback."""
    p0, p1, _ = gi.corr_case(77, n, T0, 0.6, noise=0.03)
    H = 1 << 14
    rec = _both_forms([(p0, p1)], 0.3, H, seed=3)
    res = _against_oracle(rec[0], p0, p1, 0.3, H, 3)
    assert res.survivors > 100


@pytest.mark.parametrize("P", [1, 2, 33])
def test_batches(P):
    """33 pairs cross the 32-pair rule of the count bound; ragged sizes from 5 to 5600 (5600 > 5461: the launch keeps one workgroup per CU)."""
    sizes = [5000, 5, 777, 64, 5600, 1500, 33][:max(P, 1)] if P <= 7 else [5000, 5, 777, 64, 5600, 1500, 33] + [300 + 37 * k for k in range(P - 7)]
    cases = []
    for b, n in enumerate(sizes):
        p0, p1, _ = gi.corr_case(300 + b, n, T0, 0.3 if n > 100 else 1.0, noise=0.04)
        cases.append((p0, p1))
    H = 1 << 16
    rec = _both_forms(cases, 0.3, H, seed=21)
    for b in sorted({0, P - 1, min(2, P - 1)}):
        _against_oracle(rec[b], cases[b][0], cases[b][1], 0.3, H, 21 + b)


def test_no_survivor_and_every_hypothesis_surviving():
    rng = np.random.default_rng(0)
    noise0 = ((rng.random((900, 3)) - 0.5) * 80).astype(np.float32)
    noise1 = ((rng.random((900, 3)) - 0.5) * 80).astype(np.float32)
    same = ((rng.random((700, 3)) - 0.5) * 60).astype(np.float32)
    H = 1 << 15
    rec = _both_forms([(noise0, noise1), (same, same.copy())], 0.3, H, seed=5)
    none = _against_oracle(rec[0], noise0, noise1, 0.3, H, 5)
    every = _against_oracle(rec[1], same, same, 0.3, H, 6, winner=False)
    assert none.survivors == 0 and every.survivors == H and every.inliers == 700


@pytest.mark.parametrize("pad", [79.9, 1.0e4])
def test_adversarial_edges(pad):
    """The threshold family of the host test (edge ratios at fp32(0.9) and one ulp beside it) as a cloud, a cloud of coincident and
    sub-step points, and a cloud whose points are all equal (every edge has length zero: every hypothesis passes the edge checks)."""
    fam = _edge_family([0.003, 0.05, 0.3, 1.0, 7.7, 31.0, 64.0], (0.3, -2.0, 0.7), (-11.3, 7.9, 1.1), pad)
    rng = np.random.default_rng(1)
    base = ((rng.random((300, 3)) - 0.5) * 2 * pad).astype(np.float32)
    tiny = np.concatenate([base, base[:100], base[:100] + np.float32(pad * 2.0 ** -17)]).astype(np.float32)
    R, t = T0[:3, :3].astype(np.float32), T0[:3, 3].astype(np.float32)
    tiny_t = (tiny @ R.T + t + rng.normal(0, 0.03, tiny.shape)).astype(np.float32)
    # the family's points lie on one line: well-spread inliers beside them, so that the fits the winner comes from are not degenerate
    fam_s = np.concatenate([fam[:, :3], base])
    fam_t = np.concatenate([fam[:, 3:], (base @ R.T + t + rng.normal(0, 0.03, base.shape)).astype(np.float32)])
    equal = np.tile(np.array([[3.5, -2.25, 0.75]], np.float32), (40, 1))
    cases = [(fam_s, fam_t), (tiny, tiny_t), (equal, equal.copy())]
    H = 1 << 14
    rec = _both_forms(cases, 0.3, H, seed=9)
    for b, (p0, p1) in enumerate(cases):
        _against_oracle(rec[b], p0, p1, 0.3, H, 9 + b, winner=b < 2)
    for es in (0.5, 1.0):
        rec = _both_forms(cases[:2], 0.3, H, seed=9, edge_sim=es)
        _against_oracle(rec[0], cases[0][0], cases[0][1], 0.3, H, 9, edge_sim=es, inliers=es < 1.0)


def test_a_pair_with_a_nan_coordinate_beside_a_clean_pair():
    """The clean pair keeps its bytes (those of a run on its own); the faulty pair and an all-zero pair - neither has a usable scale:
    k_fit evaluates the exact expression on all of their hypotheses - behave as under form 0."""
    p0, p1, _ = gi.corr_case(55, 600, T0, 0.5, noise=0.03)
    b0, b1, _ = gi.corr_case(56, 400, T0, 0.6, noise=0.03)
    b0 = b0.copy(); b0[17, 1] = np.nan
    z = np.zeros((50, 3), np.float32)
    H = 1 << 15
    alone = _both_forms([(p0, p1)], 0.3, H, seed=13)
    rec = _both_forms([(p0, p1), (b0, b1), (z, z)], 0.3, H, seed=13)
    np.testing.assert_array_equal(rec[0], alone[0])
    _against_oracle(rec[0], p0, p1, 0.3, H, 13)
    from eyoc_amd import registration as reg
    assert reg.decode_ransac_result(torch.from_numpy(rec[2]), 50).survivors == H


# ---------------------------------------------------------------------------------------------------------------------
# knn_pack_targets_mfma
# ---------------------------------------------------------------------------------------------------------------------
F32, F64 = np.float32, np.float64


def _fma32(a, b, c):
    """Correctly rounded fp32 fma of fp32 arrays: the product is exact in fp64; the fp64 sum is rounded to odd (TwoSum gives the sign of
    what it lost), so the final rounding to fp32 is the only one that counts."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    nudged = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    s = np.where((err != 0) & even & np.isfinite(s), nudged, s)
    return s.astype(F32)


def _pack_reference(B, seg_b, zero_norm=False):
    """(packed float32 words, bmax bits) as the kernel writes them."""
    out, bmax = [], []
    for s in range(len(seg_b) - 1):
        rows = B[seg_b[s]:seg_b[s + 1]]
        nb = len(rows)
        n16 = (nb + 15) // 16
        v = rows.reshape(nb, 8, 4)
        x, y, z, w = v[..., 0], v[..., 1], v[..., 2], v[..., 3]
        term = _fma32(w, w, _fma32(z, z, _fma32(x, x, (y * y).astype(F32))))          # [nb, 8]
        n2 = (term[:, 0] + term[:, 1]).astype(F32)
        for q in range(2, 8):
            n2 = (n2 + term[:, q]).astype(F32)
        mx = np.abs(rows).max(1) if nb else np.zeros(0, F32)
        scale = np.ones(nb, F32)
        good = (mx > 0) & np.isfinite(mx)
        scale[good] = np.ldexp(F32(1.0), 8 - np.frexp(mx[good])[1]).astype(F32)
        xs = (rows * scale[:, None]).astype(F32)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(F32)).astype(np.float16)
        tile = np.zeros((n16, 3, 64, 4), F32)
        hi_w = np.zeros((n16 * 16, 4, 8), np.float16); lo_w = np.zeros_like(hi_w)
        hi_w[:nb] = hi.reshape(nb, 4, 8); lo_w[:nb] = lo.reshape(nb, 4, 8)
        # lane (g, j) of tile t: channels 8 g .. 8 g + 7 of target 16 t + j
        hv = hi_w.reshape(n16, 16, 4, 8).transpose(0, 2, 1, 3).reshape(n16, 64, 8)
        lv = lo_w.reshape(n16, 16, 4, 8).transpose(0, 2, 1, 3).reshape(n16, 64, 8)
        tile[:, 0] = np.ascontiguousarray(hv).view(F32).reshape(n16, 64, 4)
        tile[:, 1] = np.ascontiguousarray(lv).view(F32).reshape(n16, 64, 4)
        norm = np.full(n16 * 16, np.inf, F32); norm[:nb] = 0.0 if zero_norm else n2
        inv = np.zeros(n16 * 16, F32); inv[:nb] = F32(1.0) / scale
        tile[:, 2, :, 0] = np.tile(norm.reshape(n16, 1, 16), (1, 4, 1)).reshape(n16, 64)
        tile[:, 2, :, 1] = np.tile(inv.reshape(n16, 1, 16), (1, 4, 1)).reshape(n16, 64)
        out.append(tile.reshape(-1))
        bmax.append(int(n2.view(np.int32).max()) if nb else 0)
    return np.concatenate(out) if out else np.zeros(0, F32), np.array(bmax, np.int32)


@pytest.mark.parametrize("zero_norm", [0, 1])
def test_pack_targets_bit_identical(zero_norm):
    """Segments of 1, 15, 16, 17 and 5000 targets with empty segments between live ones, rows of very different magnitude: the packed
    operand (fp16 hi / lo halves, norms, inverse scales) and the per-segment largest norm, bit for bit."""
    L, lib = _lib()
    sizes = [1, 0, 15, 16, 0, 0, 17, 5000, 0, 64, 65]
    seg_b = [0]
    for n in sizes:
        seg_b.append(seg_b[-1] + n)
    rng = np.random.default_rng(42)
    B = rng.normal(size=(seg_b[-1], 32)).astype(F32)
    B *= np.exp2(rng.integers(-12, 12, (seg_b[-1], 1))).astype(F32)                        # every row its own magnitude
    B[3] = 0.0                                                                             # an all-zero row: scale 1
    want, want_max = _pack_reference(B, seg_b, bool(zero_norm))
    Bd = torch.from_numpy(B).cuda()
    packed = torch.full((want.size + 64,), 7.0, dtype=torch.float32, device="cuda")
    bmax = torch.full((len(sizes),), -1, dtype=torch.int32, device="cuda")
    sb = (C.c_int32 * len(seg_b))(*seg_b)
    L.check(lib.eyoc_knn_pack_targets(L.ctx(), L.ptr(Bd), sb, len(sizes), zero_norm, L.ptr(packed), want.size, L.ptr(bmax), L.stream_ptr()))
    got = packed.cpu().numpy()
    np.testing.assert_array_equal(got[:want.size].view(np.uint32), want.view(np.uint32))
    assert (got[want.size:] == 7.0).all()                                                  # nothing past the last tile
    np.testing.assert_array_equal(bmax.cpu().numpy(), want_max)
