"""GPU parity: feature nearest neighbour / pdist through the C ABI vs the oracle (bit-exact) and vs
the reference's golden vectors (tie audit)."""
import os

import numpy as np
import pytest
import torch

import _inputs as gi
import mutual_restatement as M

pytestmark = pytest.mark.gpu


def _golden(name):
    return np.load(os.path.join(os.path.dirname(__file__), "golden", name))


@pytest.mark.parametrize("tag", ["big", "odd", "wide"])
def test_find_nn_gpu_bit_exact_vs_oracle_and_golden(tag):
    import eyoc_amd
    from oracle import matching as om
    g = _golden("g1_nn.npz")
    seed, n0, n1 = (int(v) for v in g[f"{tag}_meta"])
    F0, F1 = gi.nn_case(seed, n0, n1)
    inds, d = eyoc_amd.find_nn_gpu(torch.from_numpy(F0).cuda(), torch.from_numpy(F1).cuda(), nn_max_n=500,
                                   return_distance=True)
    assert inds.dtype == torch.int64 and not inds.is_cuda and d.shape == (n0, 1)
    o_i, o_d = om.find_nn(F0, F1, return_distance=True)
    np.testing.assert_array_equal(inds.numpy(), o_i)                      # indices: bit-exact
    np.testing.assert_array_equal(d.numpy().view(np.uint32), o_d.view(np.uint32))   # distances: bit-exact
    ref = g[f"{tag}_inds"].astype(np.int64)
    diff = np.nonzero(inds.numpy() != ref)[0]
    assert len(diff) <= max(2, n0 // 1000)
    for i in diff:                                                         # only genuine near-ties may differ
        D = om.sqdist_rows(F0[i:i + 1], F1)[0]
        assert abs(D[inds[i]] - D[ref[i]]) <= 4e-6
    # L2 variant
    indsL, dL = eyoc_amd.find_nn_gpu(torch.from_numpy(F0).cuda(), torch.from_numpy(F1).cuda(), return_distance=True,
                                     dist_type="L2")
    oL_i, oL_d = om.find_nn(F0, F1, return_distance=True, dist_type="L2")
    np.testing.assert_array_equal(indsL.numpy(), oL_i)
    np.testing.assert_array_equal(dL.numpy().view(np.uint32), oL_d.view(np.uint32))


@pytest.mark.parametrize("c", [16, 64, 128])
def test_find_nn_other_feature_dims(c):
    import eyoc_amd
    from oracle import matching as om
    F0, F1 = gi.nn_case(70 + c, 333, 777, c=c)
    inds = eyoc_amd.find_nn_gpu(torch.from_numpy(F0).cuda(), torch.from_numpy(F1).cuda())
    np.testing.assert_array_equal(inds.numpy(), om.find_nn(F0, F1))


def test_find_nn_ties_and_edge_shapes():
    import eyoc_amd
    F1 = torch.zeros(600, 32)
    F1[5] = F1[300] = F1[599] = 1.0                       # three identical candidates in different tiles/waves
    F0 = torch.ones(3, 32)
    assert eyoc_amd.find_nn_gpu(F0.cuda(), F1.cuda()).tolist() == [5, 5, 5]
    assert eyoc_amd.find_nn_gpu(torch.zeros(1, 32).cuda(), F1.cuda()).tolist() == [0]
    assert eyoc_amd.find_nn_gpu(torch.zeros(0, 32).cuda(), F1.cuda()).shape == (0,)
    with pytest.raises(eyoc_amd.EyocError):
        eyoc_amd.find_nn_gpu(torch.zeros(4, 24).cuda(), torch.zeros(4, 24).cuda())   # unsupported width
    with pytest.raises(NotImplementedError):
        eyoc_amd.find_nn_gpu(F0.cuda(), F1.cuda(), dist_type="cosine")


def test_segmented_knn_equals_per_segment_calls():
    import eyoc_amd
    from oracle import matching as om
    rng = np.random.default_rng(0)
    sizes_a, sizes_b = [100, 1, 257, 64], [300, 50, 129, 1000]
    A = [gi.unit_feats(90 + i, n) for i, n in enumerate(sizes_a)]
    B = [gi.unit_feats(95 + i, n) for i, n in enumerate(sizes_b)]
    seg_a, seg_b = np.cumsum([0] + sizes_a), np.cumsum([0] + sizes_b)
    idx, dist = eyoc_amd.knn1_segmented(torch.from_numpy(np.concatenate(A)).cuda(), torch.from_numpy(np.concatenate(B)).cuda(),
                                        seg_a, seg_b)
    for s in range(4):
        oi, od = om.find_nn(A[s], B[s], return_distance=True)
        np.testing.assert_array_equal(idx[seg_a[s]:seg_a[s + 1]].cpu().numpy(), oi)
        np.testing.assert_array_equal(dist[seg_a[s]:seg_a[s + 1]].cpu().numpy(), od[:, 0])


def test_pdist_matches_oracle_and_golden():
    import eyoc_amd
    from oracle import matching as om
    g = _golden("g1_nn.npz")
    A, B = gi.nn_case(14, 16, 8)
    for dt, key in (("SquareL2", "small_pdist_sq"), ("L2", "small_pdist_l2")):
        out = eyoc_amd.pdist(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), dt).cpu().numpy()
        np.testing.assert_array_equal(out, om.pdist(A, B, dt))
        np.testing.assert_allclose(out, g[key], atol=2e-6)


def test_find_corr_and_random_sample_glue():
    import eyoc_amd
    from oracle import matching as om
    F0, F1 = gi.nn_case(33, 900, 800)
    xyz0 = torch.from_numpy(gi._u(34, 900, 3).astype(np.float32))
    xyz1 = torch.from_numpy(gi._u(35, 800, 3).astype(np.float32))
    a0, a1 = eyoc_amd.find_corr(xyz0, xyz1, torch.from_numpy(F0).cuda(), torch.from_numpy(F1).cuda(), subsample_size=500,
                                rng=np.random.RandomState(7))
    r = np.random.RandomState(7)
    i0, i1 = r.choice(900, 500, replace=False), r.choice(800, 500, replace=False)
    b0, b1 = om.find_corr(xyz0.numpy(), xyz1.numpy(), F0, F1, 500, inds0=i0, inds1=i1)
    np.testing.assert_array_equal(a0.numpy(), b0)
    np.testing.assert_array_equal(a1.numpy(), b1)
    # no sub-sampling when the cloud is small
    c0, c1 = eyoc_amd.find_corr(xyz0, xyz1, torch.from_numpy(F0).cuda(), torch.from_numpy(F1).cuda(), subsample_size=5000)
    assert c0.shape == (900, 3) and c1.shape == (900, 3)
    p, f = eyoc_amd.random_sample(xyz0.numpy(), torch.from_numpy(F0), 1200, rng=np.random.RandomState(1))
    assert p.shape == (1200, 3) and f.shape == (1200, 32)
    p, f = eyoc_amd.random_sample(xyz0.numpy(), torch.from_numpy(F0), 900)
    assert p.shape == (900, 3)


def test_dotmax_streaming_argmax_vs_dense_matmul():
    """eyoc_dotmax = ``(F0 @ F1.T).max(dim=1)`` of util/transform_estimation.py:131-133 without the matrix: weights to
    fp32 rounding, indices equal wherever the dense maximum is unambiguous; also a negative-only row and segments."""
    from eyoc_amd.eval import dotmax_segmented
    rng = np.random.default_rng(17)

    def unit(n, c):
        f = rng.normal(size=(n, c)).astype(np.float32)
        return f / np.linalg.norm(f, axis=1, keepdims=True).astype(np.float32)

    for na, nb, c in ((3000, 3500, 32), (70, 9, 16), (500, 1200, 64)):
        A, B = unit(na, c), unit(nb, c)
        A[5] = -B.mean(0) * 50                                  # every inner product of this row is negative
        w, idx = dotmax_segmented(torch.from_numpy(A), torch.from_numpy(B), [0, na], [0, nb])
        D = A.astype(np.float64) @ B.T.astype(np.float64)
        ref_i, ref_w = D.argmax(1), D.max(1)
        np.testing.assert_allclose(w.cpu().numpy(), ref_w, rtol=0, atol=3e-6 * max(1.0, np.abs(ref_w).max()))
        top2 = np.sort(D, axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 1e-5 * np.abs(top2[:, 1]).clip(1e-3)
        np.testing.assert_array_equal(idx.cpu().numpy()[clear], ref_i[clear])
        assert clear.mean() > 0.9
    A, B = unit(600, 32), unit(700, 32)
    w, idx = dotmax_segmented(torch.from_numpy(A), torch.from_numpy(B), [0, 100, 600], [0, 300, 700])
    D0, D1 = A[:100] @ B[:300].T, A[100:] @ B[300:].T
    got = idx.cpu().numpy()
    assert (got[:100] == D0.argmax(1)).mean() > 0.98 and (got[100:] == D1.argmax(1)).mean() > 0.98
    assert got[:100].max() < 300 and got[100:].max() < 400


def test_many_segments_in_one_call():
    """100 segments in one launch and 150 through the wrapper's chunking (the library takes 128 per launch)."""
    from eyoc_amd.eval import knn1_segmented
    from oracle import matching as om
    rng = np.random.default_rng(23)
    for nseg in (100, 150):
        na = rng.integers(1, 40, nseg); nb = rng.integers(1, 50, nseg)
        A = rng.normal(size=(int(na.sum()), 32)).astype(np.float32)
        B = rng.normal(size=(int(nb.sum()), 32)).astype(np.float32)
        sa, sb = np.r_[0, np.cumsum(na)], np.r_[0, np.cumsum(nb)]
        idx, d = knn1_segmented(torch.from_numpy(A), torch.from_numpy(B), sa, sb)
        idx, d = idx.cpu().numpy(), d.cpu().numpy()
        for s in range(nseg):
            ri, rd = om.find_nn(A[sa[s]:sa[s + 1]], B[sb[s]:sb[s + 1]], return_distance=True)
            np.testing.assert_array_equal(idx[sa[s]:sa[s + 1]], ri)
            np.testing.assert_array_equal(d[sa[s]:sa[s + 1]], rd[:, 0])


@pytest.fixture
def prefilter_always():
    from eyoc_amd import _lib
    lib = _lib.load()
    prev = _lib.knob("eyoc_knn_prefilter", 2)
    yield lib
    _lib.knob("eyoc_knn_prefilter", prev)


def test_mfma_prefilter_gives_the_contract_indices(prefilter_always):
    """The fp32-MFMA score pre-filter (knn.hip) only ever decides rows whose runner-up is out of rounding reach and
    hands the rest to the exact kernel: indices identical to the oracle on ordinary features, on segments of odd sizes,
    on exact ties (duplicated targets, lowest index wins), on near-ties one ulp apart, with NaN rows and with
    features of very different norms."""
    import eyoc_amd
    from eyoc_amd import _lib
    from oracle import matching as om
    lib = prefilter_always
    rng = np.random.default_rng(5)

    def check(A, B, seg_a=None, seg_b=None, oracle=True):
        seg_a = np.array([0, len(A)]) if seg_a is None else seg_a
        seg_b = np.array([0, len(B)]) if seg_b is None else seg_b
        got = eyoc_amd.knn1_segmented(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), seg_a, seg_b,
                                      return_distance=False).cpu().numpy()
        for s in range(len(seg_a) - 1 if oracle else 0):
            np.testing.assert_array_equal(got[seg_a[s]:seg_a[s + 1]], om.find_nn(A[seg_a[s]:seg_a[s + 1]], B[seg_b[s]:seg_b[s + 1]]))
        _lib.knob("eyoc_knn_prefilter", 0)
        ref = eyoc_amd.knn1_segmented(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), seg_a, seg_b,
                                      return_distance=False).cpu().numpy()
        _lib.knob("eyoc_knn_prefilter", 2)
        np.testing.assert_array_equal(got, ref)

    # ordinary unit features, ragged segments (tiles of 16 targets / 64 queries with tails)
    sizes_a, sizes_b = [100, 1, 257, 64, 1000], [300, 50, 129, 1000, 17]
    A = np.concatenate([gi.unit_feats(190 + i, n) for i, n in enumerate(sizes_a)])
    B = np.concatenate([gi.unit_feats(195 + i, n) for i, n in enumerate(sizes_b)])
    check(A, B, np.cumsum([0] + sizes_a), np.cumsum([0] + sizes_b))
    # exact ties: every target appears three times (shuffled), queries ARE targets
    base = gi.unit_feats(7, 400)
    B = np.concatenate([base, base, base])[rng.permutation(1200)]
    check(base[:300].copy(), B)
    # near-ties: targets that differ from each other in the last bits of one channel
    B = np.repeat(gi.unit_feats(8, 50), 20, axis=0)
    B[:, 3] = np.nextafter(B[:, 3], np.float32(2.0) * np.sign(rng.normal(size=len(B))).astype(np.float32))
    check(gi.unit_feats(9, 500), B)
    # clustered features: many candidates within 1e-5 of the best
    centre = gi.unit_feats(10, 1)
    B = (centre + 1e-6 * rng.normal(size=(2000, 32))).astype(np.float32)
    check((centre + 1e-6 * rng.normal(size=(200, 32))).astype(np.float32), B)
    # very different norms
    A = (gi.unit_feats(11, 300) * rng.uniform(1e-3, 1e3, size=(300, 1))).astype(np.float32)
    B = (gi.unit_feats(12, 900) * rng.uniform(1e-3, 1e3, size=(900, 1))).astype(np.float32)
    check(A, B)
    # ... and a NaN / an inf row on either side: whatever the exact kernel answers (a NaN distance never wins there;
    # numpy's argmin, i.e. the oracle, lets it win), the pre-filter must answer the same
    A[7, 5] = np.nan
    A[9, 0] = np.inf
    B[100, 2] = np.nan
    B[200, 1] = np.inf
    check(A, B, oracle=False)


def test_mfma_prefilter_decides_almost_every_row_of_the_bench_query(prefilter_always):
    """5000 x 5000 unit features per pair (the bench's query): the exact second pass sees a handful of rows."""
    import eyoc_amd
    from eyoc_amd import _lib
    from oracle import matching as om
    F0, F1 = gi.unit_feats(300, 5000), gi.unit_feats(301, 5000)
    got = eyoc_amd.knn1_segmented(torch.from_numpy(F0).cuda(), torch.from_numpy(F1).cuda(), np.array([0, 5000]), np.array([0, 5000]),
                                  return_distance=False).cpu().numpy()
    np.testing.assert_array_equal(got, om.find_nn(F0, F1))


def test_two_streams_share_the_scratch_safely():
    """kNN calls issued back to back on two torch streams use the same grow-only scratch buffer of the context: the
    library makes the second stream wait for the first one's work (eyoc_ctx::ensure_scratch), so both results are right."""
    import eyoc_amd
    from oracle import matching as om
    cases = [(gi.unit_feats(400 + i, 3000), gi.unit_feats(410 + i, 3000)) for i in range(4)]
    dev = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in cases]
    want = [om.find_nn(a, b) for a, b in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(3):
        got = []
        for i, (a, b) in enumerate(dev):
            with torch.cuda.stream(streams[i & 1]):
                got.append(eyoc_amd.knn1_segmented(a, b, np.array([0, len(a)]), np.array([0, len(b)]), return_distance=False))
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g.cpu().numpy(), w)


# ----------------------------------------------------------------------------- Matcher.match_pair
def _gemm_l2(A, B, seg_a=None, seg_b=None, dist=True):
    import eyoc_amd
    seg_a = np.array([0, len(A)]) if seg_a is None else seg_a
    seg_b = np.array([0, len(B)]) if seg_b is None else seg_b
    out = eyoc_amd.knn1_segmented(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), seg_a, seg_b, "GemmL2", return_distance=dist)
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if dist else out.cpu().numpy()


def _match_cases():
    rng = np.random.default_rng(77)
    F0, F1 = gi.nn_case(500, 5000, 5000)                        # unit-norm, the path's size
    F1 = F1.copy()
    F1[1000:1400] = F1[:400]                                    # exact ties (lowest index must win)
    F1[2000:2300] = F1[:300]
    F1[2000:2300, 7] = np.nextafter(F1[2000:2300, 7], np.float32(2.0))     # ... and one-ulp near-ties
    yield "unit+ties", F0, F1
    centre = gi.unit_feats(501, 1)                              # hundreds of candidates whose distances round together
    yield "cluster", (centre + 1e-6 * rng.normal(size=(300, 32))).astype(np.float32), \
        (centre + 1e-6 * rng.normal(size=(3000, 32))).astype(np.float32)
    R0, R1 = gi.match_pair_case("raw", 502, 3000, 4000)         # NOT unit-norm: arg-max of <a,b>, NaN rows
    yield "raw", R0, R1
    yield "raw-big", (R0 * 40).astype(np.float32), (R1 * 0.03).astype(np.float32)
    yield "odd", *gi.match_pair_case("raw", 503, 257, 129)


_ORACLE_MATCH = {}       # case name -> (indices, distances of the first 400 rows): both parametrisations ask the CPU oracle for the same


@pytest.mark.parametrize("prefilter", [0, 2])
def test_match_pair_nn_bit_exact_vs_oracle(prefilter):
    """eyoc_knn1 dist_type 2 = the reference's ``argmin sqrt(2 - 2 S + 1e-6)`` (SC2_PCR.py:296-298): indices AND distance
    bits equal to oracle.matching (first NaN wins, ties to the lowest index, distances that round together), with the
    MFMA pre-filter forced on and off."""
    from eyoc_amd import _lib
    from oracle import matching as om
    lib = _lib.load()
    prev = _lib.knob("eyoc_knn_prefilter", prefilter)
    try:
        saw_nan = False
        for name, A, B in _match_cases():
            if name not in _ORACLE_MATCH:
                _ORACLE_MATCH[name] = (om.match_pair_indices(A, B), om.match_pair_distance(A[:400], B))
            want = _ORACLE_MATCH[name][0]
            got = _gemm_l2(A, B, dist=False)
            np.testing.assert_array_equal(got, want, err_msg=name)
            gi_, gd = _gemm_l2(A, B)                              # with distances: the exact kernel alone
            np.testing.assert_array_equal(gi_, want, err_msg=name)
            rows = slice(0, 400)
            D = _ORACLE_MATCH[name][1]
            wd = D[np.arange(D.shape[0]), want[rows]]
            fin = ~np.isnan(wd)
            np.testing.assert_array_equal(gd[rows][fin].view(np.uint32), wd[fin].view(np.uint32), err_msg=name)
            assert np.array_equal(np.isnan(gd[rows]), np.isnan(wd)), name
            saw_nan |= bool(np.isnan(wd).any())
        assert saw_nan
    finally:
        _lib.knob("eyoc_knn_prefilter", prev)


def test_match_pair_segments_and_l2_difference():
    """Segmented dist_type 2 equals per-segment calls; on descriptors that are not unit-norm it is NOT the L2 neighbour
    (the substitution round 2 made silently) - the two disagree on most rows of the raw case."""
    import eyoc_amd
    from oracle import matching as om
    sizes_a, sizes_b = [100, 1, 257, 1000], [300, 50, 129, 17]
    A = np.concatenate([gi.match_pair_case("raw", 510 + i, n, 8)[0] for i, n in enumerate(sizes_a)])
    B = np.concatenate([gi.match_pair_case("raw", 520 + i, 8, n)[1] for i, n in enumerate(sizes_b)])
    sa, sb = np.cumsum([0] + sizes_a), np.cumsum([0] + sizes_b)
    got = _gemm_l2(A, B, sa, sb, dist=False)
    for s in range(len(sizes_a)):
        np.testing.assert_array_equal(got[sa[s]:sa[s + 1]], om.match_pair_indices(A[sa[s]:sa[s + 1]], B[sb[s]:sb[s + 1]]))
    R0, R1 = gi.match_pair_case("raw", 502, 3000, 4000)
    l2 = eyoc_amd.find_nn_gpu(torch.from_numpy(R0).cuda(), torch.from_numpy(R1).cuda()).numpy()
    assert (l2 != om.match_pair_indices(R0, R1)).mean() > 0.3


def test_matcher_match_pair_vs_reference_golden_and_oracle():
    """Matcher.match_pair itself (resampling draw + NN + gathers) against the reference's own output (golden g6) -
    index-coded key points reveal the rows - with the same near-tie audit as the oracle's CPU test, and against the
    oracle exactly."""
    import json
    import eyoc_amd
    from oracle import matching as om
    g = _golden("g6_match.npz")
    for i, (kind, seed, n0, n1, num_node) in enumerate(json.loads(str(g["cases"]))):
        F0, F1 = gi.match_pair_case(kind, seed, n0, n1)
        k0 = np.zeros((1, n0, 3), np.float32); k0[0, :, 0] = np.arange(n0)
        k1 = np.zeros((1, n1, 3), np.float32); k1[0, :, 0] = np.arange(n1)
        m = eyoc_amd.Matcher(inlier_threshold=0.6, num_node=num_node, use_mutual=False, d_thre=0.1, num_iterations=20,
                             ratio=0.2, nms_radius=0.6, max_points=8000, k1=30, k2=20)
        sc, tc = m.match_pair(torch.from_numpy(k0).cuda(), torch.from_numpy(k1).cuda(), torch.from_numpy(F0)[None].cuda(),
                              torch.from_numpy(F1)[None].cuda(), rng=np.random.RandomState(seed))
        src, tgt = sc[0, :, 0].cpu().numpy().astype(np.int64), tc[0, :, 0].cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(src, g[f"src{i}"])                       # the reference's draw
        if num_node == "all":
            t_sel = np.arange(n1)
        else:
            rs = np.random.RandomState(seed)
            rs.choice(n0, num_node)
            t_sel = rs.choice(n1, num_node)
        A, B = F0[src], F1[t_sel]
        want = om.match_pair_indices(A, B)
        np.testing.assert_array_equal(tgt, t_sel[want])                        # vs oracle: exact
        ref = g[f"tgt{i}"].astype(np.int64)
        diff = np.nonzero(tgt != ref)[0]
        assert len(diff) <= max(2, len(A) // 500)
        for row in diff:                                                         # vs reference: only rounding-level ties
            cand = np.nonzero(t_sel == ref[row])[0][:1]
            d = om.match_pair_distance(A[row:row + 1], B[[want[row], cand[0]]])[0]
            assert np.isnan(d).any() or abs(float(d[0]) - float(d[1])) <= 2e-4 * max(1.0, float(d[0]))


# ----------------------------------------------------------------------------- every instantiation of knn1_kernel
_EXACT_REF = {}          # (query, c, na, nb) -> the restatement's outputs, computed once


def _exact_reference(query, c, na, nb):
    """What the exact kernel must return for ``M.pair_inputs(na, nb, c)``: the three distance forms from tests/mutual_restatement.py
    (index and the winner's entry of its distance matrix), the runner-up and the inner product from oracle.matching's contract
    (``sqdist_rows`` with the winner struck out; ``dot_rows``, first maximum)."""
    from oracle import matching as om
    key = (query, c, na, nb)
    if key not in _EXACT_REF:
        A, B = M.pair_inputs(na, nb, c)
        rows = np.arange(na)
        if query in M.DIST:
            idx = M.search(A, B, [0, na], [0, nb], M.DIST[query])[0]
            out = (idx, M.distance_matrix(A, B, M.DIST[query])[rows, idx])
        elif query == "knn2":
            D = om.sqdist_rows(A, B)
            idx = np.argmin(D, axis=1).astype(np.int64)
            d1 = D[rows, idx].copy()
            D[rows, idx] = np.inf
            out = (idx, d1, D.min(axis=1))
        else:
            S = om.dot_rows(A, B)
            idx = np.argmax(S, axis=1).astype(np.int64)
            out = (idx, S[rows, idx])
        assert not any(np.isnan(o).any() for o in out[1:])              # unit rows: every value is a number, so bits can be compared
        _EXACT_REF[key] = out
    return _EXACT_REF[key]


@pytest.mark.parametrize("query", ["SquareL2", "L2", "GemmL2", "knn2", "dotmax"])
@pytest.mark.parametrize("c", M.WIDTHS)
def test_exact_kernel_every_width_and_query_bit_exact(c, query):
    """knn1_kernel<C, TOP2, MODE> has 5 widths x {distance (SquareL2 and L2 share one), GemmL2, runner-up, inner product} = 20
    instantiations; with the pre-filter off every query below runs exactly one of them.  Index bytes and the bits of every float the
    call returns, at 65 x 33 (a query tile boundary at 64, a target count that is no multiple of the group of 8, a split boundary at 32)
    and 257 x 255 (several tiles and splits, all four waves busy)."""
    import eyoc_amd
    from eyoc_amd import _lib
    from eyoc_amd.eval import dotmax_segmented
    prev = _lib.knob("eyoc_knn_prefilter", 0)
    try:
        for na, nb in M.WIDE_SHAPES:
            A, B = (torch.from_numpy(x).cuda() for x in M.pair_inputs(na, nb, c))
            if query in M.DIST:
                got = eyoc_amd.knn1_segmented(A, B, [0, na], [0, nb], query)
            elif query == "knn2":
                got = eyoc_amd.knn2_segmented(A, B, [0, na], [0, nb])
            else:
                w, idx = dotmax_segmented(A, B, [0, na], [0, nb])
                got = (idx, w)
            want = _exact_reference(query, c, na, nb)
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                g = g.cpu().numpy()
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"output {k} of {query}, c = {c}, {na} x {nb} differs"
    finally:
        _lib.knob("eyoc_knn_prefilter", prev)
