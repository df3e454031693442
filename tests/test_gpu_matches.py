"""Radius matches on the GPU (``eyoc_radius_matches_count`` / ``_fill``, ``eyoc_amd.matches``) against the fp64 restatement
(tests/matches_restatement.py, ``brute``: all n0 x n1 candidates).  Every comparison is EXACT - pairs, their order, the bits of d2 and
the status: both sides evaluate the same fp64 expression on the same fp32 inputs, so there is nothing for a tolerance to absorb."""
import numpy as np
import pytest
import torch

import matches_cases as cases
import matches_restatement as M

pytestmark = pytest.mark.gpu


def _device(pairs, T=True):
    src, tgt = [torch.from_numpy(np.ascontiguousarray(s)) for s, _, _ in pairs], [torch.from_numpy(np.ascontiguousarray(t)) for _, t, _ in pairs]
    return src, tgt, (np.stack([T for _, _, T in pairs]) if T else None)


def _run(pairs, r, K=None, collated=False):
    from eyoc_amd import matches
    src, tgt, T = _device(pairs)
    corr, seg, status, d2 = matches.matching_indices_batched(src, tgt, T, r, K, collated=collated, return_d2=True)
    return corr.cpu().numpy(), seg.cpu().numpy(), status.cpu().numpy(), d2.cpu().numpy()


_REF = {}


def _ref(name, pairs, r, K=None):
    """The restatement of a case, computed once and shared (never modified)."""
    key = (name, K)
    if key not in _REF:
        _REF[key] = [M.brute(s, t, T, r, K) for s, t, T in pairs], [M.status(s, t, T, r) for s, t, T in pairs]
    return _REF[key]


def _check(name, pairs, r, K=None):
    corr, seg, status, d2 = _run(pairs, r, K)
    ref, ref_status = _ref(name, pairs, r, K)
    assert status.tolist() == ref_status
    assert seg.tolist() == np.concatenate([[0], np.cumsum([len(p) for p, _ in ref])]).tolist()
    assert corr.dtype == np.int64 and corr.shape == (seg[-1], 2) and d2.dtype == np.float64
    for b, (p, d) in enumerate(ref):
        assert np.array_equal(corr[seg[b]:seg[b + 1]], p), f"pair {b}: pairs or their order differ"
        assert d2[seg[b]:seg[b + 1]].tobytes() == d.tobytes(), f"pair {b}: d2 bits differ"
    return corr, seg, status, d2


def test_ragged_batch_with_faulty_and_empty_pairs():
    pairs, r = cases.ragged()
    corr, seg, status, _ = _check("ragged", pairs, r)
    assert status.tolist() == [0, 0, 0, 0, 0, 0, M.BAD_INIT, M.RANGE, 0]
    m = np.diff(seg)
    assert m[0] > 300 and m[1] > 0 and m[2] > 0 and m[8] > 0 and m[3:8].tolist() == [0] * 5


def test_dense_cluster_ties_and_gate():
    pairs, r = cases.dense()
    (src, tgt, T), = pairs
    d = M._d2(M.pose(src, T)[0][None], tgt.astype(np.float64))
    assert int((d == r * r).sum()) == 6                             # the restatement really sees gate-equal candidates ...
    corr, seg, _, d2 = _check("dense", pairs, r)
    row0 = corr[:, 0] == 0
    assert int(row0.sum()) == 150
    assert int((np.diff(d2[row0]) == 0).sum()) >= 75                # ... and exact ties
    assert not (d2 == r * r).any()


@pytest.mark.parametrize("r", [0.5, 0.45])
def test_cell_faces_negative_cells_and_the_key_range(r):
    pairs, _ = cases.faces(r)
    _, seg, status, _ = _check(f"faces{r}", pairs, r)
    assert status.tolist() == [0, 0, 0, M.RANGE, 0, M.RANGE, M.RANGE]
    assert seg[3] - seg[2] >= 3 and seg[5] - seg[4] >= 3            # matches in the outermost cells of the key range


@pytest.mark.parametrize("K", [1, 3, 1000])
def test_K_keeps_the_first_of_the_sorted_list(K):
    pairs, r = cases.ragged()
    corr, seg, _, d2 = _check("ragged", pairs, r, K)
    if K == 1000:
        full, _ = _ref("ragged", pairs, r, None)
        assert sum(len(p) for p, _ in full) == len(corr)
    if K == 1:      # the nearest neighbour under the same gate, wherever the ICP evaluation returns one
        from eyoc_amd import icp
        for b in (0, 1, 2, 8):
            s, t, T = pairs[b]
            c, dd = icp.correspondences(torch.from_numpy(s), torch.from_numpy(t), T, r)
            c, dd = c.cpu().numpy(), dd.cpu().numpy()
            rows = np.flatnonzero(c >= 0)
            mine = dict(zip(corr[seg[b]:seg[b + 1], 0].tolist(), zip(corr[seg[b]:seg[b + 1], 1].tolist(), d2[seg[b]:seg[b + 1]].tolist())))
            assert len(rows) > 0 and all(mine[int(i)] == (int(c[i]), float(dd[i])) for i in rows)


def test_chunk_boundary_and_pair_independence():
    from eyoc_amd import matches
    pairs, r = cases.chunked()
    assert len(pairs) == 65
    corr, seg, status, d2 = _check("chunked", pairs, r)
    assert (np.diff(seg) > 0).all() and not status.any()            # offsets continue across the chunk boundary (pair 64 is checked above)
    rev = pairs[::-1]
    rcorr, rseg, _, rd2 = _run(rev, r)
    for b in (0, 1, 31, 63, 64):
        s, t, T = pairs[b]
        one, _, _, one_d2 = matches.matching_indices_batched([torch.from_numpy(s)], [torch.from_numpy(t)], T[None], r, collated=False,
                                                             return_d2=True)
        assert one.cpu().numpy().tobytes() == corr[seg[b]:seg[b + 1]].tobytes()
        assert one_d2.cpu().numpy().tobytes() == d2[seg[b]:seg[b + 1]].tobytes()
    for b in range(65):
        a = 64 - b
        assert rcorr[rseg[a]:rseg[a + 1]].tobytes() == corr[seg[b]:seg[b + 1]].tobytes()
        assert rd2[rseg[a]:rseg[a + 1]].tobytes() == d2[seg[b]:seg[b + 1]].tobytes()


def test_host_functions():
    import eyoc_amd
    from eyoc_amd import o3d
    pairs, r = cases.ragged()
    good = [pairs[b] for b in (0, 2, 8)]
    # two identical runs
    a, b = _run(pairs, r, collated=True), _run(pairs, r, collated=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # the collation, with the empty and faulty pairs in the batch
    ref, _ = _ref("ragged", pairs, r)
    want, want_seg = M.collate([p for p, _ in ref], [len(s) for s, _, _ in pairs], [len(t) for _, t, _ in pairs])
    assert np.array_equal(a[0], want) and a[1].tolist() == want_seg.tolist()
    # identity = no pose (the base stage)
    base = [(s, t, np.eye(4)) for s, t, _ in good]
    src, tgt, _ = _device(base)
    none = eyoc_amd.matching_indices_batched(src, tgt, None, r, collated=False)[0].cpu().numpy()
    assert np.array_equal(none, np.concatenate([M.brute(s, t, None, r)[0] for s, t, _ in base]))
    # the reference's per-pair signature: arrays, tensors, o3d point clouds
    s, t, T = pairs[0]
    for source, target in ((s, t), (torch.from_numpy(s), torch.from_numpy(t)), (o3d.PointCloud(s), o3d.PointCloud(t))):
        for K in (None, 2):
            got = eyoc_amd.get_matching_indices(source, target, T, r, K)
            assert got.dtype == torch.int64 and got.tolist() == M.brute(s, t, T, r, K)[0].tolist()
    # the overlap ratio, single and batched
    for s, t, T in good:
        assert eyoc_amd.compute_overlap_ratio(s, t, T, 0.3) == M.overlap_ratio(s, t, T, 0.3)
    src, tgt, Ts = _device(good)
    got = eyoc_amd.overlap_ratio_batched(src, tgt, Ts, 0.3).cpu().numpy()
    assert got.tolist() == [M.overlap_ratio(s, t, T, 0.3) for s, t, T in good]


def test_collated_pairs_through_the_loss():
    """The one existing consumer: the collated tensor as ``positive_pairs`` gives the two loss values of the restatement's pairs."""
    import eyoc_amd
    pairs, r = cases.ragged()
    good = [pairs[b] for b in (0, 2, 8)]
    src, tgt, Ts = _device(good)
    corr, seg, _ = eyoc_amd.matching_indices_batched(src, tgt, Ts, r)
    want, _ = M.collate([M.brute(s, t, T, r)[0] for s, t, T in good], [len(s) for s, _, _ in good], [len(t) for _, t, _ in good])
    assert np.array_equal(corr.cpu().numpy(), want)
    g = torch.Generator().manual_seed(3)
    F0 = torch.nn.functional.normalize(torch.randn(sum(len(s) for s, _, _ in good), 32, generator=g), dim=1).cuda()
    F1 = torch.nn.functional.normalize(torch.randn(sum(len(t) for _, t, _ in good), 32, generator=g), dim=1).cuda()
    out = []
    for pos in (corr, torch.from_numpy(want).cuda()):
        out.append([float(v) for v in eyoc_amd.contrastive_hardest_negative_loss(F0, F1, pos, rng=np.random.RandomState(11))])
    assert out[0] == out[1] and all(np.isfinite(out[0]))
