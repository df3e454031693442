"""Mutual nearest neighbours on the device (``eyoc_knn1_mutual`` / ``eyoc_mutual_compact``) against the restatement of
tests/mutual_restatement.py and against ``eyoc_knn1`` in both directions, byte for byte, on both routes; then the layers above: the
chunked Python calls, the Open3D-shaped call, and the registration pipeline with ``mutual_filter``."""
import types

import numpy as np
import pytest
import torch

import mutual_restatement as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _L():
    from eyoc_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _restore_knobs():
    L = _L()
    route, pre = L.knob("eyoc_knn_mutual_select", -2) - 2, L.knob("eyoc_knn_prefilter", -1)
    yield
    L.knob("eyoc_knn_mutual_select", route)
    L.knob("eyoc_knn_prefilter", pre)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device(A, B, seg_a, seg_b, dist_type, min_keep=0, route=None, prefilter=None):
    """The six outputs as numpy arrays, through the Python layer (chunking included)."""
    from eyoc_amd import eval as ev
    L = _L()
    if route is not None:
        L.knob("eyoc_knn_mutual_select", route)
    if prefilter is not None:
        L.knob("eyoc_knn_prefilter", prefilter)
    name = {v: k for k, v in M.DIST.items()}[dist_type]
    _, idx_ab, flags, idx_ba = ev._knn1_mutual_flags(_up(A), _up(B), seg_a, seg_b, name, True)
    rows, corr, seg_out = ev.mutual_compact_device(idx_ab, flags, seg_a, min_keep)
    seg_out = seg_out.cpu().numpy()
    m = int(seg_out[-1])
    return tuple(t.cpu().numpy() for t in (idx_ab, idx_ba, flags)) + (rows[:m].cpu().numpy(), corr[:m].cpu().numpy(), seg_out)


def _one_way(A, B, seg_a, seg_b, dist_type):
    from eyoc_amd.eval import knn1_segmented
    name = {v: k for k, v in M.DIST.items()}[dist_type]
    return knn1_segmented(_up(A), _up(B), seg_a, seg_b, name, return_distance=False).cpu().numpy()


CASES = [(na, nb, c) for na, nb in M.SHAPES for c in (M.WIDTHS if (na, nb) in M.WIDE_SHAPES else (32,))]


@pytest.mark.parametrize("na,nb,c", CASES, ids=[f"{a}x{b}x{c}" for a, b, c in CASES])
def test_both_routes_equal_the_one_way_queries_and_the_restatement(na, nb, c):
    A, B = M.pair_inputs(na, nb, c)
    sa, sb = [0, na], [0, nb]
    for dist_type in (0, 1, 2):
        want = M.search(A, B, sa, sb, dist_type)
        if min(na, nb) >= 32:
            assert 0.10 <= M.mutual_share(want[2]) <= 0.90
        for prefilter in ((0, 2) if c == 32 else (None,)):
            if prefilter is not None:
                _L().knob("eyoc_knn_prefilter", prefilter)
            ab, ba = _one_way(A, B, sa, sb, dist_type), _one_way(B, A, sb, sa, dist_type)
            for route in (0, 1):
                got = _device(A, B, sa, sb, dist_type, route=route)
                assert got[0].tobytes() == ab.tobytes() and got[1].tobytes() == ba.tobytes(), (dist_type, prefilter, route)
                M.check(got, A, B, sa, sb, dist_type)


@pytest.mark.parametrize("route", (0, 1))
def test_exact_duplicates_tie_to_the_lowest_index(route):
    A, B = M.pair_inputs(130, 70, 32, seed=1)
    B[37] = B[5]                                               # across a 32-target boundary
    A[3] = A[67] = B[5]                                        # across a 64-row tile: both at distance exactly 0 from targets 5 and 37
    for dist_type in (0, 1, 2):
        got = _device(A, B, [0, 130], [0, 70], dist_type, route=route)
        M.check(got, A, B, [0, 130], [0, 70], dist_type)
        idx_ab, idx_ba, flags = got[:3]
        assert idx_ab[3] == 5 and idx_ab[67] == 5 and idx_ba[5] == 3 and idx_ba[37] == 3
        assert flags[3] == 3 and flags[67] == 2               # only the lowest duplicate is mutual


@pytest.mark.parametrize("route", (0, 1))
def test_non_finite_rows(route):
    A, B = M.pair_inputs(70, 40, 32, seed=2)
    A[66, 7] = np.nan
    B[0, 3] = np.nan
    got = _device(A, B, [0, 70], [0, 40], 0, route=route)
    M.check(got, A, B, [0, 70], [0, 40], 0)
    assert got[0][66] == 0 and got[2][66] == 0 and got[1][0] == 0 and not (got[2][got[0] == 0] & 1).any()
    # rows of norm > 1 under GemmL2: NaN distances, the first one wins both ways
    A2, B2 = (3.0 * M.unit_rows(21, 70, 32)).astype(np.float32), (3.0 * M.unit_rows(22, 40, 32)).astype(np.float32)
    assert np.isnan(M.distance_matrix(A2, B2, 2)).any()
    got = _device(A2, B2, [0, 70], [0, 40], 2, route=route)
    M.check(got, A2, B2, [0, 70], [0, 40], 2)
    assert got[0].tobytes() == _one_way(A2, B2, [0, 70], [0, 40], 2).tobytes()
    assert got[1].tobytes() == _one_way(B2, A2, [0, 40], [0, 70], 2).tobytes()


@pytest.mark.parametrize("route", (0, 1))
def test_empty_segments_between_live_ones(route):
    na, nb = [70, 0, 40, 0, 65], [33, 20, 0, 0, 300]           # live, empty A, empty B, both empty, live
    sa, sb = np.concatenate([[0], np.cumsum(na)]), np.concatenate([[0], np.cumsum(nb)])
    A, B = M.pair_inputs(int(sa[-1]), int(sb[-1]), 32, seed=3)
    for min_keep in (0, 4):
        got = _device(A, B, sa, sb, 0, min_keep, route=route)
        M.check(got, A, B, sa, sb, 0, min_keep)
        for s in (0, 4):                                       # ... and equals the call on that segment alone
            one = _device(A[sa[s]:sa[s + 1]], B[sb[s]:sb[s + 1]], [0, na[s]], [0, nb[s]], 0, min_keep, route=route)
            assert np.array_equal(got[0][sa[s]:sa[s + 1]], one[0]) and np.array_equal(got[1][sb[s]:sb[s + 1]], one[1])
            assert np.array_equal(got[2][sa[s]:sa[s + 1]], one[2])
            assert np.array_equal(got[3][got[5][s]:got[5][s + 1]], one[3])


def test_130_segments_go_through_chunks():
    rng = np.random.default_rng(4)
    na, nb = rng.integers(0, 7, 130), rng.integers(0, 7, 130)
    sa, sb = np.concatenate([[0], np.cumsum(na)]), np.concatenate([[0], np.cumsum(nb)])
    A, B = M.pair_inputs(int(sa[-1]), int(sb[-1]), 32, seed=4)
    for route in (0, 1):
        for min_keep in (0, 3):
            M.check(_device(A, B, sa, sb, 0, min_keep, route=route), A, B, sa, sb, 0, min_keep)
    from eyoc_amd.eval import knn1_mutual_segmented, mutual_correspondences
    idx_ab, mutual, idx_ba = knn1_mutual_segmented(_up(A), _up(B), sa, sb, return_reverse=True)
    want = M.search(A, B, sa, sb, 0)
    assert mutual.dtype == torch.bool and np.array_equal(mutual.cpu().numpy(), (want[2] & 1) != 0)
    assert np.array_equal(idx_ab.cpu().numpy(), want[0]) and np.array_equal(idx_ba.cpu().numpy(), want[1])
    rows, corr, seg_out = mutual_correspondences(_up(A), _up(B), sa, sb, min_keep=3)
    M.check((None, None, None, rows.cpu().numpy(), corr.cpu().numpy(), seg_out), A, B, sa, sb, 0, 3)


@pytest.mark.parametrize("route", (0, 1))
def test_fallback_at_an_exact_count(route):
    for k, kept in ((2, None), (3, 4)):                        # 3 mutual rows < 4: every row stays; 4 mutual rows: those four
        A, B = M.fallback_case(k)
        got = _device(A, B, [0, len(A)], [0, len(B)], 0, 4, route=route)
        M.check(got, A, B, [0, len(A)], [0, len(B)], 0, 4)
        assert int((got[2] & 1).sum()) == k + 1
        assert got[5][1] == (len(A) if kept is None else kept)


# ---- the layers above

N_POINTS, HYP = 256, 20000


def _model():
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    sd = syn.make_weights()
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def three_pairs():
    from eyoc_amd import synthetic as syn
    return [syn.make_pair(40 + s, beams=16, azimuths=500, band=None) for s in range(3)]


def _batch(pairs, isolate=False):
    """Pair 2 is built to fall back: all of its target samples are ONE row with ONE planted descriptor, so every source row's nearest
    target is target 0 and exactly one correspondence is mutual."""
    from eyoc_amd.harness import DeviceBatch
    b = DeviceBatch(pairs, [40, 41, 42], torch.device("cuda"), n_points=N_POINTS, descriptor=dict(inlier_ratio=0.3), isolate=isolate)
    b.sel1.view(3, N_POINTS)[2] = b.sel1.view(3, N_POINTS)[2, 0].clone()
    b.G1.view(3, N_POINTS, -1)[2] = b.G1.view(3, N_POINTS, -1)[2, 0].clone()
    return b


def _cfg(**kw):
    from eyoc_amd.harness import RegistrationConfig
    return RegistrationConfig(ransac_max_iteration=HYP, n_points=N_POINTS, **kw)


def _by_hand(model, batch, seed):
    """The parent commit's API alone: forward, two one-way searches, a torch filter, the batched RANSAC on the kept rows."""
    from eyoc_amd import registration as reg
    from eyoc_amd.eval import knn1_segmented
    from eyoc_amd.harness import RegistrationPipeline
    plain = RegistrationPipeline(model, _cfg())
    with torch.no_grad():
        F, _ = plain._features(batch, None, sampled=True)
    F0, F1 = plain._sampled_halves(types.SimpleNamespace(batch=batch, F=F))
    seg = np.asarray(batch.seg)
    ab = knn1_segmented(F0, F1, seg, seg, "SquareL2", return_distance=False)
    ba = knn1_segmented(F1, F0, seg, seg, "SquareL2", return_distance=False)
    first = torch.repeat_interleave(_up(seg[:-1].astype(np.int64)), _up(np.diff(seg).astype(np.int64)))
    mutual = ba[ab + first] + first == torch.arange(len(ab), device=ab.device)         # (finite unit rows: every row has a neighbour)
    pair = torch.repeat_interleave(torch.arange(len(seg) - 1, device=ab.device), _up(np.diff(seg).astype(np.int64)))
    count = torch.zeros(len(seg) - 1, dtype=torch.int64, device=ab.device).index_add_(0, pair, mutual.to(torch.int64))
    keep = mutual | (count < 4)[pair]
    kept_seg = np.concatenate([[0], np.cumsum(torch.zeros(len(seg) - 1, dtype=torch.int64, device=ab.device)
                                              .index_add_(0, pair, keep.to(torch.int64)).cpu().numpy())])
    L = _L()
    prev = L.knob("eyoc_registration_accept_degenerate", 1)
    try:
        res = reg.ransac_batched_from_correspondences(batch.xyz0.reshape(-1, 3)[keep], batch.xyz1.reshape(-1, 3), ab[keep], kept_seg, seg,
                                                      0.3, HYP, seed=seed)
    finally:
        L.knob("eyoc_registration_accept_degenerate", prev)
    return res.cpu().numpy(), kept_seg, count.cpu().numpy()


def test_pipeline_register_and_enqueue_equal_the_hand_composed_route(three_pairs):
    from eyoc_amd.harness import RegistrationPipeline
    model, batch = _model(), _batch(three_pairs)
    want, kept_seg, count = _by_hand(model, batch, 7)
    assert count[2] < 4 and kept_seg[3] - kept_seg[2] == N_POINTS and (count[:2] >= 4).all()     # pair 2 fell back, the others did not
    assert (np.diff(kept_seg)[:2] < N_POINTS).all()
    pipe = RegistrationPipeline(model, _cfg(mutual_filter=True))
    dev = pipe.register(batch, seed=7, return_device=True).cpu().numpy()
    assert dev.tobytes() == want.tobytes()
    assert pipe.last_nn_idx.shape[0] == 3 * N_POINTS                                              # the full forward result stays
    results = pipe.register(batch, seed=7)
    for p, r in enumerate(results):
        assert r.fitness == r.inliers / max(int(kept_seg[p + 1] - kept_seg[p]), 1)
    for tail in (False, True):
        host, _ = pipe.enqueue(batch, seed=7, tail_stream=tail).wait()
        assert host.numpy().tobytes() == want.tobytes(), tail
    torch.cuda.synchronize()
    # icp_refine behind the filter: the ICP of the FULL sample sets started from the filtered route's poses - the hand-composed
    # records sent through icp_batched by hand (gate 2 voxels, 30 iterations: the config's defaults), byte for byte
    from eyoc_amd import icp
    got = RegistrationPipeline(model, _cfg(mutual_filter=True, icp_refine=True)).register(batch, seed=7, return_device=True)
    T0 = torch.from_numpy(want.copy()).to(DEV).view(torch.float32)[:, :16]
    rec = icp.icp_batched(batch.xyz0.reshape(-1, 3), batch.xyz1.reshape(-1, 3), batch.seg, batch.seg, 0.6, T0.to(torch.float64), 30)
    T1 = rec.view(torch.float64)[:, :16].to(torch.float32)
    assert torch.isfinite(T1[:2]).all()                                                     # (pair 2 matches nonsense: any pose)
    assert got.view(torch.float32)[:, :16].cpu().numpy().tobytes() == T1.cpu().numpy().tobytes()
    assert got.cpu().numpy()[:, 64:].tobytes() == want[:, 64:].tobytes()                       # counts and rmse stay the back-end's


def test_pipeline_with_a_dropped_pair(three_pairs):
    from eyoc_amd import harness as h
    pairs = [dict(p) for p in three_pairs]
    for k in ("coords0", "feats0", "xyz0"):                    # pair 1: a duplicated row fails its map build
        pairs[1][k] = np.concatenate([pairs[1][k], pairs[1][k][10:11]])
    model, batch = _model(), _batch(pairs, isolate=True)
    pipe = h.RegistrationPipeline(model, _cfg(mutual_filter=True, isolate_failures=True))
    got = pipe.register(batch, seed=7, return_device=True).cpu().numpy()
    reduced = pipe.registered_batch
    assert reduced.dropped.tolist() == [0, h.DROPPED_DUPLICATE, 0]
    want, kept_seg, _ = _by_hand(model, reduced, 7)
    assert kept_seg[2] == kept_seg[1] and got.tobytes() == want.tobytes()
    host, _ = pipe.enqueue(batch, seed=7).wait()
    assert host.numpy().tobytes() == want.tobytes()


def test_shim_with_mutual_filter():
    import eyoc_amd.o3d as o3d
    from eyoc_amd import registration as reg
    from eyoc_amd.eval import mutual_correspondences
    rng = np.random.default_rng(11)
    n = 300
    F1 = M.unit_rows(12, n, 32)
    F0 = F1[rng.integers(0, n, n)] + 0.35 * M.unit_rows(13, n, 32)      # several source rows per target: one of them is mutual
    F0 = (F0 / np.linalg.norm(F0, axis=1, keepdims=True)).astype(np.float32)
    x0, x1 = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    rows, corr, seg = mutual_correspondences(_up(F0), _up(F1), [0, n], [0, n], min_keep=4)
    assert 4 <= seg[1] < n
    want = reg.ransac_from_correspondences(_up(x0)[rows], _up(x1), corr, 0.3, HYP, seed=3)
    r = o3d.pipelines.registration
    pc = []
    for x in (x0, x1):
        p = o3d.geometry.PointCloud()
        p.points = o3d.utility.Vector3dVector(x.astype(np.float64))
        pc.append(p)
    fs = []
    for F in (F0, F1):
        f = r.Feature()
        f.data = np.ascontiguousarray(F.T, np.float64)
        fs.append(f)
    got = r.registration_ransac_based_on_feature_matching(
        pc[0], pc[1], fs[0], fs[1], True, 0.3, r.TransformationEstimationPointToPoint(False), 4,
        [r.CorrespondenceCheckerBasedOnEdgeLength(0.9), r.CorrespondenceCheckerBasedOnDistance(0.3)],
        r.RANSACConvergenceCriteria(HYP, 10000), seed=3)
    assert got.transformation.tobytes() == want.transformation.tobytes() and got.inliers == want.inliers
    assert got.fitness == want.fitness == want.inliers / max(int(seg[1]), 1)


def test_matcher_keyword():
    from eyoc_amd import registration as reg
    n = 200
    S, T = M.pair_inputs(n, n + 20, 32, seed=6)
    kp0, kp1 = _up(np.random.default_rng(1).normal(size=(1, n, 3)).astype(np.float32)), _up(np.random.default_rng(2).normal(size=(1, n + 20, 3)).astype(np.float32))
    m = reg.Matcher(num_node="all", use_mutual=True)
    a, b = m.match_pair(kp0, kp1, _up(S)[None], _up(T)[None])
    assert a.shape[1] == n                                       # use_mutual stays inert
    idx_ab, _, flags = M.segment(S, T, 2)
    rows = np.flatnonzero(flags & 1)
    a, b = m.match_pair(kp0, kp1, _up(S)[None], _up(T)[None], mutual=True)
    assert np.array_equal(a.cpu().numpy(), kp0.cpu().numpy()[:, rows]) and np.array_equal(b.cpu().numpy(), kp1.cpu().numpy()[:, idx_ab[rows]])


def test_config_refuses_sc2pcr():
    from eyoc_amd.harness import RegistrationConfig
    with pytest.raises(ValueError):
        RegistrationConfig(use_RANSAC=False, mutual_filter=True)
