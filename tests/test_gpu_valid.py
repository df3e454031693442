"""GPU: the batched validation step - ``eyoc_irls_quad_batched`` against ``eyoc_irls_quad`` byte for byte, ``eyoc_valid_metrics_batched``
against its fp64 restatement and the reference's outputs (``g12_valid.npz``), and ``RegistrationPipeline.validate`` end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _inputs as gi
from valid_restatement import check_against_g12, g12_cases, valid_record

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 5000]      # around a wave, around one 1024-row sweep, several sweeps
T_TRUE = gi.rigid(0.02, -0.01, 0.12, 1.5, -0.4, 0.1)


def _golden(name):
    return np.load(os.path.join(os.path.dirname(__file__), "golden", name))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _pairs(sizes, seed0):
    """-> per pair (p0, p1, w) on the device."""
    out = []
    for b, n in enumerate(sizes):
        p0, p1, _ = gi.corr_case(seed0 + 4 * b, n, T_TRUE, 0.8, noise=0.04)
        w = (0.05 + 0.95 * gi._u(seed0 + 4 * b + 3, n)).astype(np.float32)
        out.append(tuple(torch.from_numpy(a).cuda() for a in (p0, p1, w)))
    return out


def _seg(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _batched(pairs, order, weights, iters):
    import eyoc_amd
    P0 = torch.cat([pairs[b][0] for b in order])
    P1 = torch.cat([pairs[b][1] for b in order])
    W = torch.cat([pairs[b][2] for b in order]) if weights else None
    return eyoc_amd.est_quad_linear_robust_batched(P0, P1, _seg([len(pairs[b][0]) for b in order]), weight=W, iters=iters)


@pytest.fixture(scope="module")
def sized_pairs():
    return _pairs(SIZES, 300)


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("iters", [0, 1, 20])
def test_batched_irls_equals_single_byte_for_byte(sized_pairs, weights, iters):
    import eyoc_amd
    single = [_bits(eyoc_amd.est_quad_linear_robust(p0, p1, w if weights else None, iters=iters)) for p0, p1, w in sized_pairs]
    order = list(range(len(SIZES)))
    for o in (order, order[::-1]):
        T = _batched(sized_pairs, o, weights, iters)
        assert T.is_cuda and T.shape == (len(SIZES), 4, 4) and T.dtype == torch.float32
        got = _bits(T)
        for k, b in enumerate(o):
            np.testing.assert_array_equal(got[k], single[b], err_msg=f"pair of {SIZES[b]} rows at slot {k}")
    if iters == 20:     # the large pairs are solved as well (1 and 2 rows are singular: NaN from both kernels alike)
        ok = [b for b, n in enumerate(SIZES) if n >= 1023]
        np.testing.assert_allclose(_batched(sized_pairs, order, weights, iters).cpu().numpy()[ok], np.tile(T_TRUE, (len(ok), 1, 1)), atol=0.05)


def test_batched_irls_130_tiny_segments_cross_the_launch_chunk():
    import eyoc_amd
    sizes = [3 + (b * 37) % 198 for b in range(130)]
    assert min(sizes) == 3 and max(sizes) == 200
    pairs = _pairs(sizes, 900)
    T = _bits(_batched(pairs, list(range(130)), True, 20))
    for b, (p0, p1, w) in enumerate(pairs):
        np.testing.assert_array_equal(T[b], _bits(eyoc_amd.est_quad_linear_robust(p0, p1, w)), err_msg=f"pair {b}, {sizes[b]} rows")


def _gather_case():
    """Three pairs whose p1 segments differ in length from their correspondences; idx1 maps into them with repeats."""
    rng = np.random.default_rng(5)
    n0, n1 = [700, 1300, 90], [400, 2100, 91]
    pairs = _pairs(n1, 500)
    p0 = [torch.from_numpy(((gi._u(600 + b, n, 3) - 0.5) * 40).astype(np.float32)).cuda() for b, n in enumerate(n0)]
    idx = [torch.from_numpy(rng.integers(0, m, n)).cuda() for n, m in zip(n0, n1)]
    assert all(len(np.unique(i.cpu().numpy())) < len(i) for i in idx[:2])
    return n0, n1, p0, [p[1] for p in pairs], idx


def test_fused_gather_equals_pregathered_call():
    import eyoc_amd
    n0, n1, p0, p1, idx = _gather_case()
    fused = eyoc_amd.est_quad_linear_robust_batched(torch.cat(p0), torch.cat(p1), _seg(n0), _seg(n1), idx1=torch.cat(idx))
    plain = eyoc_amd.est_quad_linear_robust_batched(torch.cat(p0), torch.cat([q[i] for q, i in zip(p1, idx)]), _seg(n0))
    np.testing.assert_array_equal(_bits(fused), _bits(plain))
    assert np.isfinite(fused.cpu().numpy()).all()
    for b in range(3):
        np.testing.assert_array_equal(_bits(fused[b]), _bits(eyoc_amd.est_quad_linear_robust(p0[b], p1[b][idx[b]])))


def test_five_g2_cases_in_one_call():
    import eyoc_amd
    g = _golden("g2_irls.npz")
    P0, P1, W, lens = [], [], [], []
    for seed, n, frac, use_w, tp in json.loads(str(g["cases"])):
        p0, p1, _ = gi.corr_case(seed, n, gi.rigid(*tp), frac)
        w = (0.05 + 0.95 * gi._u(seed + 9, n, 1)).astype(np.float32).reshape(-1) if use_w else np.ones(n, np.float32)   # (no weight = weight 1)
        P0.append(p0); P1.append(p1); W.append(w); lens.append(n)
    T = eyoc_amd.est_quad_linear_robust_batched(np.concatenate(P0), np.concatenate(P1), _seg(lens), weight=np.concatenate(W)).cpu().numpy()
    for i in range(len(lens)):
        print(f"g2 case {i}: max |T - T_ref| = {np.abs(T[i] - g[f'T{i}']).max():.2e}")
        np.testing.assert_allclose(T[i], g[f"T{i}"], rtol=0, atol=1e-4, err_msg=f"case {i}")


def _metrics(p0, p1, seg0, seg1, idx1, x0, segx, T_est, T_gt, thresh=0.1):
    import eyoc_amd
    raw = eyoc_amd.valid_metrics_batched(p0, p1, seg0, seg1, idx1, x0, segx, T_est, T_gt, thresh).cpu().numpy()
    return raw, eyoc_amd.decode_valid_records(raw)


def test_empty_segment_between_live_ones():
    import eyoc_amd
    from eyoc_amd import validate as V
    pairs = _pairs([100, 200], 700)
    (a0, a1, _), (b0, b1, _) = pairs
    x0 = torch.cat([a0, b0])
    Tg = torch.from_numpy(np.stack([T_TRUE, T_TRUE, T_TRUE]).astype(np.float32))
    T3 = eyoc_amd.est_quad_linear_robust_batched(torch.cat([a0, b0]), torch.cat([a1, b1]), [0, 100, 100, 300])
    T2 = eyoc_amd.est_quad_linear_robust_batched(torch.cat([a0, b0]), torch.cat([a1, b1]), [0, 100, 300])
    assert np.isnan(T3[1].cpu().numpy()).all()
    np.testing.assert_array_equal(_bits(T3[[0, 2]]), _bits(T2))
    raw3, r3 = _metrics(torch.cat([a0, b0]), torch.cat([a1, b1]), [0, 100, 100, 300], None, None, x0, [0, 100, 100, 300], T3, Tg)
    raw2, r2 = _metrics(torch.cat([a0, b0]), torch.cat([a1, b1]), [0, 100, 300], None, None, x0, [0, 100, 300], T2, Tg[:2])
    assert r3["status"].tolist() == [0, V.EMPTY | V.POSE_NONFINITE, 0]
    assert np.isnan(r3["hit_ratio"][1]) and np.isnan(r3["loss"][1]) and r3["n_corr"][1] == 0 and r3["hits"][1] == 0
    assert raw3[[0, 2]].tobytes() == raw2.tobytes()
    # EMPTY alone: a finite pose handed to a pair without correspondences (and with a cloud) still has no ratio and no loss
    _, r = _metrics(torch.cat([a0, b0]), torch.cat([a1, b1]), [0, 100, 100, 300], None, None, torch.cat([a0, a0, b0]), [0, 100, 200, 400], Tg, Tg)
    assert r["status"].tolist() == [0, V.EMPTY, 0] and np.isnan(r["loss"][1]) and r["rte"][1] == 0.0 and r["n_points"][1] == 100
    # an all-empty batch is still a call
    assert np.isnan(eyoc_amd.est_quad_linear_robust_batched(a0[:0], a1[:0], [0, 0, 0]).cpu().numpy()).all()


@pytest.mark.parametrize("bad", ["minus_one", "len"])
def test_bad_index_marks_its_pair_only(bad):
    """The bad index sits in the middle pair of three (neither the first nor the last), so even an unclamped load would stay inside the
    tensor."""
    import eyoc_amd
    from eyoc_amd import validate as V
    n0, n1, p0, p1, idx = _gather_case()
    P0, P1, s0, s1 = torch.cat(p0), torch.cat(p1), _seg(n0), _seg(n1)
    Tg = torch.from_numpy(np.stack([T_TRUE] * 3).astype(np.float32))
    clean_T = eyoc_amd.est_quad_linear_robust_batched(P0, P1, s0, s1, idx1=torch.cat(idx))
    clean_raw, _ = _metrics(P0, P1, s0, s1, torch.cat(idx), P0, s0, clean_T, Tg, 5.0)
    broken = [i.clone() for i in idx]
    broken[1][77] = -1 if bad == "minus_one" else n1[1]
    T = eyoc_amd.est_quad_linear_robust_batched(P0, P1, s0, s1, idx1=torch.cat(broken))
    assert np.isnan(T[1].cpu().numpy()).all()
    np.testing.assert_array_equal(_bits(T[[0, 2]]), _bits(clean_T[[0, 2]]))
    raw, r = _metrics(P0, P1, s0, s1, torch.cat(broken), P0, s0, clean_T, Tg, 5.0)       # the clean poses: BAD_INDEX and nothing else
    assert r["status"].tolist() == [0, V.BAD_INDEX, 0]
    assert np.isnan(r["hit_ratio"][1]) and r["hits"][1] == 0 and r["n_corr"][1] == n0[1] and np.isfinite(r["loss"][1])
    assert raw[[0, 2]].tobytes() == clean_raw[[0, 2]].tobytes()
    _, r = _metrics(P0, P1, s0, s1, torch.cat(broken), P0, s0, T, Tg, 5.0)               # the poses the IRLS call left
    assert r["status"].tolist() == [0, V.BAD_INDEX | V.POSE_NONFINITE, 0]


def test_invalid_arguments_are_refused():
    import eyoc_amd
    from eyoc_amd import _lib
    p = torch.zeros((8, 3), device="cuda")
    T = torch.zeros((4, 16), device="cuda")
    rec = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    seg = lambda *v: (C.c_int32 * len(v))(*v)                                  # noqa: E731
    lib, ctx = _lib.load(), _lib.ctx(0)

    def irls(s0, s1, nseg, idx=None):
        return lib.eyoc_irls_quad_batched(ctx, _lib.ptr(p), _lib.ptr(p), idx, None, s0, s1, nseg, 20, _lib.ptr(T), _lib.stream_ptr())

    def metrics(s0, s1, sx, nseg, idx=None):
        return lib.eyoc_valid_metrics_batched(ctx, _lib.ptr(p), _lib.ptr(p), idx, s0, s1, _lib.ptr(p), sx, nseg, _lib.ptr(T), _lib.ptr(T), 0.1, 1.0,
                                              _lib.ptr(rec), _lib.stream_ptr())
    ok, idx = seg(0, 4, 8), _lib.ptr(torch.zeros(8, dtype=torch.int64, device="cuda"))
    assert irls(ok, ok, 2) == 0 and metrics(ok, ok, ok, 2) == 0
    assert irls(ok, ok, 0) == _lib.ERR_INVALID and metrics(ok, ok, ok, 0) == _lib.ERR_INVALID
    assert irls(seg(0, 5, 3, 8), seg(0, 5, 3, 8), 3) == _lib.ERR_INVALID                    # decreasing offsets
    assert metrics(ok, ok, seg(0, 5, 3), 2) == _lib.ERR_INVALID
    assert irls(ok, seg(0, 5, 8), 2) == _lib.ERR_INVALID and irls(ok, seg(0, 5, 8), 2, idx) == 0    # differing segments need idx1
    assert metrics(ok, seg(0, 5, 8), ok, 2) == _lib.ERR_INVALID and metrics(ok, seg(0, 5, 8), ok, 2, idx) == 0
    with pytest.raises(eyoc_amd.EyocError) as ei:                                            # 1025 pairs
        eyoc_amd.est_quad_linear_robust_batched(p[:0], p[:0], [0] * 1026)
    assert ei.value.code == _lib.ERR_INVALID
    torch.cuda.synchronize()


# ---- the metrics

@pytest.fixture(scope="module")
def g12():
    return _golden("g12_valid.npz")


@pytest.fixture(scope="module")
def metric_pairs(g12):
    """The twelve g12 pairs, then four pairs whose full clouds have 1, 1023, 1025 and 30 000 rows (a pose a little off the truth) ->
    (per pair (p0, p1, x0, T_est, T_gt), the device's raw records of ONE call over all of them, decoded)."""
    pairs = [(p0, p1, x0, T_est, T_gt) for _, _, p0, p1, x0, T_est, T_gt in g12_cases(g12)]
    for k, nx in enumerate((1, 1023, 1025, 30000)):
        p0, p1, _ = gi.corr_case(800 + k, 300 + k, T_TRUE, 0.7, noise=0.04)
        x0 = ((gi._u(810 + k, nx, 3) - 0.5) * np.array((60.0, 60.0, 6.0))).astype(np.float32)
        T_est = (T_TRUE @ gi.rigid(0.001 * k, 0.002, -0.003, 0.05, -0.02 * k, 0.01)).astype(np.float32)
        pairs.append((p0, p1, x0, T_est, T_TRUE.astype(np.float32)))
    raw, rec = _call(pairs)
    return pairs, raw, rec


def _call(pairs):
    return _metrics(np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]), _seg([len(p[0]) for p in pairs]), None, None,
                    np.concatenate([p[2] for p in pairs]), _seg([len(p[2]) for p in pairs]), np.stack([p[3] for p in pairs]),
                    np.stack([p[4] for p in pairs]))


def test_metrics_equal_the_fp64_restatement(metric_pairs):
    pairs, raw, rec = metric_pairs
    assert raw.shape == (16, 64) and rec["n_points"].tolist()[12:] == [1, 1023, 1025, 30000]
    for b, (p0, p1, x0, T_est, T_gt) in enumerate(pairs):
        want = valid_record(p0, p1, None, x0, T_est, T_gt)
        got = rec[b]
        print(f"pair {b}: loss {got['loss']:.12g} / {want['loss']:.12g}  cos - 1 {got['cos_rre'] - 1:.3e} / {want['cos_rre'] - 1:.3e}  "
              f"rre {got['rre']:.9g} / {want['rre']:.9g}  hits {got['hits']} / {want['hits']}")
        for k in ("hits", "n_corr", "n_points", "status"):
            assert int(got[k]) == want[k], (b, k)
        assert got["hit_ratio"] == want["hit_ratio"] and got["reserved"] == 0.0
        for k in ("loss", "rte", "cos_rre"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-10, atol=0, err_msg=f"pair {b} {k}")
        assert np.isnan(got["rre"]) == np.isnan(want["rre"]), b
        if not np.isnan(want["rre"]):
            # a cosine within rtol 1e-10 moves its arc cosine by 1e-10 / sin(rre) at the most (acos itself: a few ulps)
            assert abs(got["rre"] - want["rre"]) <= 1e-10 / max(np.sin(want["rre"]), 1e-8) + 1e-12, b
    assert np.isnan(rec["rre"]).any(), "the fixture holds a cosine above 1 (the reference's own rre is NaN there)"


def test_a_record_is_the_same_bytes_alone_and_in_the_batch(metric_pairs):
    pairs, raw, _ = metric_pairs
    for b in range(len(pairs)):
        alone, _ = _call(pairs[b:b + 1])
        assert alone.tobytes() == raw[b].tobytes(), b
    again, _ = _call(pairs)
    assert again.tobytes() == raw.tobytes()


def test_metrics_against_the_reference_fixture(g12, metric_pairs):
    _, _, rec = metric_pairs
    for b, (c, v, p0, *_rest) in enumerate(g12_cases(g12)):
        r = rec[b]
        print(f"g12 case {c} variant {v}: loss {r['loss']:.9f} ref {g12['loss'][c, v]:.9f}  rte {r['rte']:.7f} ref {g12['rte'][c, v]:.7f}  "
              f"rre {r['rre']:.7f} ref {g12['rre'][c, v]:.7f}  hits {r['hits']}")
        assert r["status"] == 0
        check_against_g12(g12, c, v, r, len(p0))
        assert r["hit_ratio"] == pytest.approx(float(g12["hit_ratio"][c, v]), abs=1e-6)


def test_batched_irls_reaches_the_reference_poses_of_g12(g12):
    """The poses the fixture's metrics were computed on are the reference's ``est_quad_linear_robust`` outputs: the batched solver,
    all six pairs in one call, within the project's pose bar of them (three points fit their noise: ill-conditioned, left out)."""
    import eyoc_amd
    cases = [c for c in g12_cases(g12) if c[1] == 0]
    T = eyoc_amd.est_quad_linear_robust_batched(np.concatenate([c[2] for c in cases]), np.concatenate([c[3] for c in cases]),
                                                _seg([len(c[2]) for c in cases])).cpu().numpy()
    for k, c in enumerate(cases):
        if len(c[2]) >= 64:
            np.testing.assert_allclose(T[k], c[5], rtol=0, atol=1e-4, err_msg=f"case {k}")


# ---- the step, end to end

N_POINTS = 1000


@pytest.fixture(scope="module")
def scene():
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    pairs = [syn.make_pair(s, beams=32, azimuths=1000, band=None) for s in (11, 12, 13)]
    sd = syn.make_weights()
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return pairs, m.cuda().eval()


def test_validate_end_to_end(scene):
    import eyoc_amd
    from eyoc_amd import harness as h
    from eyoc_amd import validate as V
    pairs, model = scene
    dev = torch.device("cuda")
    batch = h.DeviceBatch(pairs, [21, 22, 23], dev, n_points=N_POINTS)
    pcd0 = [p["xyz0"] for p in pairs]
    pipe = h.RegistrationPipeline(model, h.RegistrationConfig(n_points=N_POINTS))
    step = pipe.validate(batch, pcd0=pcd0)
    assert isinstance(step, V.ValidStep) and step.T_est.is_cuda and step.T_est.shape == (3, 4, 4) and step.records.shape == (3,)

    # the per-pair route built from existing calls: full features, rows at sel0 / sel1, find_nn_gpu, est_quad_linear_robust
    F = pipe.features(batch).F
    x0, x1 = batch.xyz0.cpu().numpy(), batch.xyz1.cpu().numpy()
    meters = V.ValidMeters()
    for b in range(3):
        rows = slice(b * N_POINTS, (b + 1) * N_POINTS)
        nn = eyoc_amd.find_nn_gpu(F[batch.sel0[rows]], F[batch.sel1[rows]])
        np.testing.assert_array_equal(step.nn_idx[rows].cpu().numpy(), nn.numpy())
        T = eyoc_amd.est_quad_linear_robust(batch.xyz0[b], batch.xyz1[b][nn.to(dev)])
        np.testing.assert_array_equal(_bits(step.T_est[b]), _bits(T), err_msg=f"pair {b}")
        want = valid_record(x0[b], x1[b], nn.numpy(), pcd0[b], T.cpu().numpy(), batch.T_gt[b])
        got = step.records[b]
        for k in ("hits", "n_corr", "n_points", "status"):
            assert int(got[k]) == want[k], (b, k)
        assert got["n_corr"] == N_POINTS and got["n_points"] == len(pcd0[b])
        for k in ("loss", "rte", "cos_rre"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-10, atol=0, err_msg=f"pair {b} {k}")
        assert np.isnan(got["rre"]) == np.isnan(want["rre"])
        meters.update(got)
    whole = V.ValidMeters()
    whole.update(step.records)
    assert whole.summary() == meters.summary() and whole.skipped == 0
    assert V.valid_epoch(pipe, [batch], pcd0=lambda k, b: pcd0) == meters.summary()
    # pcd0 = None: the sample set stands in for the full cloud; the packed form of pcd0 is the list's
    assert pipe.validate(batch).records["n_points"].tolist() == [N_POINTS] * 3
    packed = (np.concatenate(pcd0), _seg([len(c) for c in pcd0]))
    assert pipe.validate(batch, pcd0=packed).records.tobytes() == step.records.tobytes()

    # isolate_failures with pair 1 dropped: EMPTY, skipped, and the other two records keep their bytes
    ipipe = h.RegistrationPipeline(model, h.RegistrationConfig(n_points=N_POINTS, isolate_failures=True))
    dropped = ipipe.validate(batch.without_pairs({1: h.DROPPED_RANGE}), pcd0=pcd0)
    assert dropped.records["status"][1] & V.EMPTY and np.isnan(dropped.T_est[1].cpu().numpy()).all()
    assert dropped.records[[0, 2]].tobytes() == step.records[[0, 2]].tobytes()
    np.testing.assert_array_equal(_bits(dropped.T_est[[0, 2]]), _bits(step.T_est[[0, 2]]))
    m = V.ValidMeters()
    m.update(dropped.records)
    assert m.skipped == 1 and m.count == 2
