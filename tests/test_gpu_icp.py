"""Batched point-to-point ICP on the GPU (csrc/icp.hip, eyoc_amd/icp.py) against the CPU restatement of its contract
(tests/icp_restatement.py), on ``synthetic.make_pair`` inputs.

Bounds, none of them tuned on the kernel's output:
* B = 4e-12 m^2 for a single evaluation: fp32 inputs are exact in fp64, a posed component carries <= 6 roundings at magnitude <= 256 m
  (1.7e-13 m), so two correct fp64 evaluations differ by at most 2 * 2 r sqrt(3) * 1.7e-13 ~ 1.1e-12 m^2 for r <= 1 m; B leaves a
  factor 4.  A row whose decision is closer than B to flipping in the restatement (runner-up d2 - best d2, |d2 - r^2|) is excused;
  at most 1e-5 of the rows may be.
* whole runs: every entry of T within 1e-4 (the project's pose bar), inlier_rmse within 1e-4 m, equal iteration count,
  CONVERGED bit and correspondence count - the count may differ by the number of rows within 1e-8 m^2 of the gate under the
  restatement's final T.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import icp_restatement as R

pytestmark = pytest.mark.gpu

B = 4e-12
GATE_BAND = 1e-8


@functools.lru_cache(maxsize=None)
def _pair(seed):
    from eyoc_amd import synthetic as syn
    return syn.make_pair(seed, keep_raw=True)


@functools.lru_cache(maxsize=None)
def _case(seed, kind):
    """-> (src f32 [n, 3], tgt f32 [m, 3], init f64 [4, 4]): ``kind`` = "samples" (the harness's two 5000-point draws) or "5cm" (the raw
    sweeps voxelised at 5 cm, ~100 k points each)."""
    from eyoc_amd import harness as h
    from eyoc_amd import synthetic as syn
    p = _pair(seed)
    T0 = R.perturb(np.asarray(p["T_gt"], np.float64), np.random.default_rng(seed), 1.0, 0.2)
    if kind == "samples":
        i0 = h.sample_indices(seed, 0, len(p["xyz0"]), 5000)
        i1 = h.sample_indices(seed, 1, len(p["xyz1"]), 5000)
        return np.ascontiguousarray(p["xyz0"][i0], np.float32), np.ascontiguousarray(p["xyz1"][i1], np.float32), T0
    x0 = p["raw0"][syn.voxelize(p["raw0"], 0.05)[0]]
    x1 = p["raw1"][syn.voxelize(p["raw1"], 0.05)[0]]
    return np.ascontiguousarray(x0[:, :3], np.float32), np.ascontiguousarray(x1[:, :3], np.float32), T0


@functools.lru_cache(maxsize=None)
def _restated(seed, kind, gate):
    src, tgt, T0 = _case(seed, kind)
    return R.icp(src, tgt, gate, T0, 30)


CASES = [(s, "samples", g) for s in (0, 1, 2) for g in (0.3, 0.6)] + [(s, "5cm", 0.2) for s in (0, 1, 2)]


def _decode(res):
    from eyoc_amd import icp
    return [icp.decode_icp_result(r) for r in res.cpu()]


# ---- 1. one evaluation, row for row

@pytest.mark.parametrize("seed,kind,gate", CASES)
def test_one_evaluation_row_for_row(seed, kind, gate):
    from eyoc_amd import icp
    src, tgt, _ = _case(seed, kind)
    run = _restated(seed, kind, gate)
    for k in sorted({0, min(5, run.iterations), run.iterations}):
        T = run.trajectory[k]
        want = R.evaluate(src, tgt, T, gate)
        corr, d2, rec = icp.correspondences(src, tgt, T, gate, return_records=True)
        corr, d2 = corr.cpu().numpy(), d2.cpu().numpy()
        excused = want.margin < B
        print(f"seed {seed} {kind} gate {gate} T_{k}: {int(excused.sum())} rows excused of {len(src)}, smallest margin {want.margin.min():.3e} m^2")
        assert excused.sum() <= 1e-5 * len(src), "the inputs of this case are too close to a tie for a row-for-row comparison"
        ok = ~excused
        np.testing.assert_array_equal(corr[ok], want.corr[ok])
        hit = ok & (want.corr >= 0)
        err = np.abs(d2[hit] - want.d2[hit]).max()
        print(f"    max |d2 - restatement| = {err:.3e} m^2 over {int(hit.sum())} correspondences")
        assert err <= B
        assert np.isinf(d2[ok & (want.corr < 0)]).all()
        r = _decode(rec)[0]
        assert r.iterations == 0 and r.status == 0 and np.array_equal(r.transformation, T)
        if not excused.any():
            assert r.inliers == int((want.corr >= 0).sum()) and r.fitness == want.fitness
            assert abs(r.inlier_rmse - want.inlier_rmse) < 1e-9


# ---- 2. whole runs

def check_whole_run(got, want, src, tgt, gate, what=""):
    """A decoded device run (with its correspondence set) against the restated run of the same inputs, under the module's bounds."""
    from eyoc_amd import icp
    # best d2 of every row up to just beyond the gate (a wider gate keeps the rows right above it too)
    near_gate = int((np.abs(R.evaluate(src, tgt, want.T, np.sqrt(gate * gate + 2 * GATE_BAND)).d2 - gate * gate) < GATE_BAND).sum())
    dT = np.abs(got.transformation - want.T).max()
    print(f"{what}: iterations {got.iterations} / {want.iterations}, status {got.status} / {want.status}, max |dT| "
          f"{dT:.3e}, d rmse {abs(got.inlier_rmse - want.inlier_rmse):.3e}, correspondences {got.inliers} / {want.correspondences} "
          f"({near_gate} rows within {GATE_BAND} m^2 of the gate)")
    assert got.iterations == want.iterations
    assert (got.status & icp.CONVERGED) == (want.status & R.CONVERGED) and got.status == want.status
    assert dT < 1e-4
    assert abs(got.inlier_rmse - want.inlier_rmse) < 1e-4
    assert abs(got.inliers - want.correspondences) <= near_gate
    assert abs(got.fitness - got.inliers / len(src)) < 1e-15
    assert got.correspondence_set.shape == (got.inliers, 2)
    if near_gate == 0:
        np.testing.assert_array_equal(got.correspondence_set[:, 0], np.flatnonzero(want.last.corr >= 0))


@pytest.mark.parametrize("seed,kind,gate", CASES + [(3, "samples", 0.6)])
def test_whole_run_matches_the_restatement(seed, kind, gate):
    from eyoc_amd import icp
    src, tgt, T0 = _case(seed, kind)
    want = _restated(seed, kind, gate)
    res, corr = icp.icp_batched(src, tgt, [0, len(src)], [0, len(tgt)], gate, T0[None], 30, return_correspondences=True)
    got = icp.decode_icp_result(res[0], corr)
    check_whole_run(got, want, src, tgt, gate, f"seed {seed} {kind} gate {gate}")
    if (seed, kind, gate) == (3, "samples", 0.6):
        assert want.status & R.CONVERGED and want.iterations < 30        # the case the issue names: it stops early


# ---- 3. batch invariance and reproducibility

def _eight():
    """8 pairs with segments that are no multiples of the workgroup's 256 rows -> packed clouds, segments, inits."""
    srcs, tgts, inits = [], [], []
    for b in range(8):
        s, t, T0 = _case(b % 4, "samples")
        n, m = 5000 - 311 * b, 5000 - 97 * (7 - b)
        srcs.append(s[:n]); tgts.append(t[:m])
        inits.append(R.perturb(T0, np.random.default_rng(100 + b), 0.3, 0.05) if b >= 4 else T0)
    seg_s = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    seg_t = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
    return srcs, tgts, np.stack(inits), seg_s, seg_t


def test_batch_invariance_and_reproducibility():
    from eyoc_amd import icp
    srcs, tgts, inits, seg_s, seg_t = _eight()
    S, T = np.concatenate(srcs), np.concatenate(tgts)
    a, ca = icp.icp_batched(S, T, seg_s, seg_t, 0.6, inits, 30, return_correspondences=True)
    b, cb = icp.icp_batched(S, T, seg_s, seg_t, 0.6, inits, 30, return_correspondences=True)
    a, ca = a.cpu().numpy(), ca.cpu().numpy()
    assert a.tobytes() == b.cpu().numpy().tobytes() and ca.tobytes() == cb.cpu().numpy().tobytes()
    its = []
    for p in range(8):
        one, c1 = icp.icp_batched(srcs[p], tgts[p], [0, len(srcs[p])], [0, len(tgts[p])], 0.6, inits[p][None], 30,
                                  return_correspondences=True)
        assert one.cpu().numpy().tobytes() == a[p].tobytes(), p
        assert c1.cpu().numpy().tobytes() == ca[seg_s[p]:seg_s[p + 1]].tobytes(), p
        its.append(icp.decode_icp_result(one[0]).iterations)
    print("iterations per pair:", its)
    assert min(its) >= 1


def test_more_pairs_than_one_launch_set_holds():
    """70 pairs: two chunks of the library's 64-pair launch sets; every record equals the single-pair call."""
    from eyoc_amd import icp
    s, t, T0 = _case(0, "samples")
    P, n = 70, 300
    S = np.concatenate([s[(7 * b) % 1000:][:n] for b in range(P)])
    T = np.concatenate([t[:2000]] * P)
    seg_s, seg_t = np.arange(P + 1) * n, np.arange(P + 1) * 2000
    got = icp.icp_batched(S, T, seg_s, seg_t, 0.6, np.stack([T0] * P), 5).cpu().numpy()
    for b in (0, 63, 64, 69):
        one = icp.icp_batched(S[seg_s[b]:seg_s[b + 1]], t[:2000], [0, n], [0, 2000], 0.6, T0[None], 5).cpu().numpy()
        assert one[0].tobytes() == got[b].tobytes(), b


# ---- 4. it refines

@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_it_refines(seed):
    from eyoc_amd import icp
    from eyoc_amd.metrics import registration_errors
    src, tgt, T0 = _case(seed, "samples")
    T_gt = np.asarray(_pair(seed)["T_gt"], np.float32)
    got = icp.registration_icp(src, tgt, 0.6, T0)
    rte0, rre0, _ = registration_errors(T0.astype(np.float32), T_gt, 2.0, 5.0)
    rte1, rre1, _ = registration_errors(got.transformation.astype(np.float32), T_gt, 2.0, 5.0)
    print(f"seed {seed}: RTE {rte0:.3f} -> {rte1:.3f} m, RRE {np.rad2deg(rre0):.3f} -> {np.rad2deg(rre1):.3f} deg, "
          f"{got.iterations} iterations, fitness {got.fitness:.4f}")
    assert rte1 <= rte0 and rre1 <= rre0


# ---- 5. status paths (none of them may fault)

def test_status_paths():
    from eyoc_amd import icp
    srcs, tgts, inits, _, _ = _eight()
    srcs, tgts, inits = srcs[:3], tgts[:3], inits[:3]

    def call(srcs, tgts, inits):
        seg_s = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
        seg_t = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
        res, corr = icp.icp_batched(np.concatenate(srcs).reshape(-1, 3), np.concatenate(tgts).reshape(-1, 3), seg_s, seg_t, 0.6,
                                    np.stack(inits), 10, return_correspondences=True)
        torch.cuda.synchronize()
        return res.cpu().numpy(), corr.cpu().numpy(), seg_s
    clean, _, _ = call(srcs, tgts, inits)

    def with_pair(src, tgt, init, status):
        """the faulty pair in the MIDDLE of the clean three: its record, and the others byte-identical to the call without it"""
        got, corr, seg = call([srcs[0], src, srcs[1], srcs[2]], [tgts[0], tgt, tgts[1], tgts[2]], [inits[0], init, inits[1], inits[2]])
        assert got[[0, 2, 3]].tobytes() == clean.tobytes(), status
        r = icp.decode_icp_result(torch.from_numpy(got[1]))
        assert r.status == status, (r.status, status)
        assert r.transformation.tobytes() == np.asarray(init, np.float64).tobytes()           # T as given, NaN bits included
        assert (r.fitness, r.inlier_rmse, r.inliers, r.iterations) == (0.0, 0.0, 0, 0)
        assert (corr[seg[1]:seg[2]] == -1).all()
        return r

    bad = inits[1].copy()
    bad[1, 3] = np.nan
    with_pair(srcs[1], tgts[1], bad, icp.BAD_INIT)
    inf = inits[1].copy()
    inf[0, 0] = np.inf
    with_pair(srcs[1], tgts[1], inf, icp.BAD_INIT)
    for which in ("src", "tgt"):
        s, t = srcs[1].copy(), tgts[1].copy()
        (s if which == "src" else t)[1234, 2] = np.nan
        with_pair(s, t, inits[1], icp.RANGE)
    t = tgts[1].copy()
    t[77] = (1e9, 0.0, 0.0)
    with_pair(srcs[1], t, inits[1], icp.RANGE)
    s = srcs[1].copy()
    s[77] = (1e9, 0.0, 0.0)                       # a far SOURCE point is no fault: it has no correspondence, the pair runs
    got, corr, seg = call([srcs[0], s, srcs[2]], [tgts[0], tgts[1], tgts[2]], inits)
    r = icp.decode_icp_result(torch.from_numpy(got[1]))
    assert not r.status & (icp.RANGE | icp.FEW | icp.BAD_INIT) and r.iterations >= 1 and corr[seg[1] + 77] == -1
    assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes()
    # disjoint clouds
    with_pair(srcs[1], tgts[1] + np.float32(500.0), inits[1], icp.FEW)
    # an empty segment between live ones (source, target, both)
    e = np.zeros((0, 3), np.float32)
    for s, t in ((e, tgts[1]), (srcs[1], e), (e, e)):
        with_pair(s, t, inits[1], icp.FEW)
    # a call in which every pair is empty
    got, _, _ = call([e, e], [e, tgts[0]], inits[:2])
    assert [icp.decode_icp_result(torch.from_numpy(g)).status for g in got] == [icp.FEW, icp.FEW]


def test_invalid_arguments_are_refused_not_run():
    from eyoc_amd import _lib, icp
    s, t, T0 = _case(0, "samples")
    for kw in (dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=float("nan")), dict(max_iteration=-1)):
        args = dict(max_correspondence_distance=0.6, max_iteration=5)
        args.update(kw)
        with pytest.raises(_lib.EyocError) as ei:
            icp.icp_batched(s, t, [0, len(s)], [0, len(t)], init=T0[None], **args)
        assert ei.value.code == _lib.ERR_INVALID
    lib = _lib.load()
    sd, td = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
    seg = (C.c_int32 * 2)(0, len(s))
    p = _lib.IcpParams(0.6, 1e-6, 1e-6, 5, 0)
    res = torch.zeros(160, dtype=torch.uint8, device="cuda")
    ws = _lib.workspace(1024, sd.device)
    rc = lib.eyoc_icp_batched(_lib.ctx(0), _lib.ptr(sd), _lib.ptr(td), seg, seg, 1, None, C.byref(p), _lib.ptr(res), None, _lib.ptr(ws), 1024,
                              _lib.stream_ptr())
    assert rc == _lib.ERR_WORKSPACE


# ---- 6. the reference's call sites, verbatim

def test_shim_runs_the_reference_lines():
    import eyoc_amd.o3d as o3d
    from eyoc_amd import icp
    src, tgt, T0 = _case(1, "5cm")
    M = T0

    def make_open3d_point_cloud(xyz):                      # util/pointcloud.py:9-14
        pcd = o3d.geometry.PointCloud()
        pcd.points = o3d.utility.Vector3dVector(xyz)
        return pcd

    def apply_transform(pts, trans):                       # lib/data_loaders.py:389-394
        R_, T_ = trans[:3, :3], trans[:3, 3]
        return pts @ R_.T + T_
    xyz0, xyz1 = src, tgt
    # lib/data_loaders.py:496-507
    xyz0_t = apply_transform(xyz0, M)
    pcd0 = make_open3d_point_cloud(xyz0_t)
    pcd1 = make_open3d_point_cloud(xyz1)
    reg = o3d.pipelines.registration.registration_icp(
        pcd0, pcd1, 0.2, np.eye(4),
        o3d.pipelines.registration.
        TransformationEstimationPointToPoint(),
        o3d.pipelines.registration.ICPConvergenceCriteria(
            max_iteration=200))
    pcd0.transform(reg.transformation)
    M2 = M @ reg.transformation
    assert M2.shape == (4, 4) and np.isfinite(M2).all()
    x32 = np.asarray(xyz0_t, np.float32)
    want = icp.decode_icp_result(icp.icp_batched(x32, xyz1, [0, len(x32)], [0, len(xyz1)], 0.2, None, 200)[0])
    assert reg.transformation.tobytes() == want.transformation.tobytes()
    assert (reg.fitness, reg.inlier_rmse, reg.iterations, reg.status) == (want.fitness, want.inlier_rmse, want.iterations, want.status)
    assert reg.fitness > 0.3 and len(reg.correspondence_set) == want.inliers
    np.testing.assert_allclose(np.asarray(pcd0.points), apply_transform(xyz0_t.astype(np.float64), reg.transformation), atol=1e-12)

    # scripts/SC2_PCR/benchmark_utils.py:40-56
    s, t, T0 = _case(2, "samples")
    src_keypts, tgt_keypts = torch.from_numpy(s)[None].cuda(), torch.from_numpy(t)[None].cuda()
    pred_trans = torch.from_numpy(T0.astype(np.float32))[None].cuda()
    refined = icp.icp_refine(src_keypts, tgt_keypts, pred_trans)
    assert refined.shape == (1, 4, 4) and refined.dtype == torch.float32 and refined.device == pred_trans.device
    want = icp.decode_icp_result(icp.icp_batched(s, t, [0, len(s)], [0, len(t)], 0.10, T0.astype(np.float32).astype(np.float64)[None], 30)[0])
    assert refined[0].cpu().numpy().tobytes() == want.transformation.astype(np.float32).tobytes()
    legacy = o3d.registration.registration_icp(make_open3d_point_cloud(s), make_open3d_point_cloud(t), 0.10,
                                               T0.astype(np.float32), o3d.registration.TransformationEstimationPointToPoint())
    assert legacy.transformation.tobytes() == want.transformation.tobytes()


# ---- 7. the harness stage

N_POINTS = 2000


def _model():
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    sd = syn.make_weights()
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.cuda().eval()


def _cfg(use_ransac, **kw):
    from eyoc_amd.harness import RegistrationConfig
    sc2 = dict(RegistrationConfig().sc2pcr, num_node=2000, max_points=2000)
    return RegistrationConfig(ransac_max_iteration=100000, n_points=N_POINTS, use_RANSAC=use_ransac, sc2pcr=sc2, **kw)


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def batch():
    from eyoc_amd import harness as h
    pairs = [_pair(s) for s in range(4)]
    return h.DeviceBatch(pairs, [0, 1, 2, 3], torch.device("cuda:0"), n_points=N_POINTS, descriptor=dict(inlier_ratio=0.3))


@pytest.mark.parametrize("use_ransac", [True, False])
def test_harness_stage(model, batch, use_ransac):
    from eyoc_amd import harness as h
    from eyoc_amd import icp
    plain = h.RegistrationPipeline(model, _cfg(use_ransac))
    base = plain.register(batch, seed=3, return_device=True)
    torch.cuda.synchronize()
    assert plain.last_icp is None and plain._icp_dev is None
    base_h = base.cpu().numpy()
    T32 = (base.view(torch.float32)[:, :16] if use_ransac else base.reshape(-1, 16)).clone()
    want = icp.icp_batched(batch.xyz0.reshape(-1, 3), batch.xyz1.reshape(-1, 3), batch.seg, batch.seg, 2 * 0.3, T32.to(torch.float64), 30)
    want_h = want.cpu().numpy()
    want_T = want.view(torch.float64)[:, :16].to(torch.float32).cpu().numpy()

    pipe = h.RegistrationPipeline(model, _cfg(use_ransac, icp_refine=True))
    got = pipe.register(batch, seed=3, return_device=True).cpu().numpy()
    assert pipe._icp_dev.cpu().numpy().tobytes() == want_h.tobytes()
    if use_ransac:
        assert got.shape == base_h.shape
        assert got.view(np.float32)[:, :16].tobytes() == want_T.tobytes()
        assert got[:, 64:].tobytes() == base_h[:, 64:].tobytes()            # inliers / hypothesis / survivors / rmse stay RANSAC's
    else:
        assert got.reshape(-1, 16).tobytes() == want_T.tobytes()
    results = pipe.register(batch, seed=3)
    assert [r.status for r in pipe.last_icp] == [icp.decode_icp_result(torch.from_numpy(w)).status for w in want_h]
    for p, r in enumerate(results):
        assert r.transformation.astype(np.float32).tobytes() == want_T[p].tobytes()
    rows_plain = plain.evaluate(batch, plain.register(batch, seed=3))
    rows = pipe.evaluate(batch, results)
    print("RANSAC" if use_ransac else "SC2-PCR", "RTE m:", [(round(a["rte"], 3), round(b["rte"], 3)) for a, b in zip(rows_plain, rows)],
          "ICP iterations:", [r.iterations for r in pipe.last_icp])
    for tail in (False, True):
        step = pipe.enqueue(batch, seed=3, slot=int(tail), tail_stream=tail)
        host, overflow = step.wait()
        assert not overflow and host.numpy().tobytes() == got.tobytes(), tail
        assert step.icp.numpy().tobytes() == want_h.tobytes(), tail
    # off again: the records of the plain path, byte for byte
    again = h.RegistrationPipeline(model, _cfg(use_ransac, icp_refine=False)).register(batch, seed=3, return_device=True)
    assert again.cpu().numpy().tobytes() == base_h.tobytes()


def test_harness_failed_pairs_stay_failed(model, batch):
    """isolate_failures + icp_refine: a dropped pair keeps its failed record and its ICP record says BAD_INIT; the live pairs are
    refined from their own RANSAC poses."""
    from eyoc_amd import harness as h
    from eyoc_amd import icp
    reduced = batch.without_pairs({1: h.DROPPED_DUPLICATE})
    cfg = _cfg(True, isolate_failures=True, icp_refine=True)
    pipe = h.RegistrationPipeline(model, cfg)
    res = pipe.register(reduced, seed=3)
    assert res[1].status == h.DROPPED_DUPLICATE and np.isnan(res[1].transformation).all()
    assert pipe.last_icp[1].status & (icp.BAD_INIT | icp.FEW)
    live = [p for p in range(4) if p != 1]
    assert all(pipe.last_icp[p].iterations >= 1 and not pipe.last_icp[p].status & (icp.BAD_INIT | icp.RANGE) for p in live)
    assert all(np.isfinite(res[p].transformation).all() for p in live)
    step = pipe.enqueue(reduced, seed=3, tail_stream=True)
    host, _ = step.wait()
    assert np.isnan(host.numpy().view(np.float32)[1, :16]).all() and step.status[1] == h.DROPPED_DUPLICATE
    assert icp.decode_icp_result(step.icp[1]).status & (icp.BAD_INIT | icp.FEW)
