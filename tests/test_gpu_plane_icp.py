"""Device-side normal estimation and batched point-to-plane ICP (csrc/icp.hip sections 5 and 6, eyoc_amd/icp.py) against the CPU
restatement of their contracts (tests/plane_icp_restatement.py), on ``synthetic.make_pair`` inputs.

Bounds, none of them tuned on the kernel's output:
* normals: count equal, rows with k < 3 exactly zero, otherwise |n x n_ref| <= 2^-22 + beta_i - 2^-22 covers the fp32 rounding of the
  three output components (sqrt(3) 2^-25 < 2^-24) with a factor 4, beta_i = 256 k 2^-53 lam1 / (lam2 - lam3) is the restatement's
  Davis-Kahan bound for two correct fp64 evaluations of the covariance.  A row with beta_i > 2^-30 is excused (its two smallest
  eigenvalues nearly coincide: the normal is not determined); at most 0.5 % of the rows may be (CPU: 0 % on the sample sets, 0.04-0.06 %
  on the full clouds).  The sign: n . x_i <= 0, checked where the restated |n_ref . x_i| exceeds (2^-22 + beta_i) |x_i| - below that the
  sign itself is within the bound of flipping.
* whole runs: equal iteration count and status, every entry of T within 1e-4 (the project's pose bar), inlier_rmse within
  1e-4 m, the correspondence count within the number of rows within 1e-8 m^2 of the gate under the restatement's final T.  CPU: the
  restated runs of seeds 0-3 take 18, 18, 20 and 30 iterations and stay 1.8e-7 or more away from a convergence threshold.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import icp_restatement as R
import plane_icp_restatement as PR

pytestmark = pytest.mark.gpu

GATE, GATE_BAND = 0.6, 1e-8
RADIUS, MAX_NN = 1.5, 30


@functools.lru_cache(maxsize=None)
def _pair(seed):
    from eyoc_amd import synthetic as syn
    return syn.make_pair(seed)


@functools.lru_cache(maxsize=None)
def _case(seed):
    """-> (src f32 [5000, 3], tgt f32 [5000, 3], init f64 [4, 4]): the harness's two sample sets and a RANSAC-grade start"""
    from eyoc_amd import harness as h
    p = _pair(seed)
    T0 = R.perturb(np.asarray(p["T_gt"], np.float64), np.random.default_rng(seed), 1.0, 0.2)
    i0 = h.sample_indices(seed, 0, len(p["xyz0"]), 5000)
    i1 = h.sample_indices(seed, 1, len(p["xyz1"]), 5000)
    return np.ascontiguousarray(p["xyz0"][i0], np.float32), np.ascontiguousarray(p["xyz1"][i1], np.float32), T0


def _lattice(n, pitch=0.3):
    g = (np.arange(n, dtype=np.float32) - np.float32(n // 2)) * np.float32(pitch)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32(4.0)


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """-> (points, radius, max_nn)"""
    if name.startswith("samples"):
        return _case(int(name[-1]))[1], RADIUS, MAX_NN
    if name == "full0":
        return np.ascontiguousarray(_pair(0)["xyz1"], np.float32), 0.9, MAX_NN
    if name == "all":
        return _case(0)[1], RADIUS, 0
    return _lattice(7), 0.65, MAX_NN


@functools.lru_cache(maxsize=None)
def _restated_normals(name):
    return PR.normals(*_cloud(name))


@functools.lru_cache(maxsize=None)
def _normals32(seed):
    """the restatement's normals of the seed's target sample set, rounded once to fp32: what both sides of a whole run are given"""
    return np.ascontiguousarray(_restated_normals(f"samples{seed}").normals.astype(np.float32))


@functools.lru_cache(maxsize=None)
def _restated_run(seed):
    src, tgt, T0 = _case(seed)
    return PR.icp_plane(src, tgt, _normals32(seed), GATE, T0, 30)


def _segments(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])])


# ---- 1. normals, row for row

@pytest.mark.parametrize("name", ["samples0", "samples1", "full0", "all", "lattice"])
def test_normals_row_for_row(name):
    from eyoc_amd import icp
    pts, radius, max_nn = _cloud(name)
    want = _restated_normals(name)
    got, count, status = icp.estimate_normals_batched(pts, [0, len(pts)], radius, max_nn, return_count=True)
    got, count = got.cpu().numpy().astype(np.float64), count.cpu().numpy()
    assert int(status[0]) == 0
    np.testing.assert_array_equal(count, want.k)
    few = want.k < 3
    assert (got[few] == 0).all()
    length = np.linalg.norm(got[~few], axis=1)
    assert np.abs(length - 1.0).max() < 2.0 ** -22
    if name == "lattice":        # lam2 == lam3 by symmetry on most rows: nothing about the direction is pinned
        assert (want.k == 30).any() and (want.k < 30).any()
        print(f"{name}: {len(pts)} rows, k from {want.k.min()} to {want.k.max()}")
        return
    if max_nn:
        print(f"{name}: {len(pts)} rows, {few.mean():.1%} with k < 3, {(want.k == max_nn).mean():.1%} cut at {max_nn}")
    excused = ~few & (want.beta > 2.0 ** -30)
    ok = ~few & ~excused
    err = np.linalg.norm(np.cross(got[ok], want.normals[ok]), axis=1)
    print(f"{name}: excused {excused.sum()} of {len(pts)} rows ({excused.mean():.3%}), largest |n x n_ref| {err.max():.3e} "
          f"(largest bound {(2.0 ** -22 + want.beta[ok]).max():.3e})")
    assert excused.mean() <= 0.005
    assert (err <= 2.0 ** -22 + want.beta[ok]).all()
    x = pts[ok].astype(np.float64)
    decided = np.abs((want.normals[ok] * x).sum(1)) > (2.0 ** -22 + want.beta[ok]) * np.linalg.norm(x, axis=1)
    assert decided.mean() > 0.99
    assert ((got[ok] * x).sum(1)[decided] < 0).all() and ((got[ok] * want.normals[ok]).sum(1)[decided] > 0).all()


# ---- 2. whole runs

def check_whole_run(got, want, src, tgt, gate, what=""):
    """A decoded device run (with its correspondence set) against the restated run of the same inputs, under the module's bounds."""
    near_gate = int((np.abs(R.evaluate(src, tgt, want.T, np.sqrt(gate * gate + 2 * GATE_BAND)).d2 - gate * gate) < GATE_BAND).sum())
    dT = np.abs(got.transformation - want.T).max()
    print(f"{what}: iterations {got.iterations} / {want.iterations}, status {got.status} / {want.status}, max |dT| {dT:.3e}, d rmse "
          f"{abs(got.inlier_rmse - want.inlier_rmse):.3e}, correspondences {got.inliers} / {want.correspondences} ({near_gate} rows within "
          f"{GATE_BAND} m^2 of the gate)")
    assert got.iterations == want.iterations
    assert got.status == want.status
    assert dT < 1e-4
    assert abs(got.inlier_rmse - want.inlier_rmse) < 1e-4
    assert abs(got.inliers - want.correspondences) <= near_gate
    assert got.correspondence_set.shape == (got.inliers, 2)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_whole_run_matches_the_restatement(seed):
    from eyoc_amd import icp
    src, tgt, T0 = _case(seed)
    want, closest = _restated_run(seed)
    assert closest > 1e-9, "this case's iteration count hangs on rounding: use another seed"
    res, corr = icp.icp_plane_batched(src, tgt, _normals32(seed), [0, len(src)], [0, len(tgt)], GATE, T0[None], 30, return_correspondences=True)
    got = icp.decode_icp_result(res[0], corr)
    check_whole_run(got, want, src, tgt, GATE, f"seed {seed} (closest approach to a threshold {closest:.3e})")


# ---- 3. kernel-shape edges: byte-identical from run to run and to the pair / cloud alone

def _plane(srcs, tgts, nrms, inits, iterations=8):
    from eyoc_amd import icp
    res, corr = icp.icp_plane_batched(np.concatenate(srcs).reshape(-1, 3), np.concatenate(tgts).reshape(-1, 3),
                                      np.concatenate(nrms).reshape(-1, 3), _segments(srcs), _segments(tgts), GATE, np.stack(inits), iterations,
                                      return_correspondences=True)
    return res.cpu().numpy(), corr.cpu().numpy()


def _check_batch(srcs, tgts, nrms, inits, alone, iterations=8):
    a, ca = _plane(srcs, tgts, nrms, inits, iterations)
    b, cb = _plane(srcs, tgts, nrms, inits, iterations)
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    seg = _segments(srcs)
    for p in alone:
        one, c1 = _plane(srcs[p:p + 1], tgts[p:p + 1], nrms[p:p + 1], inits[p:p + 1], iterations)
        assert one[0].tobytes() == a[p].tobytes(), p
        assert c1.tobytes() == ca[seg[p]:seg[p + 1]].tobytes(), p
    return a


def test_block_tail_segments():
    from eyoc_amd import icp
    s, t, T0 = _case(0)
    n = _normals32(0)
    rec = _check_batch([s[:255], s[300:556], s[1000:1257]], [t, t, t], [n, n, n], [T0] * 3, alone=(0, 1, 2))
    runs = [icp.decode_icp_result(torch.from_numpy(r)) for r in rec]
    assert all(r.iterations >= 1 and not r.status & ~icp.CONVERGED for r in runs)


def test_a_pair_of_more_than_64_workgroups():
    from eyoc_amd import icp
    s, t, T0 = _case(0)
    big = np.ascontiguousarray(_pair(0)["xyz0"][:64 * 256 + 1], np.float32)
    assert len(big) == 16385
    n = _normals32(0)
    rec = _check_batch([s[:255], big], [t, t], [n, n], [T0, T0], alone=(1,), iterations=4)
    r = icp.decode_icp_result(torch.from_numpy(rec[1]))
    assert r.iterations >= 1 and r.inliers > 1000 and not r.status & ~icp.CONVERGED


def test_one_pair_more_than_a_launch_set():
    s, t, T0 = _case(0)
    n = _normals32(0)
    P = 65
    _check_batch([s[(7 * b) % 1000:][:100] for b in range(P)], [t[:1500]] * P, [n[:1500]] * P, [T0] * P, alone=(0, 63, 64), iterations=3)


def test_empty_segments_between_live_pairs():
    from eyoc_amd import icp
    s, t, T0 = _case(0)
    n = _normals32(0)
    e = np.zeros((0, 3), np.float32)
    rec = _check_batch([s[:500], e, s[500:1000], s[1000:1500], s[1500:2000]], [t, t, t, e, t], [n, n, n, e, n], [T0] * 5, alone=(0, 2, 4))
    st = [icp.decode_icp_result(torch.from_numpy(r)).status for r in rec]
    assert st[1] == icp.FEW and st[3] == icp.FEW and not (st[0] | st[2] | st[4]) & ~icp.CONVERGED


def test_normals_batch_invariance():
    from eyoc_amd import icp
    t = _case(0)[1]
    clouds = [t[(37 * b) % 2000:][:150] for b in range(65)] + [t[:257]]
    seg = _segments(clouds)

    def call(parts):
        n, c, st = icp.estimate_normals_batched(np.concatenate(parts), _segments(parts), RADIUS, MAX_NN, return_count=True)
        assert (st == 0).all()
        return n.cpu().numpy(), c.cpu().numpy()
    a, ca = call(clouds)
    b, cb = call(clouds)
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    assert (ca >= 3).any()
    for p in (0, 63, 64, 65):
        one, c1 = call(clouds[p:p + 1])
        assert one.tobytes() == a[seg[p]:seg[p + 1]].tobytes() and c1.tobytes() == ca[seg[p]:seg[p + 1]].tobytes(), p


# ---- 4. status paths (none of them may fault)

def _plane_scene():
    """an exact lattice plane z = -1.5 as the target, a shifted part of it as the source"""
    g = np.arange(-20, 20, dtype=np.float32) * np.float32(0.25)
    tgt = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    tgt = np.concatenate([tgt, np.full((len(tgt), 1), -1.5, np.float32)], 1).astype(np.float32)
    src = (tgt[200:1200] + np.float32([0.05, 0.03, 0.1])).astype(np.float32)
    return src, tgt


def test_status_paths():
    from eyoc_amd import icp
    s, t, T0 = _case(0)
    n = _normals32(0)
    srcs, tgts, nrms, inits = [s[:1000], s[1000:2000]], [t, t], [n, n], [T0, T0]
    clean, _ = _plane(srcs, tgts, nrms, inits)

    def with_pair(src, tgt, nrm, init, status, untouched=True):
        """the pair in the MIDDLE of the clean two: its record, and the others byte-identical to the call without it"""
        got, corr = _plane([srcs[0], src, srcs[1]], [tgts[0], tgt, tgts[1]], [nrms[0], nrm, nrms[1]], [inits[0], init, inits[1]])
        assert got[[0, 2]].tobytes() == clean.tobytes(), status
        r = icp.decode_icp_result(torch.from_numpy(got[1]))
        assert r.status == status, (r.status, status)
        assert r.transformation.tobytes() == np.asarray(init, np.float64).tobytes()           # T as given, NaN bits included
        assert r.iterations == 0
        if untouched:
            assert (r.fitness, r.inlier_rmse, r.inliers) == (0.0, 0.0, 0)
            assert (corr[len(srcs[0]):len(srcs[0]) + len(src)] == -1).all()
        return r

    # an exact plane with one normal: rotation about the normal and the two shifts inside the plane are free
    ps, pt = _plane_scene()
    up = np.broadcast_to(np.float32([0, 0, 1]), pt.shape).copy()
    r = with_pair(ps, pt, up, np.eye(4), icp.SINGULAR, untouched=False)
    assert r.fitness > 0 and r.inliers >= 3
    # a NaN normal: RANGE for that pair only
    bad_n = n.copy()
    bad_n[1234, 1] = np.nan
    with_pair(s[2000:3000], t, bad_n, T0, icp.RANGE)
    # a non-finite init
    bad = T0.copy()
    bad[1, 3] = np.nan
    with_pair(s[2000:3000], t, n, bad, icp.BAD_INIT)
    # disjoint clouds: fewer than 3 correspondences
    with_pair(s[2000:3000], t + np.float32(500.0), n, T0, icp.FEW)
    # all-zero normals, as a cloud gives them where every row has k < 3: A = 0
    zero, count, st = icp.estimate_normals_batched(t, [0, len(t)], 1e-3, MAX_NN, return_count=True)
    assert int(st[0]) == 0 and int(count.max()) < 3 and not zero.any()
    r = with_pair(s[2000:3000], t, zero.cpu().numpy(), T0, icp.SINGULAR, untouched=False)
    assert r.fitness > 0
    # a cloud the grid cannot hold: RANGE, zero normals, count 0 - and its neighbour in the batch is what it is alone
    far = t[:300].copy()
    far[7] = (np.inf, 0.0, 0.0)
    nn, cc, st = icp.estimate_normals_batched(np.concatenate([far, t[:300]]), [0, 300, 600], RADIUS, MAX_NN, return_count=True)
    one, c1, _ = icp.estimate_normals_batched(t[:300], [0, 300], RADIUS, MAX_NN, return_count=True)
    assert st.tolist() == [icp.RANGE, 0] and not nn[:300].any() and not cc[:300].any()
    assert nn[300:].cpu().numpy().tobytes() == one.cpu().numpy().tobytes() and cc[300:].cpu().numpy().tobytes() == c1.cpu().numpy().tobytes()


def test_invalid_arguments_are_refused_not_run():
    from eyoc_amd import _lib, icp
    s, t, T0 = _case(0)
    n = _normals32(0)
    for kw in (dict(max_nn=65), dict(max_nn=-1), dict(radius=-1.0), dict(radius=0.0), dict(radius=float("nan"))):
        args = dict(radius=RADIUS, max_nn=MAX_NN)
        args.update(kw)
        with pytest.raises(_lib.EyocError) as ei:
            icp.estimate_normals_batched(t, [0, len(t)], **args)
        assert ei.value.code == _lib.ERR_INVALID, kw
    lib = _lib.load()
    sd, td, nd = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(n).cuda()
    seg = (C.c_int32 * 2)(0, len(s))
    p = _lib.IcpParams(GATE, 1e-6, 1e-6, 5, 0)
    res = torch.zeros(160, dtype=torch.uint8, device="cuda")
    need = lib.eyoc_icp_plane_workspace_bytes(1, len(s), len(t))
    ws = _lib.workspace(need + 256, sd.device)

    def plane(normals, ws_ptr, ws_bytes):
        return lib.eyoc_icp_plane_batched(_lib.ctx(0), _lib.ptr(sd), _lib.ptr(td), normals, seg, seg, 1, None, C.byref(p), _lib.ptr(res), None,
                                          ws_ptr, ws_bytes, _lib.stream_ptr())
    assert plane(None, _lib.ptr(ws), need) == _lib.ERR_INVALID                        # NULL normals with target rows
    assert plane(_lib.ptr(nd), C.c_void_p(ws.data_ptr() + 128), need) == _lib.ERR_INVALID          # a misaligned workspace
    assert plane(_lib.ptr(nd), _lib.ptr(ws), need - 1) == _lib.ERR_WORKSPACE          # one byte short
    out = torch.zeros((len(t), 3), dtype=torch.float32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = lib.eyoc_normals_workspace_bytes(1, len(t))

    def nrm(ws_ptr, ws_bytes, out_ptr=_lib.ptr(out)):
        return lib.eyoc_normals_batched(_lib.ctx(0), _lib.ptr(td), seg, 1, RADIUS, MAX_NN, out_ptr, None, _lib.ptr(st), ws_ptr, ws_bytes,
                                        _lib.stream_ptr())
    assert need <= ws.numel()
    assert nrm(C.c_void_p(ws.data_ptr() + 128), need) == _lib.ERR_INVALID
    assert nrm(_lib.ptr(ws), need - 1) == _lib.ERR_WORKSPACE
    assert nrm(_lib.ptr(ws), need, None) == _lib.ERR_INVALID                          # NULL output with rows
    torch.cuda.synchronize()
    assert not res.any() and not out.any()                                            # nothing ran


# ---- 5. end to end: normals estimated on the device

def test_end_to_end_with_device_normals():
    from eyoc_amd import icp
    from eyoc_amd.metrics import registration_errors
    src, tgt, T0 = _case(0)
    want, _ = _restated_run(0)
    got = icp.registration_icp_point_to_plane(src, tgt, GATE, T0, normal_radius=RADIUS, max_nn=MAX_NN)
    dT = np.abs(got.transformation - want.T).max()
    T_gt = np.asarray(_pair(0)["T_gt"], np.float32)
    rte, rre, _ = registration_errors(got.transformation.astype(np.float32), T_gt, 2.0, 5.0)
    print(f"iterations {got.iterations} / {want.iterations}, status {got.status} / {want.status}, max |dT| {dT:.3e}, RTE {rte:.3f} m, "
          f"RRE {np.rad2deg(rre):.3f} deg")
    assert dT < 1e-4
    given = icp.registration_icp_point_to_plane(src, tgt, GATE, T0, target_normals=_normals32(0))
    assert np.abs(given.transformation - want.T).max() < 1e-4
    with pytest.raises(ValueError):
        icp.registration_icp_point_to_plane(src, tgt, GATE, T0)


# ---- 6. the harness option

N_POINTS = 2000


def _cfg(**kw):
    from eyoc_amd.harness import RegistrationConfig
    return RegistrationConfig(ransac_max_iteration=100000, n_points=N_POINTS, use_RANSAC=True, **kw)


@pytest.fixture(scope="module")
def model():
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    sd = syn.make_weights()
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.cuda().eval()


@pytest.fixture(scope="module")
def batch():
    from eyoc_amd import harness as h
    pairs = [_pair(s) for s in range(4)]
    return h.DeviceBatch(pairs, [0, 1, 2, 3], torch.device("cuda:0"), n_points=N_POINTS, descriptor=dict(inlier_ratio=0.3))


def test_harness_plane_and_point(model, batch):
    from eyoc_amd import harness as h
    from eyoc_amd import icp
    plain = h.RegistrationPipeline(model, _cfg())
    base = plain.register(batch, seed=3, return_device=True)
    T32 = base.view(torch.float32)[:, :16].clone()
    xyz0, xyz1 = batch.xyz0.reshape(-1, 3), batch.xyz1.reshape(-1, 3)
    # "point" is the path as it was: the records of icp_batched on the same inputs, byte for byte
    pipe = h.RegistrationPipeline(model, _cfg(icp_refine=True, icp_method="point"))
    got = pipe.register(batch, seed=3, return_device=True).cpu().numpy()
    want = icp.icp_batched(xyz0, xyz1, batch.seg, batch.seg, 0.6, T32.to(torch.float64), 30)
    assert pipe._icp_dev.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert got.view(np.float32)[:, :16].tobytes() == want.view(torch.float64)[:, :16].to(torch.float32).cpu().numpy().tobytes()
    # "plane": normals of the target sample sets inside 5 voxels, then the point-to-plane records
    pipe = h.RegistrationPipeline(model, _cfg(icp_refine=True, icp_method="plane"))
    results = pipe.register(batch, seed=3)
    normals, st = icp.estimate_normals_batched(xyz1, batch.seg, 1.5, 30)
    want = icp.icp_plane_batched(xyz0, xyz1, normals, batch.seg, batch.seg, 0.6, T32.to(torch.float64), 30)
    assert (st == 0).all() and pipe._icp_dev.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert len(pipe.last_icp) == batch.P == len(results)
    assert all(np.isfinite(r.transformation).all() for r in results)
    assert all(r.iterations >= 1 and not r.status & (icp.BAD_INIT | icp.RANGE) for r in pipe.last_icp)
    rows = pipe.evaluate(batch, results)
    rows_plain = plain.evaluate(batch, plain.register(batch, seed=3))
    print("RTE m (no ICP, plane):", [(round(a["rte"], 3), round(b["rte"], 3)) for a, b in zip(rows_plain, rows)],
          "iterations:", [r.iterations for r in pipe.last_icp], "status:", [r.status for r in pipe.last_icp])


def test_harness_plane_failed_pairs_stay_failed(model, batch):
    from eyoc_amd import harness as h
    from eyoc_amd import icp
    reduced = batch.without_pairs({1: h.DROPPED_DUPLICATE})
    pipe = h.RegistrationPipeline(model, _cfg(isolate_failures=True, icp_refine=True, icp_method="plane"))
    res = pipe.register(reduced, seed=3)
    assert res[1].status == h.DROPPED_DUPLICATE and np.isnan(res[1].transformation).all()
    assert pipe.last_icp[1].status & icp.BAD_INIT
    live = [p for p in range(4) if p != 1]
    assert all(pipe.last_icp[p].iterations >= 1 and not pipe.last_icp[p].status & (icp.BAD_INIT | icp.RANGE) for p in live)
    assert all(np.isfinite(res[p].transformation).all() for p in live)
