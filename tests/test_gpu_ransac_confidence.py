"""eyoc_ransac_converging_batched_ws (include/eyoc_hip.h "RANSACConvergenceCriteria ... with confidence below 1") and the Python
layers above it.  The contract is checked against the EXISTING one-pass call: a pair that stopped at checkpoint E must carry, byte for
byte, the record ``eyoc_ransac_batched_ws`` gives with ``max_iteration = E``, and E must be the checkpoint the fp64 restatement
(tests/ransac_confidence_restatement.py) picks from the one-pass call's inlier counts at the checkpoints.  The restatement's ``log``
and the device's may differ in the last bits, so every decision looked at is asserted to be far from borderline."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _inputs as gi
import ransac_confidence_restatement as RC
import test_gpu_workspace_contract as G

pytestmark = pytest.mark.gpu

THR = RC.THRESHOLD
C999 = 0.999


def _lib():
    from eyoc_amd import _lib as L
    return L, L.load()


def _pack(cases):
    seg = [0]
    for p0, _ in cases:
        seg.append(seg[-1] + len(p0))
    s = torch.from_numpy(np.concatenate([c[0] for c in cases]).astype(np.float32)).cuda()
    t = torch.from_numpy(np.concatenate([c[1] for c in cases]).astype(np.float32)).cuda()
    corr = torch.cat([torch.arange(len(c[0])) for c in cases]).cuda()
    return s, t, corr, seg


def _one_pass(cases, H, seed):
    """The existing call -> records ``uint8 [P, 80]``."""
    from eyoc_amd import registration as reg
    s, t, corr, seg = _pack(cases)
    return reg.ransac_batched_from_correspondences(s, t, corr, seg, seg, THR, H, seed=seed).cpu().numpy()


def _converging(cases, H, first, seed, c=C999, budget=0, fill=None):
    """The new entry point through ctypes, on a workspace of this test's making -> ``(records uint8 [P, 80], iterations int32 [P])``."""
    L, lib = _lib()
    s, t, corr, seg = _pack(cases)
    P = len(cases)
    nbytes = lib.eyoc_ransac_converging_workspace_bytes(L.ctx(), P, seg[-1], H, first, budget)
    assert nbytes > 0
    ws = L.workspace(nbytes, s.device)
    if fill is not None:
        ws.fill_(fill)
    res = torch.full((P, C.sizeof(L.RansacResult)), 0xA5, dtype=torch.uint8, device=s.device)
    it = torch.full((P,), -7, dtype=torch.int32, device=s.device)
    sg = (C.c_int32 * (P + 1))(*seg)
    p = L.RansacParams(THR, 0.9, H, seed)
    L.check(lib.eyoc_ransac_converging_batched_ws(L.ctx(), L.ptr(s), L.ptr(t), L.ptr(corr), sg, sg, P, C.byref(p), c, first, L.ptr(res),
                                                  L.ptr(it), L.ptr(ws), nbytes, L.stream_ptr()), "eyoc_ransac_converging_batched_ws")
    return res.cpu().numpy(), it.cpu().numpy()


def _inliers(rec_bytes):
    L, _ = _lib()
    return L.RansacResult.from_buffer_copy(rec_bytes.tobytes()).inliers


def _check_prefix(p0, p1, H, first, seed, rec, it, c=C999):
    """``rec`` / ``it``: one pair's record and iterations.  The stop is the restatement's on the one-pass call's counts, no decision is
    borderline, and the record is the one-pass call's at ``max_iteration = it``.  -> the decisions looked at."""
    one = functools.lru_cache(maxsize=None)(lambda E: _one_pass([(p0, p1)], E, seed)[0])
    stop, seen = RC.stop_checkpoint(lambda E: _inliers(one(E)), len(p0), RC.as_device(c), first, H)
    print(f"n={len(p0)} H={H} first_check={first} seed={seed}: iterations={it}, decisions={seen}")
    assert not any(RC.borderline(E, k) for E, _, k, _ in seen)
    assert it == stop
    assert rec.tobytes() == one(int(it)).tobytes()
    return seen


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n", [4, 64, 600])
def test_confidence_one_through_the_new_entry_point(n):
    p0, p1, _ = gi.corr_case(1000 + n, n, gi.rigid(*RC.T0_ARGS), 1.0 if n < 63 else 0.5, noise=0.03)
    H = 1 << 14
    want = _one_pass([(p0, p1)], H, RC.SEED)
    for c in (1.0, 10000.0):
        rec, it = _converging([(p0, p1)], H, 1024, RC.SEED, c=c)
        assert rec.tobytes() == want.tobytes() and it.tolist() == [H], c


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", list(RC.HOST_CASES))
def test_prefix_identity_of_the_host_cases(name):
    n, _, H, first, inliers, _, stops_at = RC.HOST_CASES[name]
    p0, p1 = RC.case_points(name)
    rec, it = _converging([(p0, p1)], H, first, RC.SEED)
    seen = _check_prefix(p0, p1, H, first, RC.SEED, rec[0], int(it[0]))
    assert int(it[0]) == stops_at and _inliers(rec[0]) == inliers            # what the host test found on the oracle
    assert [E for E, *_ in seen] == [E for E in RC.checkpoints(first, H) if E <= stops_at]


# ---------------------------------------------------------------------------------------------------------------- 3
def test_one_batch_of_six_pairs_and_one_pair_per_chunk():
    L, _ = _lib()
    H, first, seed = 1 << 17, 1024, 7
    cases = [RC.case_points(name) for name in RC.HOST_CASES]
    two = (cases[0][0][:2].copy(), cases[0][1][:2].copy())                    # degenerate: 2 rows
    cases = cases[:3] + [two] + cases[3:]
    prev = L.knob("eyoc_registration_accept_degenerate", 1)
    try:
        rec, it = _converging(cases, H, first, seed)
        rec1, it1 = _converging(cases, H, first, seed, budget=1)              # one pair per chunk
    finally:
        L.knob("eyoc_registration_accept_degenerate", prev)
    assert rec1.tobytes() == rec.tobytes() and it1.tolist() == it.tolist()
    print("iterations of the batch:", it.tolist())
    assert it[3] == 0 and _inliers(rec[3]) == 0 and np.isnan(rec[3].view(np.float32)[:16]).all()
    assert len(set(it.tolist())) >= 4                                         # 0, and at least three different checkpoints
    for b, (p0, p1) in enumerate(cases):
        if b == 3:
            continue
        r, i = _converging([(p0, p1)], H, first, seed + b)
        assert rec[b].tobytes() == r[0].tobytes() and it[b] == i[0], b
    # the pair with 8 % inliers, alone in the table above with seed 7, draws with seed 7 + 4 here: its stop is checked from scratch
    _check_prefix(*cases[4], H, first, seed + 4, rec[4], int(it[4]))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name,H,first", [("frac0.15", 100000, 1000), ("frac0.15", 4096, 4096), ("frac0.15", 4096, 1 << 20),
                                          ("frac0.5", 4096, 4096), ("all_inliers", 64, 1), ("frac0.5", 64, 1)])
def test_checkpoint_edges(name, H, first):
    p0, p1 = RC.case_points(name)
    rec, it = _converging([(p0, p1)], H, first, RC.SEED)
    _check_prefix(p0, p1, H, first, RC.SEED, rec[0], int(it[0]))
    assert int(it[0]) in RC.checkpoints(first, H)
    if first >= H:
        assert int(it[0]) == H                                                # one round


# ---------------------------------------------------------------------------------------------------------------- 5
class _knob:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        L, _ = _lib()
        self.prev = L.knob(self.name, self.value)

    def __exit__(self, *exc):
        L, _ = _lib()
        L.knob(self.name, self.prev)


@pytest.mark.parametrize("knob,value", [("eyoc_ransac_select_generate", 0), ("eyoc_ransac_select_generate", 1),
                                        ("eyoc_ransac_select_pruning", 0), ("eyoc_ransac_select_pruning", 1),
                                        ("eyoc_ransac_select_pruning", 2), ("eyoc_ransac_transform_store", 1)])
def test_kernel_switches(knob, value):
    """A pair that runs four rounds, under every switch: the bytes of the prefix call under the same switch - and of the default."""
    p0, p1 = RC.case_points("frac0.15")
    H, first = 1 << 15, 1024
    want, want_it = _converging([(p0, p1)], H, first, RC.SEED)
    with _knob(knob, value):
        rec, it = _converging([(p0, p1)], H, first, RC.SEED)
        same_switch = _one_pass([(p0, p1)], int(it[0]), RC.SEED)
    assert it.tolist() == want_it.tolist() == [8192]
    assert rec.tobytes() == same_switch.tobytes() == want.tobytes()


def test_count_bound_across_rounds_in_a_chunk_of_33_pairs():
    """eyoc_ransac_select_pruning 2 applies its count bound to chunks of >= 32 pairs; a round starts the bound at the carried best count."""
    cases = [gi.corr_case(500 + b, 300 + 7 * b, gi.rigid(*RC.T0_ARGS), (0.5, 0.2, 0.12)[b % 3], noise=0.03)[:2] for b in range(33)]
    H, first, seed = 1 << 14, 512, 11
    out = {}
    for value in (0, 2):
        with _knob("eyoc_ransac_select_pruning", value):
            out[value] = _converging(cases, H, first, seed)
    assert out[0][0].tobytes() == out[2][0].tobytes() and out[0][1].tolist() == out[2][1].tolist()
    rec, it = out[2]
    print("iterations of the 33 pairs:", it.tolist())
    assert len(set(it.tolist())) >= 3
    for b in (0, 1, 2, 32):
        _check_prefix(*cases[b], H, first, seed + b, rec[b], int(it[b]))


def test_a_pair_past_the_lds_capacity_of_the_compact_records():
    p0, p1, _ = gi.corr_case(77, 12001, gi.rigid(*RC.T0_ARGS), 0.2, noise=0.03)
    H, first = 1 << 14, 1024
    rec, it = _converging([(p0, p1)], H, first, 3)
    _check_prefix(p0, p1, H, first, 3, rec[0], int(it[0]))


# ---------------------------------------------------------------------------------------------------------------- 6, 7
# The workspace contract with the instrument every other entry point is measured with (tests/workspace_contract.py): the cases are
# registered in test_gpu_workspace_contract.CASES - whose completeness test asks that every sizing function of the header has one - and
# run here through that module's own test bodies: every fill in an exact-size workspace, one byte short, misaligned.
# The registration happens when THIS module is imported, i.e. whenever pytest collects the tests directory.  Someone who runs
# tests/test_workspace_contract_host.py by its path alone gets "neither covered ... nor exempt: eyoc_ransac_converging_workspace_bytes"
# from its completeness test: add this file to the command line.  The two cases belong in test_gpu_workspace_contract.py itself
# (they would then also be part of its own parametrised tests, which are parametrised before this module registers them); they move
# there with the next change that edits that file.
CONV_H, CONV_FIRST = G.RANSAC_H, 1024


def _contract_run(s):
    from eyoc_amd import registration as reg
    return reg.ransac_batched_from_correspondences(s["s"], s["t"], s["c"], s["seg"], s["seg"], 0.3, CONV_H, seed=40, confidence=C999,
                                                   first_check=CONV_FIRST, return_iterations=True)


def _contract_sizes(s):
    L, lib = _lib()
    return [lib.eyoc_ransac_converging_workspace_bytes(L.ctx(0), len(s["src"]), s["seg"][-1], CONV_H, CONV_FIRST, 0)]


def _contract_reference(s, out):
    rec, it = out[0].cpu().numpy(), out[1].cpu().numpy()
    for b, (p0, p1) in enumerate(zip(s["src"], s["tgt"])):
        _check_prefix(p0, p1, CONV_H, CONV_FIRST, 40 + b, rec[b], int(it[b]))


_COVERS = ["eyoc_ransac_converging_workspace_bytes", "registration.py:ransac_batched_from_correspondences"]


@G.case("ransac_converging_ws", _COVERS, short="chunks", note="as ransac_batched_ws: one byte short of the two-pair chunk is a one-pair chunk")
class _Converging:
    setup = lambda: G._ransac_setup((600, 64))    # noqa: E731
    run, sizes, reference = _contract_run, _contract_sizes, _contract_reference


@G.case("ransac_converging_single", _COVERS)
class _ConvergingSingle:
    setup = lambda: G._ransac_setup((600,))       # noqa: E731
    run, sizes, reference = _contract_run, _contract_sizes, _contract_reference


@pytest.mark.parametrize("name", ["ransac_converging_ws", "ransac_converging_single"])
def test_dirty_and_exact_size_workspace(name):
    G.test_exact_workspace_under_every_fill(name)


@pytest.mark.parametrize("name", ["ransac_converging_ws", "ransac_converging_single"])
def test_short_workspace(name):
    G.test_short_workspace_is_refused_before_anything_runs(name)


@pytest.mark.parametrize("name", ["ransac_converging_ws", "ransac_converging_single"])
def test_misaligned_workspace(name):
    G.test_misaligned_workspace_is_refused_before_anything_runs(name)


def test_refused_arguments_leave_the_outputs_alone():
    L, lib = _lib()
    p0, p1 = RC.case_points("frac0.5")
    s, t, corr, seg = _pack([(p0, p1)])
    H = 4096
    nbytes = lib.eyoc_ransac_converging_workspace_bytes(L.ctx(), 1, seg[-1], H, 1024, 0)
    assert lib.eyoc_ransac_converging_workspace_bytes(L.ctx(), 1, seg[-1], H, 0, 0) == 0
    ws = L.workspace(nbytes + 256, s.device)
    res = torch.full((1, C.sizeof(L.RansacResult)), 0xA5, dtype=torch.uint8, device=s.device)
    it = torch.full((1,), -7, dtype=torch.int32, device=s.device)
    sg = (C.c_int32 * 2)(*seg)
    p = L.RansacParams(THR, 0.9, H, 7)

    def call(c, first, w, nb):
        return lib.eyoc_ransac_converging_batched_ws(L.ctx(), L.ptr(s), L.ptr(t), L.ptr(corr), sg, sg, 1, C.byref(p), c, first, L.ptr(res),
                                                     L.ptr(it), L.ptr(w), nb, L.stream_ptr())
    assert call(C999, 1024, ws, nbytes - 1) == L.ERR_WORKSPACE
    assert call(C999, 1024, ws[16:], nbytes) == L.ERR_INVALID
    for c in (0.0, -0.5, float("nan")):
        assert call(c, 1024, ws, nbytes) == L.ERR_INVALID, c
    assert call(C999, 0, ws, nbytes) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 0xA5).all() and it.cpu().tolist() == [-7]
    assert call(C999, 1024, ws, nbytes) == 0                                  # and the same buffers are fine for a valid call
    assert it.cpu().tolist() == [1024]


# ---------------------------------------------------------------------------------------------------------------- 8
def _feature_case():
    """400 points with descriptors that match their partner exactly for the inliers of a corr_case: the feature search finds them."""
    p0, p1, inl = gi.corr_case(31, 400, gi.rigid(*RC.T0_ARGS), 0.5, noise=0.03)
    F = gi.unit_feats(5, 400)
    return p0, p1, F, F.copy()


def test_the_o3d_shim_and_the_registration_call():
    from eyoc_amd import o3d, registration as reg
    p0, p1, F0, F1 = _feature_case()
    r = o3d.pipelines.registration
    pc = []
    for pts in (p0, p1):
        c = o3d.geometry.PointCloud()
        c.points = o3d.utility.Vector3dVector(pts.astype(np.float64))
        pc.append(c)
    feats = []
    for F in (F0, F1):
        f = r.Feature()
        f.data = np.ascontiguousarray(F.astype(np.float64).T)
        feats.append(f)
    checkers = [r.CorrespondenceCheckerBasedOnEdgeLength(0.9), r.CorrespondenceCheckerBasedOnDistance(THR)]
    got = r.registration_ransac_based_on_feature_matching(pc[0], pc[1], feats[0], feats[1], False, THR,
                                                          r.TransformationEstimationPointToPoint(False), 4, checkers,
                                                          r.RANSACConvergenceCriteria(100000, 0.999), seed=3)
    want = reg.registration_ransac_based_on_feature_matching(p0, p1, F0, F1, False, THR, criteria=(100000, 0.999), seed=3, confidence=0.999)
    assert 0 < got.iterations < 100000 and got.iterations == want.iterations
    assert got.best_hypothesis == want.best_hypothesis and got.inliers == want.inliers and got.survivors == want.survivors
    assert np.array_equal(got.transformation, want.transformation)
    # without the keyword the criteria's confidence is ignored, as it always was: the record of the full run
    full = reg.registration_ransac_based_on_feature_matching(p0, p1, F0, F1, False, THR, criteria=(100000, 0.999), seed=3)
    idx = torch.arange(400)
    today = reg.ransac_from_correspondences(p0, p1, idx, THR, 100000, seed=3)
    assert full.iterations == 0 and full.survivors == today.survivors > want.survivors and full.best_hypothesis == today.best_hypothesis
    assert np.array_equal(full.transformation, today.transformation)


def test_the_pipeline_with_a_confidence():
    import test_gpu_mutual as M
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import DeviceBatch, RegistrationPipeline
    pairs = [syn.make_pair(40 + s, beams=16, azimuths=500, band=None) for s in range(3)]
    batch = DeviceBatch(pairs, [40, 41, 42], torch.device("cuda"), n_points=M.N_POINTS, descriptor=dict(inlier_ratio=0.3))
    model = M._model()
    full = RegistrationPipeline(model, M._cfg()).register(batch, seed=7)
    cfg = M._cfg(ransac_confidence=0.999, ransac_first_check=1024)
    pipe = RegistrationPipeline(model, cfg)
    early = pipe.register(batch, seed=7)
    from eyoc_amd.metrics import registration_errors
    n_ok = 0
    for p, (a, b) in enumerate(zip(full, early)):
        T_gt = np.asarray(pairs[p]["T_gt"], np.float32)
        ok_full = registration_errors(a.transformation.astype(np.float32), T_gt, cfg.rte_thresh, cfg.rre_thresh)[2]
        ok_early = registration_errors(b.transformation.astype(np.float32), T_gt, cfg.rte_thresh, cfg.rre_thresh)[2]
        print(f"pair {p}: full inliers {a.inliers} ok {ok_full}; confidence 0.999 inliers {b.inliers} iterations {b.iterations} ok {ok_early}")
        assert a.iterations == 0
        if ok_full:
            n_ok += 1
            assert ok_early and 0 < b.iterations < cfg.ransac_max_iteration, p
    assert n_ok >= 2
    for tail in (False, True):
        pending = pipe.enqueue(batch, seed=7, tail_stream=tail)
        host, _ = pending.wait()
        assert tuple(host.shape) == (3, C.sizeof(M._L().RansacResult))
        assert pending.iterations.tolist() == [r.iterations for r in early]
        from eyoc_amd import registration as reg
        for p, r in enumerate(early):
            d = reg.decode_ransac_result(host[p], M.N_POINTS)
            assert d.best_hypothesis == r.best_hypothesis and d.inliers == r.inliers and np.array_equal(d.transformation, r.transformation)
    torch.cuda.synchronize()
