"""Per-pair failure isolation end to end: the drop kernel against numpy, the isolating voxeliser against the plain one, and a step
that registers past faulty pairs - byte for byte what the same kernels give on a batch the test reduced itself with numpy.

Inputs that make a call return an error code are used; nothing here is built to fault the GPU.  Every test first checks on the host
that the entry points and switches exist (``_feature``) and fails there, before anything degenerate is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_POINTS = 2000
DUP_MSG = "eyoc_maps_build: 1 duplicate coordinate rows (a sparse tensor needs unique coordinates)"
RANGE_MSG = "eyoc_maps_build: 1 coordinate rows outside the supported key range"


def _feature():
    from eyoc_amd import _lib as L
    from eyoc_amd import harness
    lib = L.load()
    for name in ("eyoc_batch_drop", "eyoc_batch_drop_workspace_bytes", "eyoc_remap_rows", "eyoc_voxelize_batched_isolating",
                 "eyoc_maps_last_fault_batches", "eyoc_registration_accept_degenerate"):
        assert hasattr(lib, name), f"{name} is missing: no launch on degenerate input"
    assert harness.RegistrationConfig().isolate_failures is False
    assert hasattr(harness.DeviceBatch, "without_pairs") and hasattr(harness, "DROPPED")
    return L, lib


# ---- 1. the drop kernel against numpy

def _collated(n, batches, c, seed):
    """``n`` rows spread over ``batches``, shuffled so that the clouds interleave."""
    rng = np.random.default_rng(seed)
    coords = np.concatenate([rng.choice(batches, (n, 1)), rng.integers(-500, 500, (n, 3))], 1).astype(np.int32)
    feats = None if c == 0 else rng.normal(size=(n, c)).astype(np.float32)
    return coords, feats


@pytest.mark.parametrize("c", [1, 32, 0, 6, 3])
def test_batch_drop_equals_numpy(c):
    _feature()
    from eyoc_amd.isolate import batch_drop, batch_mask, remap_rows
    layouts = ([0, 3, 5, 700, 701], [0, 3, 5, 9, 700, 701, 1023], [1, 2, 3, 4, 5, 6, 7, 8, 9])
    masks = ([], None, [3, 701], [3, 44], [0], [9, 1023, 5])          # None: everything; 44 is absent from every layout
    case = 0
    for n in (0, 1, 63, 100, 2048, 2049, 5000, 70001):                # below, at and above one scan tile of 2048 rows
        for batches in layouts if n in (100, 5000) else layouts[:1]:
            for drop in masks:
                case += 1
                drop = list(batches) if drop is None else drop
                coords, feats = _collated(n, batches, c, case)
                if n > 10:
                    coords[5, 0], coords[7, 0] = 1024, -1             # rows outside [0, 1024) have no mask bit: they stay
                keep = ~np.isin(coords[:, 0], drop)
                want_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
                d_coords, d_feats = torch.from_numpy(coords).cuda(), None if feats is None else torch.from_numpy(feats).cuda()
                runs = [batch_drop(d_coords, d_feats, batch_mask(drop) if case % 2 else drop) for _ in range(2)]
                for got_c, got_f, got_map, kept in runs:
                    np.testing.assert_array_equal(got_c.cpu().numpy(), coords[keep], err_msg=f"coords n={n} drop={drop}")
                    if feats is not None:
                        assert got_f.cpu().numpy().tobytes() == feats[keep].tobytes(), f"feats n={n} c={c} drop={drop}"
                    np.testing.assert_array_equal(got_map.cpu().numpy(), want_map)
                    inside = keep & (coords[:, 0] >= 0) & (coords[:, 0] < 1024)
                    np.testing.assert_array_equal(kept, np.bincount(coords[inside, 0], minlength=1024))
                    assert len(got_c) == int(keep.sum())
                np.testing.assert_array_equal(d_coords.cpu().numpy(), coords)                  # the input is not modified
                if n:
                    idx = np.random.default_rng(case).integers(0, n, 777)
                    got = remap_rows(torch.from_numpy(idx).cuda(), runs[0][2]).cpu().numpy()
                    np.testing.assert_array_equal(got, want_map[idx].astype(np.int64))
    far = remap_rows(torch.tensor([-1, 0, 70001, 1 << 40], dtype=torch.int64).cuda(), runs[0][2]).cpu().numpy()
    assert far[0] == -1 and far[2] == -1 and far[3] == -1 and far[1] == want_map[0]


def test_batch_drop_refuses_bad_arguments():
    L, lib = _feature()
    ctx = L.ctx(0)
    n_kept = C.c_int(-1)
    mask = np.zeros(32, np.uint32)
    assert lib.eyoc_batch_drop(ctx, None, None, 5, 0, mask.ctypes.data, None, None, None, C.byref(n_kept), None, None, 0, None) == L.ERR_INVALID
    assert lib.eyoc_batch_drop(ctx, None, None, 0, 0, mask.ctypes.data, None, None, None, C.byref(n_kept), None, None, 0, None) == 0
    assert n_kept.value == 0                                                                    # n = 0 launches nothing
    coords = torch.zeros((5, 4), dtype=torch.int32).cuda()
    out, rm = torch.empty_like(coords), torch.empty(5, dtype=torch.int32).cuda()
    ws = L.workspace(16, coords.device)
    rc = lib.eyoc_batch_drop(ctx, L.ptr(coords), None, 5, 0, mask.ctypes.data, L.ptr(out), None, L.ptr(rm), C.byref(n_kept), None,
                             L.ptr(ws), 16, None)
    assert rc == L.ERR_WORKSPACE


# ---- 2. the isolating voxeliser

LIM = (1 << 17) - 16


def _numpy_faults(cloud, voxel):
    x = np.asarray(cloud, np.float32)[:, :3]
    finite = np.isfinite(x).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(x[finite] / np.float32(voxel)).astype(np.float64)
    return int(((q < -LIM) | (q >= LIM)).any(1).sum()), int((~finite).sum())


@pytest.fixture(scope="module")
def sweeps():
    from eyoc_amd import synthetic as syn
    pairs = [syn.make_pair(40 + s, keep_raw=True, beams=32, azimuths=1000, band=None) for s in range(4)]
    return [np.ascontiguousarray(p[k], np.float32) for p in pairs for k in ("raw0", "raw1")]


def test_isolating_voxeliser_reports_faults_per_cloud(sweeps):
    L, lib = _feature()
    from eyoc_amd.voxelize import sparse_quantize_batch
    clouds = [c.copy() for c in sweeps]
    clouds[1][100] = (1e6, 0.0, 0.0)                   # one point 1000 km out
    clouds[3][7, 1] = np.nan
    clouds[4][0, 2] = np.inf
    clouds[4][len(clouds[4]) - 1, 0] = -np.inf
    clouds[4][50] = (0.0, -1e6, 3.0)                   # and a finite one out of range in the same cloud
    clouds[6] = np.zeros((0, 3), np.float32)
    clean = [0, 2, 5, 7]
    base = 3
    coords, sel, xyz, off, faults = sparse_quantize_batch(clouds, 0.3, base, isolate=True)
    want = np.array([_numpy_faults(c, 0.3) for c in clouds], np.int32)
    np.testing.assert_array_equal(faults, want)
    assert want[1].tolist() == [1, 0] and want[3].tolist() == [0, 1] and want[4].tolist() == [1, 2] and not want[clean].any()
    assert faults.dtype == np.int32 and off[-1] == len(coords) == len(sel) == len(xyz)
    for b in range(len(clouds)):
        rows = slice(int(off[b]), int(off[b + 1]))
        if b not in clean:
            assert off[b] == off[b + 1], f"cloud {b} must contribute no voxels"
            continue
        c1, s1, x1, o1 = sparse_quantize_batch([clouds[b]], 0.3, base + b)          # the plain call, same batch index
        assert o1[1] == off[b + 1] - off[b] > 0
        np.testing.assert_array_equal(coords[rows].cpu().numpy(), c1.cpu().numpy())
        np.testing.assert_array_equal(sel[rows].cpu().numpy(), s1.cpu().numpy())
        assert xyz[rows].cpu().numpy().tobytes() == x1.cpu().numpy().tobytes()
    # no faulty cloud: the whole output is the plain call's, bit for bit
    good = [sweeps[b] for b in (0, 1, 2)] + [np.zeros((0, 3), np.float32), sweeps[3]]
    a = sparse_quantize_batch(good, 0.3, 1, isolate=True)
    b_ = sparse_quantize_batch(good, 0.3, 1)
    assert not a[4].any() and a[4].shape == (5, 2)
    for x, y in zip(a[:3], b_[:3]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    np.testing.assert_array_equal(a[3], b_[3])
    # the plain call still fails on poisoned input, with its present message
    with pytest.raises(L.EyocError) as ei:
        sparse_quantize_batch(clouds, 0.3, base)
    assert ei.value.code == L.ERR_RANGE and "eyoc_voxelize_batched: " in str(ei.value)
    only_far = [sweeps[0], clouds[1], sweeps[2]]
    with pytest.raises(L.EyocError) as ei:
        sparse_quantize_batch(only_far, 0.3, 0)
    assert "eyoc_voxelize_batched: 1 points fall outside the key range (|c| < 2^17 - 16), the first of them in cloud 1" in str(ei.value)
    # one cloud, every cloud empty
    one = sparse_quantize_batch([clouds[1]], 0.3, 9, isolate=True)
    assert one[4].tolist() == [[1, 0]] and len(one[0]) == 0 and one[3].tolist() == [0, 0]
    none = sparse_quantize_batch([np.zeros((0, 3), np.float32)] * 2, 0.3, 0, isolate=True)
    assert none[4].tolist() == [[0, 0], [0, 0]] and len(none[0]) == 0


# ---- 3. the step

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
def eight_pairs():
    from eyoc_amd import synthetic as syn
    return [syn.make_pair(300 + s) for s in range(8)]


SEEDS = list(range(300, 308))
CASES = {"duplicate": {3: "dup"}, "range_then_duplicate": {3: "dup", 5: "range"}}


def _poisoned(pairs, case):
    """Pair 3's first cloud gets one duplicated row (features too); pair 5's second cloud a row at 1 << 17."""
    out = [dict(p) for p in pairs]
    for p, kind in CASES[case].items():
        if kind == "dup":
            for k in ("coords0", "feats0", "xyz0"):
                out[p][k] = np.concatenate([out[p][k], out[p][k][10:11]])
        else:
            c = out[p]["coords1"].copy()
            c[7, 1] = 1 << 17
            out[p]["coords1"] = c
    return out


def _batch(pairs):
    from eyoc_amd.harness import DeviceBatch
    return DeviceBatch(pairs, SEEDS, torch.device("cuda"), n_points=N_POINTS, descriptor=dict(inlier_ratio=0.3))


def _bits(case):
    from eyoc_amd import harness as h
    bits = np.zeros(8, np.int64)
    for p, kind in CASES[case].items():
        bits[p] = h.DROPPED_DUPLICATE if kind == "dup" else h.DROPPED_RANGE
    return bits


def _snapshot(batch):
    return {k: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else np.array(v).copy())
            for k, v in vars(batch).items() if isinstance(v, (torch.Tensor, np.ndarray, list)) and k != "planted"}


def _reduced_with_numpy(batch, dropped):
    """The faulty pairs' rows removed by the test itself (boolean mask, batch indices kept, sel through a cumsum) -> host arrays of the
    live pairs.  Only what the parent commit's API offers is used from here on."""
    n = batch.n_points
    coords, feats = batch.coords.cpu().numpy(), batch.feats.cpu().numpy()
    live = np.flatnonzero(dropped == 0)
    keep = ~np.isin(coords[:, 0], [2 * p + i for p in np.flatnonzero(dropped) for i in (0, 1)])
    row_map = np.cumsum(keep) - 1
    sel0, sel1 = (s.cpu().numpy().reshape(8, n)[live] for s in (batch.sel0, batch.sel1))
    assert keep[sel0].all() and keep[sel1].all()
    G0, G1 = (None if g is None else g.cpu().numpy().reshape(8, n, -1)[live].reshape(len(live) * n, -1) for g in (batch.G0, batch.G1))
    return dict(coords=coords[keep], feats=feats[keep], sel0=row_map[sel0].reshape(-1), sel1=row_map[sel1].reshape(-1), G0=G0, G1=G1,
                xyz0=batch.xyz0.cpu().numpy()[live], xyz1=batch.xyz1.cpu().numpy()[live], beta=batch.beta, n=n)


def _equivalent_records(L, model, cfg, r, dropped, seed):
    """The step on the reduced batch ``r`` from the parent's API alone: forward, row gather, nearest neighbour over the live segments,
    and the batched back-end with an EMPTY segment in every dropped slot (``accept_degenerate`` on), same ``seed``."""
    import eyoc_amd
    from eyoc_amd import registration as reg
    from eyoc_amd.eval import gather_rows, knn1_segmented
    dev = torch.device("cuda")
    P, n = len(dropped), r["n"]
    Lv = int((dropped == 0).sum())
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    with torch.no_grad():
        F = model(eyoc_amd.SparseTensor(up(r["feats"]), coordinates=up(r["coords"]))).F
    F0 = gather_rows(F, up(r["sel0"]), up(r["G0"]), r["beta"])
    F1 = gather_rows(F, up(r["sel1"]), up(r["G1"]), r["beta"])
    prev = L.knob("eyoc_registration_accept_degenerate", 1)
    try:
        if cfg.use_RANSAC:
            live_seg = np.arange(Lv + 1) * n
            nn = knn1_segmented(F0, F1, live_seg, live_seg, "SquareL2", return_distance=False)
            seg = np.concatenate([[0], np.cumsum(np.where(dropped == 0, n, 0))])
            res = reg.ransac_batched_from_correspondences(up(r["xyz0"]).reshape(-1, 3), up(r["xyz1"]).reshape(-1, 3), nn, seg, seg,
                                                          cfg.voxel_size, cfg.ransac_max_iteration, seed=seed)
            return res.cpu().numpy()
        m = reg.Matcher(**cfg.sc2pcr)
        k = int(m.num_node)
        draws = np.random.RandomState(seed).randint(0, n, (P, 2, k))[dropped == 0]                # drawn for all P, used for the live
        draws = draws + (np.arange(Lv) * n)[:, None, None]
        gs, gt = up(draws[:, 0].reshape(-1)), up(draws[:, 1].reshape(-1))
        live_seg = np.arange(Lv + 1) * k
        nn = knn1_segmented(F0[gs], F1[gt], live_seg, live_seg, "GemmL2", return_distance=False)
        nn = nn + torch.arange(Lv, device=dev).repeat_interleave(k) * k
        src, tgt = up(r["xyz0"]).reshape(-1, 3)[gs], up(r["xyz1"]).reshape(-1, 3)[gt][nn]
        keep = min(k, int(m.max_points))
        assert keep == k
        seg = np.concatenate([[0], np.cumsum(np.where(dropped == 0, keep, 0))])
        T, _, _ = m.SC2_PCR_packed(src.contiguous(), tgt.contiguous(), seg)
        return T.cpu().numpy()
    finally:
        L.knob("eyoc_registration_accept_degenerate", prev)


def _transforms(cfg, records):
    """[P, 4, 4] float64 from the RANSAC records / the SC2-PCR output."""
    from eyoc_amd import registration as reg
    if cfg.use_RANSAC:
        return np.stack([reg.decode_ransac_result(torch.from_numpy(records[p]), N_POINTS).transformation for p in range(len(records))])
    return records.astype(np.float64)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("use_ransac", [True, False], ids=["ransac", "sc2pcr"])
def test_step_registers_past_faulty_pairs(eight_pairs, use_ransac, case):
    L, lib = _feature()
    from eyoc_amd import harness as h
    model = _model()
    bits = _bits(case)
    live = np.flatnonzero(bits == 0)
    batch = _batch(_poisoned(eight_pairs, case))
    before = _snapshot(batch)
    assert not batch.dropped.any()
    want = _equivalent_records(L, model, _cfg(use_ransac), _reduced_with_numpy(batch, bits), bits, seed=5)
    pipe = h.RegistrationPipeline(model, _cfg(use_ransac, isolate_failures=True))

    # register: records on the device, then the decoded results
    got = pipe.register(batch, seed=5, return_device=True).cpu().numpy()
    assert got.shape == want.shape and got.shape[0] == 8
    assert got.tobytes() == want.tobytes(), f"records differ in pairs {[p for p in range(8) if got[p].tobytes() != want[p].tobytes()]}"
    assert pipe.dropped_pairs == len(CASES[case])
    np.testing.assert_array_equal(pipe.registered_batch.dropped, bits)
    res = pipe.register(batch, seed=5)
    assert pipe.dropped_pairs == 2 * len(CASES[case]) and len(res) == 8
    T_want = _transforms(_cfg(use_ransac), want)
    for p in range(8):
        assert res[p].status == bits[p]
        if bits[p]:
            assert np.isnan(res[p].transformation).all() and res[p].fitness == 0 and res[p].inliers == 0 and res[p].best_hypothesis == -1
            assert np.isnan(T_want[p]).all()                     # the back-end's own failed record sits in the dropped slot
        else:
            np.testing.assert_array_equal(res[p].transformation, T_want[p])
    rows = pipe.evaluate(batch, res)
    for p in np.flatnonzero(bits):
        assert rows[p]["success"] is False and np.isnan(rows[p]["rte"]) and np.isnan(rows[p]["rre_deg"])
    if use_ransac:
        ratios = pipe.correspondence_inlier_ratio(pipe.registered_batch)
        assert all(np.isnan(ratios[p]) == bool(bits[p]) for p in range(8))

    # enqueue, two streams; then the three-stream loop's handle from prepare_maps
    pend = pipe.enqueue(batch, seed=5, slot=0, tail_stream=True)
    host, overflow = pend.wait()
    assert not overflow and host.numpy().tobytes() == want.tobytes()
    np.testing.assert_array_equal(pend.status, bits)
    handle = pipe.prepare_maps(batch)
    assert len(handle) == 3 and handle[2] is not batch
    np.testing.assert_array_equal(handle[2].dropped, bits)
    pend = pipe.enqueue(batch, seed=5, maps=handle, slot=1, tail_stream=True)
    nxt = pipe.prepare_maps(batch, after=pipe.featured)           # the next build on the side stream, beside this step's tail
    host, _ = pend.wait()
    assert host.numpy().tobytes() == want.tobytes()
    np.testing.assert_array_equal(pend.status, bits)
    assert pipe.enqueue(batch, seed=5, maps=nxt, slot=0).wait()[0].numpy().tobytes() == want.tobytes()
    torch.cuda.synchronize()

    # the source batch is as it was
    after = _snapshot(batch)
    assert before.keys() == after.keys()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k

    # against the clean 8-pair run: every live pair registers under the config's own thresholds (no byte identity asserted: the
    # automatic kernel choice depends on the row counts)
    clean_pipe = h.RegistrationPipeline(model, _cfg(use_ransac))
    clean_batch = _batch(eight_pairs)
    clean = clean_pipe.register(clean_batch, seed=5)
    assert all(r["success"] for r in clean_pipe.evaluate(clean_batch, clean)), "precondition: the clean run registers 8 of 8"
    assert all(rows[p]["success"] for p in live), [rows[p] for p in live]
    same = [bool(np.array_equal(res[p].transformation, clean[p].transformation)) for p in live]
    print(f"isolation {case} {'ransac' if use_ransac else 'sc2pcr'}: live pairs byte-identical to the clean run: {sum(same)} of {len(same)}")

    # isolate_failures on a clean batch: nothing dropped, the records are those of the plain pipeline
    a = pipe.register(clean_batch, seed=5, return_device=True).cpu().numpy()
    b = clean_pipe.register(clean_batch, seed=5, return_device=True).cpu().numpy()
    assert a.tobytes() == b.tobytes() and pipe.registered_batch is clean_batch and not clean_batch.dropped.any()


@pytest.mark.parametrize("case", sorted(CASES))
def test_without_isolation_the_poisoned_batch_fails_as_before(eight_pairs, case):
    """``isolate_failures`` off (the default): the same code and message as ever.  This half needs nothing new."""
    from eyoc_amd import _lib as L
    from eyoc_amd.harness import RegistrationPipeline
    batch = _batch(_poisoned(eight_pairs, case))
    pipe = RegistrationPipeline(_model(), _cfg(True))
    for run in (lambda: pipe.register(batch, seed=5), lambda: pipe.prepare_maps(batch), lambda: pipe.enqueue(batch, seed=5, tail_stream=True)):
        with pytest.raises(L.EyocError) as ei:
            run()
        torch.cuda.synchronize()
        if case == "duplicate":
            assert ei.value.code == L.ERR_DUPLICATE and DUP_MSG in str(ei.value)
        else:
            assert ei.value.code == L.ERR_RANGE and RANGE_MSG in str(ei.value)      # the range check comes first


def test_without_pairs_by_hand(eight_pairs):
    """``without_pairs`` on a clean batch, twice, against numpy; the drop accumulates and the source stays."""
    _feature()
    from eyoc_amd import harness as h
    batch = _batch(eight_pairs)
    before = _snapshot(batch)
    one = batch.without_pairs({2: h.DROPPED_RANGE})
    two = one.without_pairs([0, 0, h.DROPPED_EMPTY, 0, 0, 0, 0, h.DROPPED_DUPLICATE])
    bits = np.array([0, 0, h.DROPPED_RANGE | h.DROPPED_EMPTY, 0, 0, 0, 0, h.DROPPED_DUPLICATE])
    np.testing.assert_array_equal(two.dropped, bits)
    r = _reduced_with_numpy(batch, bits)
    np.testing.assert_array_equal(two.coords.cpu().numpy(), r["coords"])
    assert two.feats.cpu().numpy().tobytes() == r["feats"].tobytes()
    np.testing.assert_array_equal(two.sel0.cpu().numpy(), r["sel0"])
    np.testing.assert_array_equal(two.sel1.cpu().numpy(), r["sel1"])
    for k in ("xyz0", "xyz1", "G0", "G1"):
        assert getattr(two, k).cpu().numpy().tobytes() == r[k].tobytes(), k
    sizes = np.array(batch.sizes)
    sizes[[4, 5, 14, 15]] = 0
    assert two.sizes == sizes.tolist() and two.offsets.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert two.seg.tolist() == np.concatenate([[0], np.cumsum(np.where(bits == 0, N_POINTS, 0))]).tolist()
    assert two.P == 8 and len(two.T_gt) == 8 and two.n_points == N_POINTS and two.voxels == len(r["coords"])
    after = _snapshot(batch)
    assert all(before[k].tobytes() == after[k].tobytes() for k in before) and not batch.dropped.any()
    with pytest.raises(ValueError):
        batch.without_pairs([1 << 4] * 8)                         # not a DROPPED_* bit


def test_neighbour_search_accepts_empty_segments_between_live_ones():
    """The step hands ``knn1_segmented`` the batch's segments, empty ones for dropped pairs included: the live rows must get the
    indices (and distances) of the live segments alone, with and without the MFMA pre-filter (small / large segments)."""
    from eyoc_amd.eval import knn1_segmented
    torch.manual_seed(0)
    for n in (500, 5000):
        seg = np.concatenate([[0], np.cumsum([n, 0, n + 100, 0, 0, n, n, n, n, n])])
        live = np.unique(seg)
        A, B = (torch.nn.functional.normalize(torch.randn(int(seg[-1]), 32, device="cuda"), dim=1) for _ in range(2))
        for dist in ("SquareL2", "GemmL2"):
            assert torch.equal(knn1_segmented(A, B, seg, seg, dist, return_distance=False),
                               knn1_segmented(A, B, live, live, dist, return_distance=False)), (n, dist)
        (i0, d0), (i1, d1) = knn1_segmented(A, B, seg, seg), knn1_segmented(A, B, live, live)
        assert torch.equal(i0, i1) and torch.equal(d0, d1) and int(i0.max()) < n + 100


# ---- 4. from raw scans

def test_from_scans_drops_faulty_pairs_at_construction():
    L, lib = _feature()
    from eyoc_amd import harness as h
    from eyoc_amd import synthetic as syn
    dev = torch.device("cuda")
    seeds = list(range(60, 68))
    pairs = [syn.make_pair(s, keep_raw=True, beams=32, azimuths=1000, band=None) for s in seeds]
    scans = [(p["raw0"].copy(), p["raw1"].copy()) for p in pairs]
    scans[2][1][11] = (1e6, 1.0, 1.0)                              # pair 2: a far point in the target sweep
    scans[5] = (np.zeros((0, 3), np.float32), scans[5][1])         # pair 5: an empty source sweep
    scans[6][0][3, 2] = np.nan                                     # pair 6: a NaN
    T_gt = [p["T_gt"] for p in pairs]
    bits = np.zeros(8, np.int64)
    bits[2], bits[5], bits[6] = h.DROPPED_RANGE, h.DROPPED_EMPTY, h.DROPPED_NONFINITE
    live = np.flatnonzero(bits == 0)
    with pytest.raises(L.EyocError):
        h.DeviceBatch.from_scans(scans[:3], T_gt[:3], seeds[:3], dev, n_points=N_POINTS)          # the plain constructor still refuses
    got = h.DeviceBatch.from_scans(scans, T_gt, seeds, dev, n_points=N_POINTS, isolate=True)
    ref = h.DeviceBatch.from_scans([scans[p] for p in live], [T_gt[p] for p in live], [seeds[p] for p in live], dev, n_points=N_POINTS)
    np.testing.assert_array_equal(got.dropped, bits)
    # the clean pairs re-slotted: cloud 2 q + i of the reference is cloud 2 p + i here
    slot = np.array([2 * p + i for p in live for i in (0, 1)])
    coords = ref.coords.cpu().numpy().copy()
    coords[:, 0] = slot[coords[:, 0]]
    np.testing.assert_array_equal(got.coords.cpu().numpy(), coords)
    sizes = np.zeros(16, np.int64)
    sizes[slot] = ref.sizes
    assert got.sizes == sizes.tolist() and got.offsets.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    for k in ("feats", "sel0", "sel1", "xyz0", "xyz1"):
        a, b = getattr(got, k).cpu().numpy(), getattr(ref, k).cpu().numpy()
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert got.G0 is None and got.G1 is None and got.P == 8 and got.n_points == N_POINTS and got.counts == [N_POINTS] * 8
    assert got.seg.tolist() == np.concatenate([[0], np.cumsum(np.where(bits == 0, N_POINTS, 0))]).tolist()
    assert all(np.array_equal(a, np.asarray(b, np.float32)) for a, b in zip(got.T_gt, T_gt))
    # host-voxelised pairs with an empty cloud: the same treatment in the plain constructor
    vox = [dict(p) for p in pairs[:3]]
    vox[1]["coords1"], vox[1]["feats1"], vox[1]["xyz1"] = vox[1]["coords1"][:0], vox[1]["feats1"][:0], vox[1]["xyz1"][:0]
    hb = h.DeviceBatch(vox, seeds[:3], dev, n_points=N_POINTS, isolate=True)
    assert hb.dropped.tolist() == [0, h.DROPPED_EMPTY, 0] and hb.sizes[2] == 0 and hb.sizes[3] == 0 and hb.xyz0.shape[0] == 2
    assert hb.voxels == len(hb.coords) == sum(hb.sizes)
    # the step: the records of the numpy-built equivalent, both back-ends
    model = _model()
    r = dict(coords=coords, feats=ref.feats.cpu().numpy(), sel0=ref.sel0.cpu().numpy(), sel1=ref.sel1.cpu().numpy(), G0=None, G1=None,
             xyz0=ref.xyz0.cpu().numpy(), xyz1=ref.xyz1.cpu().numpy(), beta=0.0, n=N_POINTS)
    for use_ransac in (True, False):
        want = _equivalent_records(L, model, _cfg(use_ransac), r, bits, seed=9)
        pipe = h.RegistrationPipeline(model, _cfg(use_ransac, isolate_failures=True))
        out = pipe.register(got, seed=9, return_device=True).cpu().numpy()
        assert out.tobytes() == want.tobytes(), use_ransac
        res = pipe.register(got, seed=9)
        assert [r_.status for r_ in res] == bits.tolist() and pipe.dropped_pairs == 6


# ---- 5. giving up

def test_a_row_outside_every_mask_raises_the_original_error(eight_pairs):
    L, lib = _feature()
    from eyoc_amd import harness as h
    batch = _batch(eight_pairs[:2])
    batch.coords = batch.coords.clone()
    batch.coords[17, 0] = 1024                                     # its own batch index is out of range: no mask bit names it
    pipe = h.RegistrationPipeline(_model(), _cfg(True, isolate_failures=True))
    for run in (lambda: pipe.register(batch, seed=1), lambda: pipe.prepare_maps(batch)):
        with pytest.raises(L.EyocError) as ei:
            run()
        torch.cuda.synchronize()
        assert ei.value.code == L.ERR_RANGE and RANGE_MSG in str(ei.value)
    assert L.fault_batches() == ([], []) and not batch.dropped.any() and pipe.dropped_pairs == 0
