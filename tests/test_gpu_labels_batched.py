"""GPU parity of the batched label route (eyoc_lowe_topk_segmented, eyoc_pair_filter_batched, eyoc_posed_nn_grid and the Python built on
them: match_and_filter_corr_batched, correspondences_under_pose_batched, corr_through_registration, label_step) against the per-pair
route, which tests/test_gpu_labels.py and the goldens pin to the oracle.  The contracts make the two routes byte-identical: every
comparison is assert_array_equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32


def unit(rng, n, c=32):
    f = rng.normal(size=(n, c)).astype(F32)
    return f / np.linalg.norm(f, axis=1, keepdims=True).astype(F32)


def rigid(rng, max_deg=8.0, max_t=4.0):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = np.deg2rad(rng.uniform(-max_deg, max_deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = rng.uniform(-max_t, max_t, 3)
    return T.astype(F32)


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# 1. segmented top-k
# ---------------------------------------------------------------------------------------------------------------------
def topk_inputs(sizes, seed):
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    d1 = rng.uniform(0, 1.5, n).astype(F32)
    d2 = (d1 + rng.uniform(0, 0.5, n).astype(F32)).astype(F32)
    for a, b in zip(offsets(sizes)[:-1], offsets(sizes)[1:]):
        ln = b - a
        d1[a:a + max(ln // 16, 1)] = 0.0                                 # clamp branch
        if ln >= 40:
            d2[a + 10:a + 20] = d1[a + 10:a + 20]                        # ratio exactly 1: weight 0, ties in query order
        if ln >= 130:                                                    # the LARGEST weight 100 times over, scattered: the tie straddles rank 1 and rank 64
            rows = a + rng.choice(ln, 100, replace=False)
            d1[rows], d2[rows] = 0.0, 1.25
    return d1, d2


@pytest.mark.parametrize("sizes,ks", [([700, 64, 130, 1300], (1, 64)), ([40] * 130, (40,))])
def test_segmented_topk_equals_per_segment_topk(sizes, ks):
    import eyoc_amd
    d1, d2 = topk_inputs(sizes, len(sizes))
    seg = offsets(sizes)
    D1, D2 = cuda(d1), cuda(d2)
    for k in ks:
        idx, w = eyoc_amd.lowe_topk_segmented(D1, D2, seg, k, return_weights=True)
        assert idx.shape == (len(sizes), k) and w.shape == (len(sizes), k)
        idx, w = idx.cpu().numpy(), w.cpu().numpy()
        for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
            ri, rw = eyoc_amd.lowe_topk(D1[a:b], D2[a:b], k)
            np.testing.assert_array_equal(idx[s], ri.cpu().numpy(), err_msg=f"segment {s} k {k}")
            np.testing.assert_array_equal(w[s], rw.cpu().numpy(), err_msg=f"segment {s} k {k}")
        # mode 1: weight = d1, the order of the stable fp64 argsort of the feature_filter = "None" branch
        got = eyoc_amd.lowe_topk_segmented(D1, None, seg, k, mode=1).cpu().numpy()
        for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
            np.testing.assert_array_equal(got[s], np.argsort(-d1[a:b].astype(np.float64), kind="stable")[:k], err_msg=f"segment {s} k {k}")
    if 1300 in sizes:                                                    # the planted tie really straddles rank 64
        a = seg[3]
        top = eyoc_amd.lowe_topk_segmented(D1, D2, seg, 64, return_weights=True)[1][3].cpu().numpy()
        assert (top == top[0]).all() and ((d1[a:seg[4]] == 0) & (d2[a:seg[4]] == 1.25)).sum() == 100


# ---------------------------------------------------------------------------------------------------------------------
# 2. batched filter
# ---------------------------------------------------------------------------------------------------------------------
M_LIST = [0, 1, 1024, 1025, 3000, 500, 500, 300]        # pair 5 keeps everything, pair 6 nothing, pair 7 has a NaN pose in mode 1
ALL, NONE, NANPOSE = 5, 6, 7


def synthetic_dist_sim_map(seed=0):
    """Six float64 slices [gap cells, distance cells] of the reference's shape family, similarity decaying with both coordinates."""
    rng = np.random.default_rng(seed)
    out = {}
    for i, shape in enumerate([(12, 16), (18, 16), (20, 18), (20, 18), (20, 18), (20, 18)]):
        gy, gx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        out[i] = np.clip(0.85 * np.exp(-0.12 * gy - 0.05 * gx) + 0.05 * rng.normal(size=shape), 0.0, 1.0)
    return out


def sphere(rng, n, lo, hi):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rng.uniform(lo, hi, (n, 1))).astype(F32)


def filter_case(mode, seed=7):
    rng = np.random.default_rng(seed + mode)
    P0s, P1s, i0s, i1s, Ts = [], [], [], [], []
    for b, m in enumerate(M_LIST):
        n0, n1 = int(rng.integers(200, 1500)), int(rng.integers(200, 1500))
        T = rigid(rng)
        if mode == 1:                                                   # residual under the pose on both sides of 2 m
            n1 = n0
            P0 = rng.uniform(-50, 50, (n0, 3)).astype(F32)
            scale = {ALL: 0.05, NONE: 40.0}.get(b, 1.2)
            noise = rng.normal(0, scale, (n0, 3)) + (100.0 if b == NONE else 0.0)
            P1 = ((P0.astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]) + noise).astype(F32)
            i0 = rng.integers(0, n0, m)
            i1 = np.where(rng.uniform(size=m) < (1.0 if b in (ALL, NONE) else 0.8), i0, rng.integers(0, n1, m))
            if b == NANPOSE:
                T = T.copy()
                T[1, 2] = np.nan
        else:                                                           # distances to the sensor on both sides of 20 m / all over the table
            lo, hi = {ALL: (21.0, 24.0) if mode == 0 else (6.0, 6.5), NONE: (1.0, 19.0) if mode == 0 else (76.0, 79.0)}.get(b, (2.0, 90.0))
            P0 = sphere(rng, n0, lo, hi)
            P1 = sphere(rng, n1, *((139.0, 141.0) if (mode == 2 and b == NONE) else (lo, hi)))
            i0, i1 = rng.integers(0, n0, m), rng.integers(0, n1, m)
        P0s.append(P0); P1s.append(P1); i0s.append(i0.astype(np.int64)); i1s.append(i1.astype(np.int64)); Ts.append(T)
    return P0s, P1s, i0s, i1s, Ts


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_batched_filter_equals_per_pair_filter(mode):
    import eyoc_amd
    from eyoc_amd import labels
    P0s, P1s, i0s, i1s, Ts = filter_case(mode)
    B = len(M_LIST)
    seg0, seg1, seg_m = offsets([len(p) for p in P0s]), offsets([len(p) for p in P1s]), offsets(M_LIST)
    P0, P1 = cuda(np.concatenate(P0s)), cuda(np.concatenate(P1s))
    i0, i1 = cuda(np.concatenate(i0s)), cuda(np.concatenate(i1s))
    table, gaps = synthetic_dist_sim_map(), [0, 4, 7, 12, 19, 3, 2, 100]
    kw = {}
    if mode == 0:
        kw = dict(radius=20.0)
    elif mode == 1:
        kw = dict(T=cuda(np.stack(Ts)), radius=2.0)
    else:
        host_tables, slices = labels._sim_slices(table, gaps)
        kw = dict(tables=cuda(host_tables), slices=slices, thresh=0.4)
    out, counts = eyoc_amd.pair_filter_batched(mode, P0, P1, i0, i1, seg0, seg1, seg_m, **kw)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    kept = []
    for b in range(B):
        a0, b0 = cuda(P0s[b]), cuda(P1s[b])
        if M_LIST[b] == 0:                                              # (the per-pair entry points refuse an empty list: NULL pointers)
            ref = torch.empty((0, 2), dtype=torch.int64)
        elif mode == 2:
            ref = eyoc_amd.similarity_filter(a0, b0, cuda(i0s[b]), cuda(i1s[b]), table, gaps[b], 0.4)
        else:
            ref = labels._pair_filter(mode, a0, b0, cuda(i0s[b]), cuda(i1s[b]), Ts[b] if mode == 1 else None, 20.0 if mode == 0 else 2.0)
        ref = ref.cpu().numpy()
        kept.append(len(ref))
        assert counts[b] == len(ref), (b, counts[b], len(ref))
        np.testing.assert_array_equal(out[seg_m[b]:seg_m[b] + counts[b]], ref, err_msg=f"pair {b}")
    assert kept[ALL] == M_LIST[ALL] and kept[NONE] == 0 and kept[0] == 0
    assert 0 < kept[3] < M_LIST[3] and 0 < kept[4] < M_LIST[4]
    if mode == 1:
        assert kept[NANPOSE] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. posed nearest neighbour on the cell grid
# ---------------------------------------------------------------------------------------------------------------------
R = F32(2.0)
EDGE = F32(2.0 + 2.0 ** -19)                  # the cell edge for max_dist = 2: 2 (1 + 2^-20), exact in fp32
BELOW = np.nextafter(R, F32(0))


def planted_pair():
    """Identity pose, coordinates exactly representable.  Returns (src, tgt, {case: (query row, expected target row)})."""
    src, tgt, want = [], [], {}

    def q(name, p, expect):
        want[name] = (len(src), expect)
        src.append(p)

    def t(p):
        tgt.append(p)
        return len(tgt) - 1
    dup = t((10, 10, 10)); t((10, 10, 10))                              # a duplicated target row: the lower one
    q("duplicate", (10.5, 10, 10), dup)
    # equidistant targets in different cells: x = 2.5 lies in cell 1, probed AFTER cell -1 (x = -0.5), and has the lower row
    late = t((2.5, -20, 0)); t((-0.5, -20, 0))
    q("tie across cells", (1.0, -20, 0), late)
    t((40, 2.0, 0))                                                     # exactly max_dist away: excluded
    q("at max_dist", (40, 0, 0), -1)
    inc = t((-40, float(BELOW), 0))                                     # one ulp inside: included
    q("below max_dist", (-40, 0, 0), inc)
    border = t((float(EDGE) - 1.0, 60, 60))                             # the query sits on a cell face
    q("cell border", (float(EDGE), 60, 60), border)
    neg = t((-34, -7.5, -60.5))
    q("negative", (-33.25, -7.5, -60), neg)
    q("nothing near", (0, 0, 70), -1)
    return np.array(src, F32), np.array(tgt, F32), want


def grid_batch():
    rng = np.random.default_rng(2024)
    sizes = [(int(rng.integers(50, 301)), int(rng.integers(50, 301))) for _ in range(70)] + [(5000, 6000)]
    srcs, tgts, Ts = [], [], []
    for n0, n1 in sizes:
        T = rigid(rng)
        P0 = rng.uniform(-30, 30, (n0, 3)).astype(F32) if n0 > 1000 else rng.uniform(-10, 10, (n0, 3)).astype(F32)
        m = min(n0, n1) * 2 // 3
        posed = (P0[:m].astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]) + rng.normal(0, 0.8, (m, 3))
        lim = 30 if n0 > 1000 else 10
        P1 = np.concatenate([posed, rng.uniform(-lim, lim, (n1 - m, 3))]).astype(F32)[rng.permutation(n1)]
        srcs.append(P0); tgts.append(P1); Ts.append(T)
    ps, pt, want = planted_pair()
    srcs += [ps, np.array([[1.0, 2.0, 3.0]], F32)]                      # + a single-point cloud on both sides
    tgts += [pt, np.array([[1.0, 2.0, 4.5]], F32)]
    Ts += [np.eye(4, dtype=F32), np.eye(4, dtype=F32)]
    return srcs, tgts, Ts, want


@pytest.fixture(scope="module")
def grid_reference():
    """The brute-force answer, once: knn2_segmented(pad(apply_pose(T, P0)), pad(P1)) and the fp32 gate."""
    import eyoc_amd
    from eyoc_amd import labels
    srcs, tgts, Ts, want = grid_batch()
    seg0, seg1 = offsets([len(p) for p in srcs]), offsets([len(p) for p in tgts])
    pad = lambda P: torch.cat([P, torch.zeros((P.shape[0], 1), device=P.device)], 1).contiguous()
    posed = torch.cat([labels.apply_pose(T, cuda(P)) for T, P in zip(Ts, srcs)])
    P1 = cuda(np.concatenate(tgts))
    idx, d1, _ = eyoc_amd.knn2_segmented(pad(posed), pad(P1), seg0, seg1)
    idx, d1 = idx.cpu().numpy(), d1.cpu().numpy()
    hit = np.sqrt(d1) < R                                               # fp32 square root, correctly rounded
    ref = dict(idx=np.where(hit, idx, -1), d2=np.where(hit, d1, F32(np.inf)).astype(F32))
    ref.update(srcs=srcs, tgts=tgts, Ts=Ts, want=want, seg0=seg0, seg1=seg1, P0=cuda(np.concatenate(srcs)), P1=P1, T=cuda(np.stack(Ts)))
    for v in (ref["idx"], ref["d2"]):
        v.setflags(write=False)
    return ref


def test_grid_nn_all_rows(grid_reference):
    import eyoc_amd
    g = grid_reference
    idx, d2, status = eyoc_amd.posed_nn_grid(g["P0"], g["P1"], g["seg0"], g["seg1"], g["T"], 2.0, return_d2=True)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert not status.cpu().numpy().any()
    np.testing.assert_array_equal(idx, g["idx"])
    np.testing.assert_array_equal(d2, g["d2"])
    frac = (g["idx"] >= 0).mean()
    assert 0.2 < frac < 0.95, frac
    base = g["seg0"][-3]                                                # the planted pair
    for name, (row, expect) in g["want"].items():
        assert idx[base + row] == expect, (name, idx[base + row], expect)
    assert d2[base + g["want"]["below max_dist"][0]] == BELOW * BELOW and d2[base + g["want"]["tie across cells"][0]] == 2.25
    assert idx[-1] == 0 and d2[-1] == 2.25                              # the single-point pair


def test_grid_nn_selection(grid_reference):
    import eyoc_amd
    g = grid_reference
    rng = np.random.default_rng(5)
    B = len(g["srcs"])
    sels = [rng.permutation(len(p))[:int(rng.integers(1, len(p) + 1))] for p in g["srcs"]]
    sels[3] = sels[3][:0]                                               # an empty selection
    sels[-2] = np.arange(len(g["srcs"][-2]))[::-1].copy()               # every planted query, backwards
    seg_sel = offsets([len(s) for s in sels])
    sel = cuda(np.concatenate(sels).astype(np.int64))
    idx, d2, status = eyoc_amd.posed_nn_grid(g["P0"], g["P1"], g["seg0"], g["seg1"], g["T"], 2.0, sel, seg_sel, return_d2=True)
    assert not status.cpu().numpy().any()
    rows = np.concatenate([g["seg0"][b] + sels[b] for b in range(B)]).astype(np.int64)
    np.testing.assert_array_equal(idx.cpu().numpy(), g["idx"][rows])
    np.testing.assert_array_equal(d2.cpu().numpy(), g["d2"][rows])


def test_grid_nn_status_is_per_pair(grid_reference):
    """A NaN pose, a NaN target, a selection past the end: that pair reports it and returns -1 everywhere; the others keep their bytes."""
    import eyoc_amd
    g = grid_reference
    lo, hi = 5, 12                                                      # a slice of the batch is enough
    s0, s1 = g["seg0"], g["seg1"]
    seg0, seg1 = [v - s0[lo] for v in s0[lo:hi + 1]], [v - s1[lo] for v in s1[lo:hi + 1]]
    P0, P1 = g["P0"][s0[lo]:s0[hi]].clone(), g["P1"][s1[lo]:s1[hi]].clone()
    T = g["T"][lo:hi].clone()
    T[1, 0, 3] = float("nan")
    P1[seg1[3] + 2, 1] = float("nan")
    sels = [np.arange(seg0[b + 1] - seg0[b]) for b in range(hi - lo)]
    sels[5] = np.concatenate([sels[5], [seg0[6] - seg0[5]]])            # one past the segment's end
    idx, _, status = eyoc_amd.posed_nn_grid(P0, P1, seg0, seg1, T, 2.0, cuda(np.concatenate(sels).astype(np.int64)), offsets([len(s) for s in sels]))
    idx, status = idx.cpu().numpy(), status.cpu().numpy()
    np.testing.assert_array_equal(status, [0, 2, 0, 8, 0, 8, 0])        # EYOC_ICP_BAD_INIT = 2, EYOC_ICP_RANGE = 8
    o = 0
    for b in range(hi - lo):
        got = idx[o:o + len(sels[b])]
        o += len(sels[b])
        if status[b]:
            assert (got == -1).all()
        else:
            np.testing.assert_array_equal(got, g["idx"][s0[lo + b]:s0[lo + b + 1]])


# ---------------------------------------------------------------------------------------------------------------------
# 4 - 6. the whole label step
# ---------------------------------------------------------------------------------------------------------------------
E2E_SEED = 11
E2E_SIZES = [(1500, 1300), (800, 2000), (1000, 1000), (2000, 1700), (1250, 900)]


def label_pair(rng, n0, n1):
    """Two clouds around two sensors, distances on both sides of 20 m: C1 = the posed first m points of C0 + noise, then outliers;
    the first m features correspond (planted as in tests/test_gpu_labels.py make_pair); C1 / F1 rows are shuffled."""
    T = rigid(rng, 6.0, 3.0)
    C0 = sphere(rng, n0, 4.0, 60.0)
    m = int(min(n0, n1) * 0.6)
    posed = (C0[:m].astype(np.float64) @ T[:3, :3].T.astype(np.float64) + T[:3, 3]) + rng.normal(0, 0.02, (m, 3))
    C1 = np.concatenate([posed.astype(F32), sphere(rng, n1 - m, 4.0, 60.0)])
    F0, F1 = unit(rng, n0), unit(rng, n1)
    F1[:m] = (F0[:m] + 0.05 * rng.normal(size=(m, 32))).astype(F32)
    F1[:m] /= np.linalg.norm(F1[:m], axis=1, keepdims=True)
    perm = rng.permutation(n1)
    return C0, F0, np.ascontiguousarray(C1[perm]), np.ascontiguousarray(F1[perm]), T


def e2e_batch(seed=E2E_SEED, sizes=E2E_SIZES):
    rng = np.random.default_rng(seed)
    return [label_pair(rng, a, b) for a, b in sizes]


MATCHER = dict(inlier_threshold=0.6, d_thre=0.1, ratio=0.2, nms_radius=0.6, max_points=8000, k1=30, k2=20, num_iterations=20)
GAPS = [3, 17, 8, 26, 0]


def per_pair_chain(pairs, matcher, spatial_filter, gen_seed, table):
    """The composition INTEGRATION.md shows for the per-pair route."""
    import eyoc_amd
    C0, F0, C1, F1 = ([cuda(p[i]) for p in pairs] for i in range(4))
    matches, unc = eyoc_amd.match_and_filter_corr(C0, F0, C1, F1, radius=20, feature_filter="Lowe", spatial_filter=spatial_filter,
                                                  frame_distance=GAPS[:len(pairs)], num_corres=600, dist_sim_map=table, similarity_thresh=0.3)
    src = [C0[i][u[:, 0]] for i, u in enumerate(unc)]
    tgt = [C1[i][u[:, 1]] for i, u in enumerate(unc)]
    poses = matcher.SC2_PCR_batch(src, tgt)
    g = torch.Generator().manual_seed(gen_seed)
    corr = [eyoc_amd.correspondences_under_pose(C0[i], C1[i], T.cpu().numpy(), generator=g) for i, (T, _) in enumerate(poses)]
    return matches, unc, poses, corr


def batched(pairs, matcher, spatial_filter, gen_seed, table, **kw):
    import eyoc_amd
    C0, F0, C1, F1 = ([cuda(p[i]) for p in pairs] for i in range(4))
    return eyoc_amd.label_step(C0, F0, C1, F1, matcher, radius=20, feature_filter="Lowe", spatial_filter=spatial_filter,
                               frame_distance=GAPS[:len(pairs)], num_corres=600, dist_sim_map=table, similarity_thresh=0.3,
                               generator=torch.Generator().manual_seed(gen_seed), **kw)


def assert_same_labels(got, ref, pairs, skip=()):
    pos_pairs, unc_corr, T, fits = got
    _, _, poses, corr = ref
    s0, s1 = offsets([len(p[0]) for p in pairs]), offsets([len(p[2]) for p in pairs])
    assert T.is_cuda and T.shape == (len(pairs), 4, 4) and pos_pairs.is_cuda
    for b in range(len(pairs)):
        if b in skip:
            continue
        np.testing.assert_array_equal(T[b].cpu().numpy(), poses[b][0].cpu().numpy(), err_msg=f"pose {b}")
        np.testing.assert_array_equal(fits[b].cpu().numpy(), poses[b][1].cpu().numpy(), err_msg=f"fitness {b}")
        np.testing.assert_array_equal(unc_corr[b].cpu().numpy(), corr[b].cpu().numpy(), err_msg=f"correspondences {b}")
    col = torch.cat([c + torch.tensor([s0[b], s1[b]], device=c.device) for b, c in enumerate(corr) if b not in skip])
    np.testing.assert_array_equal(pos_pairs.cpu().numpy(), col.cpu().numpy())


@pytest.mark.parametrize("spatial_filter", ["Spherical", "Similarity"])
def test_label_step_equals_the_per_pair_chain(spatial_filter):
    import eyoc_amd
    pairs = e2e_batch()
    table = synthetic_dist_sim_map()
    matcher = eyoc_amd.Matcher(**MATCHER)
    ref = per_pair_chain(pairs, matcher, spatial_filter, 123, table)
    for b, (T, _) in enumerate(ref[2]):                                  # every pair registers in the per-pair route
        rte, rre, ok = eyoc_amd.registration_errors(T.cpu().numpy(), pairs[b][4])
        assert ok and rte < 0.3, (b, rte, rre)
    for c, p in zip(ref[3], pairs):                                      # the gate keeps the planted part and drops most of the rest
        assert 0.5 * min(len(p[0]), len(p[2])) < len(c) < len(p[0])
    # the first stage on its own: device tensors, the values of match_and_filter_corr, views of one buffer
    C0, F0, C1, F1 = ([cuda(p[i]) for p in pairs] for i in range(4))
    m, unc = eyoc_amd.match_and_filter_corr_batched(C0, F0, C1, F1, radius=20, feature_filter="Lowe", spatial_filter=spatial_filter,
                                                    frame_distance=GAPS, num_corres=600, dist_sim_map=table, similarity_thresh=0.3)
    assert m.is_cuda
    np.testing.assert_array_equal(m.cpu().numpy(), ref[0].numpy())
    for a, b in zip(unc, ref[1]):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert 0 < len(b) <= 1200
    assert sum(len(b) for b in ref[1]) < 5 * 1200                        # the spatial filter drops some
    assert len({u.untyped_storage().data_ptr() for u in unc}) == 1
    assert_same_labels(batched(pairs, matcher, spatial_filter, 123, table), ref, pairs)


@pytest.mark.parametrize("feature_filter,spatial_filter", [("None", "Spherical"), ("Lowe", "None")])
def test_match_and_filter_corr_batched_other_branches(feature_filter, spatial_filter):
    import eyoc_amd
    pairs = e2e_batch(sizes=E2E_SIZES[:3])
    C0, F0, C1, F1 = ([cuda(p[i]) for p in pairs] for i in range(4))
    kw = dict(radius=20, feature_filter=feature_filter, spatial_filter=spatial_filter, num_corres=700)
    m, unc = eyoc_amd.match_and_filter_corr_batched(C0, F0, C1, F1, **kw)
    rm, ru = eyoc_amd.match_and_filter_corr(C0, F0, C1, F1, **kw)
    np.testing.assert_array_equal(m.cpu().numpy(), rm.numpy())
    for a, b in zip(unc, ru):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_correspondences_under_pose_batched_fixed_selection():
    import eyoc_amd
    pairs = e2e_batch(sizes=E2E_SIZES[:3])
    rng = np.random.default_rng(3)
    C0, C1 = [cuda(p[0]) for p in pairs], [cuda(p[2]) for p in pairs]
    Ts = [p[4] for p in pairs]
    sels = [rng.permutation(len(p[0]))[:500] for p in pairs]
    unc, col = eyoc_amd.correspondences_under_pose_batched(C0, C1, cuda(np.stack(Ts)), pos_sel=sels)
    s0, s1 = offsets([len(p[0]) for p in pairs]), offsets([len(p[2]) for p in pairs])
    want = []
    for b in range(3):
        ref = eyoc_amd.correspondences_under_pose(C0[b], C1[b], Ts[b], pos_sel=sels[b]).cpu().numpy()
        assert 100 < len(ref) < 500
        np.testing.assert_array_equal(unc[b].cpu().numpy(), ref)
        want.append(ref + np.array([s0[b], s1[b]]))
    np.testing.assert_array_equal(col.cpu().numpy(), np.concatenate(want))
    with pytest.raises(ValueError):
        eyoc_amd.correspondences_under_pose_batched(C0, C1, np.stack(Ts))     # the poses stay on the device


def degenerate_batch():
    """Pair 2 has every point inside the 20 m sphere: the spherical filter leaves it nothing to register."""
    pairs = e2e_batch()
    rng = np.random.default_rng(99)
    C0, F0, C1, F1, T = pairs[2]
    pairs[2] = (sphere(rng, len(C0), 2.0, 15.0), F0, sphere(rng, len(C1), 2.0, 15.0), F1, T)
    return pairs


def test_degenerate_pair_raise_and_skip():
    import eyoc_amd
    from eyoc_amd import _lib
    pairs = degenerate_batch()
    table = synthetic_dist_sim_map()
    matcher = eyoc_amd.Matcher(**MATCHER)
    with pytest.raises(eyoc_amd.EyocError) as per_pair:
        per_pair_chain(pairs, matcher, "Spherical", 5, table)
    assert _lib.knob("eyoc_registration_accept_degenerate", -1) == 0
    with pytest.raises(eyoc_amd.EyocError) as both:
        batched(pairs, matcher, "Spherical", 5, table)
    assert both.value.code == per_pair.value.code and str(both.value) == str(per_pair.value)
    pos_pairs, unc, T, fits = batched(pairs, matcher, "Spherical", 5, table, on_degenerate="skip")
    assert _lib.knob("eyoc_registration_accept_degenerate", -1) == 0       # restored
    assert torch.isnan(T[2]).all() and len(unc[2]) == 0 and not fits[2].any()
    # the live pairs: the bytes of a run without the degenerate one.  The per-pair draws consume the generator in pair order, so the
    # reference run skips pair 2's draw the way the per-pair loop would have made it: same generator, same order, pair 2 included
    live = [p for b, p in enumerate(pairs) if b != 2]
    C0, F0, C1, F1 = ([cuda(p[i]) for p in live] for i in range(4))
    _, unc_live = eyoc_amd.match_and_filter_corr(C0, F0, C1, F1, radius=20, num_corres=600)
    # (num_corres = 600 is below every cloud's size, so k does not depend on which pairs share the batch)
    poses = matcher.SC2_PCR_batch([C0[i][u[:, 0]] for i, u in enumerate(unc_live)], [C1[i][u[:, 1]] for i, u in enumerate(unc_live)])
    g = torch.Generator().manual_seed(5)
    corr = []
    for b, p in enumerate(pairs):
        sel = torch.randperm(len(p[0]), generator=g)[:5000]
        if b != 2:
            j = len(corr)
            corr.append(eyoc_amd.correspondences_under_pose(C0[j], C1[j], poses[j][0].cpu().numpy(), pos_sel=sel))
    s0, s1 = offsets([len(p[0]) for p in pairs]), offsets([len(p[2]) for p in pairs])
    for j, b in enumerate([0, 1, 3, 4]):
        np.testing.assert_array_equal(T[b].cpu().numpy(), poses[j][0].cpu().numpy())
        np.testing.assert_array_equal(fits[b].cpu().numpy(), poses[j][1].cpu().numpy())
        np.testing.assert_array_equal(unc[b].cpu().numpy(), corr[j].cpu().numpy())
        assert len(corr[j]) > 400
    col = torch.cat([c + torch.tensor([s0[b], s1[b]], device=c.device) for c, b in zip(corr, [0, 1, 3, 4])])
    np.testing.assert_array_equal(pos_pairs.cpu().numpy(), col.cpu().numpy())
    # an exception inside the call restores the switch too
    class Boom(eyoc_amd.Matcher):
        def SC2_PCR_packed(self, *a):
            raise RuntimeError("boom")
    with pytest.raises(RuntimeError):
        batched(pairs, Boom(**MATCHER), "Spherical", 5, table, on_degenerate="skip")
    assert _lib.knob("eyoc_registration_accept_degenerate", -1) == 0


def test_label_step_on_a_side_stream():
    """Everything is enqueued on the caller's stream: work that follows on that stream sees the results, no synchronise in between."""
    import eyoc_amd
    pairs = e2e_batch(sizes=E2E_SIZES[:3])
    table = synthetic_dist_sim_map()
    matcher = eyoc_amd.Matcher(**MATCHER)
    ref = batched(pairs, matcher, "Spherical", 9, table)
    ref_np = [ref[0].cpu().numpy(), ref[2].cpu().numpy()] + [u.cpu().numpy() for u in ref[1]]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = batched(pairs, matcher, "Spherical", 9, table)
        copies = [got[0].clone(), got[2].clone()] + [u.clone() for u in got[1]]       # consumers on the same stream
        host = [torch.empty(c.shape, dtype=c.dtype).pin_memory() for c in copies]
        for h, c in zip(host, copies):
            h.copy_(c, non_blocking=True)
        done = torch.cuda.Event()
        done.record(side)
    done.synchronize()
    for h, r in zip(host, ref_np):
        np.testing.assert_array_equal(h.numpy(), r)
