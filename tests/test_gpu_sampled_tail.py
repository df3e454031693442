"""``model(x, rows=r)`` / ``eyoc_model_forward_rows``: the last 3x3x3 layer (``block2_tr.conv2``) and the 1x1 tail computed for a LIST of
rows (``csrc/spconv_rows.hip``), bit for bit the rows of the full forward - the registration step reads 5000 rows per cloud, which the
reference draws by index only (``scripts/test_kitti.py:141-160``).

Fixture: three clouds in one batch, just above the 8192 rows from which the forward runs split16 arithmetic on Z-ordered rows.  Batch
index 0 is a dense 20 x 20 x 20 block: its 256-row tiles reference more than 639 distinct neighbour rows, so their records stage in TWO
passes and a row's products are summed pass by pass - the order the rows kernel has to reproduce; the two lidar-like clouds behind it
give one-pass tiles, a ragged last tile and chunks that mix both kinds."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REL = 1e-4            # the project's gate of a forward against the oracle
REC = 33408           # bytes of a tile record; its first word is n_u, the tile's distinct input rows (two passes above 639)


def _lib():
    from eyoc_amd import _lib as L
    return L, L.load()


def make_model(sd, math="split16"):
    import eyoc_amd
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    m.spconv_math = math
    return m


def sparse(cloud):
    import eyoc_amd
    return eyoc_amd.SparseTensor(torch.from_numpy(cloud["feats"]).cuda(), coordinates=torch.from_numpy(cloud["coords"]).cuda())


@pytest.fixture(scope="module")
def cloud():
    from eyoc_amd import synthetic as syn
    from oracle import coords as oc
    from oracle import resunet as orr
    from forward_matrix import large_batch
    L, lib = _lib()
    coords, feats, sizes = large_batch()                         # (shared with tests/test_gpu_forward_steps.py)
    n = len(coords)
    sd = syn.make_weights()
    maps = oc.build_maps(coords, 5)
    want, inter, _ = orr.resunet_forward(sd, coords, feats, maps=maps, return_intermediate=True)
    c = dict(coords=coords, feats=feats, sd=sd, maps=maps, want=want.numpy(), base={k: v.numpy() for k, v in inter["stored"].items()})
    assert n >= 8192 and n % 256 != 0
    # one input tensor (one set of maps) and the full forward for every test that compares with it
    c["model"] = make_model(sd)
    c["x"] = sparse(c)
    c["full"] = c["model"](c["x"]).F.cpu().numpy()
    assert c["model"].last_spconv_math == "split16"
    perm = c["x"].coordinate_manager.row_order()
    assert perm is not None, "the batch must run on Z-ordered rows"
    perm = perm.cpu().numpy().astype(np.int64)              # internal row -> caller's row
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    # the tile records of the level-0 stride-1 table in the forward's row order (the builder the map build runs): n_u per 256-row tile
    s1 = maps["s1"][0][:, perm]
    s1 = np.where(s1 >= 0, inv[np.maximum(s1, 0)], -1).astype(np.int32)
    nd = torch.from_numpy(np.ascontiguousarray(s1)).cuda()
    local = torch.zeros(int(lib.eyoc_spconv_local_rulebook_bytes(n)), dtype=torch.uint8, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.eyoc_spconv_build_local_rulebook(L.ctx(), L.ptr(nd), 27, n, L.ptr(local), L.ptr(ovf), L.stream_ptr()))
    n_tiles = (n + 255) // 256
    n_u = local.cpu().numpy()[:n_tiles * REC].reshape(-1, REC)[:, :4].copy().view(np.int32)[:, 0]
    assert int(ovf.item()) == 0 and n_u.min() >= 1 and n_u.max() <= 1278
    assert (n_u > 639).any() and (n_u <= 639).any(), "the fixture needs two-pass and one-pass tiles: move the dense block"
    c.update(perm=perm, inv=inv, n_u=n_u)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    rng = np.random.default_rng(17)
    lists = {f"n{k}": rng.permutation(n)[:k] for k in (1, 15, 16, 17, 5000)}
    t2 = int(np.flatnonzero(n_u > 639)[0])
    lists["n1"] = perm[t2 * 256 + 7:t2 * 256 + 8].copy()      # a single row, of a two-pass tile
    lists["dup"] = rng.integers(0, n, 300)
    lists["dup"][100:200] = lists["dup"][:100]
    lists["edges"] = np.concatenate([starts[:-1], starts[1:] - 1, perm[(n // 256) * 256:], perm[:3], lists["n1"]])
    lists["empty"] = np.zeros(0, np.int64)
    c["lists"] = {k: np.asarray(v, np.int64) for k, v in lists.items()}
    return c


def passes_of(cloud, rows):
    """-> (a listed row lies in a two-pass tile, one lies in a one-pass tile), from the built records"""
    nu = cloud["n_u"][cloud["inv"][rows] >> 8]
    return bool((nu > 639).any()), bool((nu <= 639).any())


def rows_forward(model, cloud, rows, x=None):
    return model(cloud["x"] if x is None else x, rows=torch.from_numpy(rows).cuda()).cpu().numpy()


@pytest.mark.parametrize("mode", ["sampled", "fallback", "fp32"])
@pytest.mark.parametrize("name", ["n1", "n15", "n16", "n17", "n5000", "dup", "edges", "empty"])
def test_listed_rows_equal_the_full_forward_bit_for_bit(cloud, name, mode):
    """``model(x, rows=r) == model(x).F[r]`` exactly: 1, 15, 16, 17 (one chunk, one row more or less) and 5000 rows in no order, a
    list with duplicates, the first and last row of every cloud with the rows of the ragged last tile, no row at all; with the rows
    kernel, with the knob at 0 (the full forward + a row gather) and in fp32 arithmetic (the same fallback)."""
    L, lib = _lib()
    rows = cloud["lists"][name]
    if name in ("n5000", "dup", "edges"):
        two, one = passes_of(cloud, rows)
        assert two and one, "the list must touch two-pass and one-pass tiles"
    if name == "n1":
        assert passes_of(cloud, rows) == (True, False)
    prev = L.knob("eyoc_model_sampled_tail", 0 if mode == "fallback" else 1)
    try:
        if mode == "fp32":
            if "fp32" not in cloud:                               # the fp32 reference, once
                m32 = make_model(cloud["sd"], "fp32")
                cloud["fp32"] = (m32, m32(cloud["x"]).F.cpu().numpy())
            m, full = cloud["fp32"]
            got = rows_forward(m, cloud, rows)
            assert m.last_spconv_math == "fp32"
        else:
            m, full = cloud["model"], cloud["full"]
            got = rows_forward(m, cloud, rows)
    finally:
        L.knob("eyoc_model_sampled_tail", prev)
    assert got.shape == (len(rows), 32) and got.dtype == np.float32
    np.testing.assert_array_equal(got, full[rows])
    assert np.isfinite(got).all()


@pytest.mark.parametrize("knob,value", [("eyoc_spconv_select_st_kernel", 0), ("eyoc_spconv_select_st_kernel", 1), ("eyoc_spconv_select_st_kernel", 2),
                                        ("eyoc_spconv_st_group_rows", 0), ("eyoc_spconv_st_group_rows", 1)])
def test_kernel_switches_leave_the_bits_alone(cloud, knob, value):
    """The C++ loop, the assembly loops with and without their empty-block branches, grouped and ungrouped tile records (another
    order of a tile's rows, hence other chunks): the full forward under each switch gives, at the 5000 listed rows, the bits of the
    rows kernel - which reads the records the switch built.

    The split of a tile's input blocks over several workgroups is off for the comparison: on an input this small the default
    assembly kernel splits the >= 128-channel layers of the coarse levels and adds the shares in share order, which the other
    variants do not do - other bits far upstream of the layer under test, on small inputs only (the bench batch never splits)."""
    L, lib = _lib()
    rows = cloud["lists"]["n5000"]
    prev_ks = L.knob("eyoc_spconv_st_ksplit", 0)
    try:
        want = rows_forward(cloud["model"], cloud, rows)
        prev = L.knob(knob, value)
        try:
            x = sparse(cloud)                                     # maps built under the switch
            full = cloud["model"](x).F.cpu().numpy()
            got = rows_forward(cloud["model"], cloud, rows, x)
        finally:
            L.knob(knob, prev)
    finally:
        L.knob("eyoc_spconv_st_ksplit", prev_ks)
    np.testing.assert_array_equal(full[rows], want)
    np.testing.assert_array_equal(got, want)


def test_listed_rows_meet_the_oracle_gate(cloud):
    """<= 1e-4 max |feature| against ``oracle.resunet.resunet_forward`` - the project's gate of a forward; it guards against both
    paths being wrong together."""
    rows = cloud["lists"]["n5000"]
    got = rows_forward(cloud["model"], cloud, rows)
    err = float(np.abs(got - cloud["want"][rows]).max() / np.abs(cloud["want"]).max())
    print(f"sampled tail vs oracle: {err:.2e}")
    assert err <= REL


def test_range_guard_sees_an_overflow_in_a_listed_row(cloud):
    """``block2_tr.norm2`` is scaled so that the layer's stored output passes 6e4 in some rows (the 1x1 tail is divided by the same
    factor; everything else stays O(10)).  A list that holds such a row: the forward's own flag (word 0) and the sticky word are
    raised and every returned row is NaN, as on the full path; in automatic mode ``model(x, rows=)`` re-runs in fp32 and meets the
    oracle.  An overflow confined to rows of that layer that nobody listed is NOT seen any more: those values are no longer computed
    (the full forward would have answered NaN everywhere)."""
    from oracle import resunet as orr
    L, lib = _lib()
    sd = copy.deepcopy(cloud["sd"])
    s = 1.5e5 / float(cloud["base"]["block2_tr.conv2"].max())
    sd["block2_tr.norm2.bn.weight"] = sd["block2_tr.norm2.bn.weight"] * np.float32(s)
    sd["block2_tr.norm2.bn.bias"] = sd["block2_tr.norm2.bn.bias"] * np.float32(s)
    k = sd["conv1_tr.kernel"].copy()
    k[:64] /= np.float32(s)
    sd["conv1_tr.kernel"] = k
    want, inter, _ = orr.resunet_forward(sd, cloud["coords"], cloud["feats"], maps=cloud["maps"], return_intermediate=True)
    want = want.numpy()
    peak = inter["stored"]["block2_tr.conv2"].abs().max(1).values.numpy()
    others = max(float(v.abs().max()) for k_, v in inter["stored"].items() if k_ != "block2_tr.conv2")
    over = np.flatnonzero(peak > 7e4)
    assert len(over) > 0 and others < 6e3
    rows = np.concatenate([cloud["lists"]["n17"], over[:1]]).astype(np.int64)
    m = make_model(sd, "split16")
    m.range_check = False
    got = rows_forward(m, cloud, rows)
    words = torch.zeros(4, dtype=torch.int32).pin_memory()
    m.range_snapshot(words)
    torch.cuda.synchronize()
    assert int(words[0]) != 0 and int(words[3]) != 0
    assert np.isnan(got).all()
    with pytest.raises(L.EyocError) as ei:
        m.check_range()
    assert ei.value.code == L.ERR_RANGE
    a = make_model(sd, "auto")
    got = rows_forward(a, cloud, rows)
    assert a.last_spconv_math == "fp32" and a.spconv_math == "auto"
    err = float(np.abs(got - want[rows]).max() / np.abs(want).max())
    print(f"range guard, sampled tail: fp32 re-run vs oracle {err:.2e}")
    assert err <= REL


def test_layer_work_reports_what_a_sampled_forward_multiplied(cloud):
    """After ``model(x, rows=r)`` the entry of the last 3x3x3 layer holds the (row, offset) pairs of the listed rows - the non-negative
    entries of the oracle's stride-1 table at those rows - and the 1x1 layers hold ``len(r)`` rows; after a plain forward every entry
    is the geometry's again."""
    m, rows = cloud["model"], cloud["lists"]["n5000"]
    s1 = cloud["maps"]["s1"][0]
    m(cloud["x"])
    plain = m.layer_work(cloud["x"])
    names = [w["name"] for w in plain]
    li = names.index("block2_tr.conv2")
    assert names[li + 1:] == ["conv1_tr", "final"]
    assert plain[li]["pairs"] == int((s1 >= 0).sum()) and plain[li + 1]["pairs"] == plain[li + 2]["pairs"] == s1.shape[1]
    rows_forward(m, cloud, rows)
    work = m.layer_work(cloud["x"])
    assert work[li]["pairs"] == int((s1[:, rows] >= 0).sum())
    assert work[li + 1]["pairs"] == work[li + 2]["pairs"] == len(rows)
    assert work[li]["flop"] == 2.0 * work[li]["pairs"] * 64 * 64
    assert work[:li] == plain[:li]
    m(cloud["x"])
    assert m.layer_work(cloud["x"]) == plain


@pytest.fixture(scope="module")
def four_pairs():
    from eyoc_amd import synthetic as syn
    return [syn.make_pair(40 + s, beams=32, azimuths=1000, band=None) for s in range(4)]


@pytest.mark.parametrize("use_ransac", [True, False])
def test_pipeline_records_do_not_depend_on_the_knob(cloud, four_pairs, use_ransac):
    """Four pairs with planted descriptors through ``RegistrationPipeline``: the records (one ``eyoc_ransac_result`` per pair on the RANSAC path, the
    poses on the SC2-PCR path) and the feature correspondences are byte-identical with the sampled tail and with the full forward +
    row gather - through ``register`` and through ``enqueue(tail_stream=True)`` with two steps in flight."""
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    L, lib = _lib()
    dev = torch.device("cuda")
    sc2 = dict(RegistrationConfig().sc2pcr, num_node=2000, max_points=2000)
    cfg = RegistrationConfig(ransac_max_iteration=50000, n_points=2000, use_RANSAC=use_ransac, sc2pcr=sc2)
    batch = DeviceBatch(four_pairs, [40, 41, 42, 43], dev, n_points=cfg.n_points, descriptor=dict(inlier_ratio=0.3))
    out = {}
    prev = L.knob("eyoc_model_sampled_tail", -1)
    try:
        for knob in (1, 0):
            L.knob("eyoc_model_sampled_tail", knob)
            pipe = RegistrationPipeline(make_model(cloud["sd"], "auto"), cfg)
            rec = pipe.register(batch, seed=3, return_device=True).cpu().numpy().copy()
            nn = None if pipe.last_nn_idx is None else pipe.last_nn_idx.cpu().numpy().copy()
            pend = [pipe.enqueue(batch, seed=3 + k, slot=k, tail_stream=True) for k in range(2)]
            hosts = [p.wait() for p in pend]
            assert not any(o for _, o in hosts)
            out[knob] = (rec, nn, [h.numpy().copy() for h, _ in hosts])
            pipe.model.check_range()
    finally:
        L.knob("eyoc_model_sampled_tail", prev)
    (r1, n1, h1), (r0, n0, h0) = out[1], out[0]
    assert r1.tobytes() == r0.tobytes() and np.isfinite(r1.view(np.float32)[:, :16] if use_ransac else r1).all()
    if use_ransac:
        import ctypes
        assert r1.shape == (4, ctypes.sizeof(L.RansacResult))       # one ``eyoc_ransac_result`` record per pair
        np.testing.assert_array_equal(n1, n0)
    assert h1[0].tobytes() == h0[0].tobytes() and h1[1].tobytes() == h0[1].tobytes()
