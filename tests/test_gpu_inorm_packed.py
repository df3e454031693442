"""The packed plan of the ResUNetIN2 family (``model.packed_in = True``; csrc/model.hip M_INORM, csrc/inorm.hip on SPLIT16 rows).

Kernel alone: ``eyoc_in_forward_split16`` must give, bit for bit, the SPLIT16 encoding (csrc/spconv.h: per 32 channels 32 fp16 hi halves
``fp16(x)``, then 32 lo halves ``fp16(x - hi)``; a value reads back as ``hi + lo``) of what ``eyoc_in_forward`` gives on the decoded rows - the
two are one set of templates.  The encoding is restated here in numpy (round to nearest even, as the device converts).

Whole network: the bar of tests/test_gpu_inorm_model.py, ``REL = 1e-4`` of the largest entry against the float64 restatement, on that
file's inputs (its CPU-checked condition - the float32 restatement against the float64 one under ``REL / 4`` - is what the bar stands on).
Measured worst ratios (error / largest entry) on the MI355X:
  ResUNetIN2C, three clouds (8418 voxels):  fp32 4.87e-06   split16 2.13e-06   auto (= split16, Z-ordered) 2.13e-06
  1.8 k-voxel input, fp32 / forced split16:  IN2 1.07e-06 / 1.75e-06   IN2B 5.95e-07 / 1.44e-06   IN2D 1.14e-06 / 1.84e-06
                                             IN2E 1.05e-06 / 1.95e-06
(at most 0.05 of the bar).  A block convolution scaled by 2^20 (the range-guard test), fp32 math: 1.03e-06.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import inorm_restatement as IR
import test_gpu_inorm_model as M

pytestmark = pytest.mark.gpu

REL = M.REL
EPS = 1e-8
SENTINEL = -7.25


def _lib():
    from eyoc_amd import _lib as L
    return L, L.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ the SPLIT16 row format, restated
def s16_encode(x):
    """float32 ``[n, c]`` (c % 32 == 0) -> float32-typed ``[n, c]`` holding the SPLIT16 bytes"""
    n, c = x.shape
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    out = np.empty((n, c // 32, 2, 32), np.float16)
    out[:, :, 0] = hi.reshape(n, -1, 32)
    out[:, :, 1] = lo.reshape(n, -1, 32)
    return out.reshape(n, 2 * c).view(np.float32)


def s16_decode(rows):
    n, c = rows.shape
    h = np.ascontiguousarray(rows).view(np.float16).reshape(n, c // 32, 2, 32)
    return (h[:, :, 0].astype(np.float32) + h[:, :, 1].astype(np.float32)).reshape(n, c)


def test_the_format_restated_here_is_the_library_s():
    L, lib = _lib()
    rng = np.random.default_rng(0)
    x = (rng.normal(size=(70, 64)) * 10.0 ** rng.uniform(-6, 4, (70, 64))).astype(np.float32)
    xd = dev(x)
    enc = torch.empty_like(xd)
    L.check(lib.eyoc_split16_encode(L.ctx(), L.ptr(xd), 70, 64, 64, L.ptr(enc), 64, L.stream_ptr()), "eyoc_split16_encode")
    np.testing.assert_array_equal(enc.cpu().numpy().view(np.uint32), s16_encode(x).view(np.uint32))
    np.testing.assert_array_equal(s16_decode(s16_encode(x)), s16_decode(enc.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ 3. the kernel alone
def kernel_input(rng, n, c):
    """columns with mean / std cycling through 0, 1, 30, 300 and a per-column std in [0.1, 10]: everything inside fp16's range"""
    ratio = np.array([0.0, 1.0, 30.0, 300.0])[np.arange(c) % 4]
    std = 10.0 ** rng.uniform(-1.0, 1.0, c)
    x = (std * (ratio + rng.normal(size=(n, c)))).astype(np.float32)
    x[:, c - 3] = np.float32(3.7 * std[c - 3])                       # a constant column: variance 0
    w = rng.uniform(0.5, 1.5, c).astype(np.float32)
    b = rng.normal(size=c).astype(np.float32)
    w[0], b[0] = 1.0, 0.0
    res = rng.normal(size=(n, c)).astype(np.float32)
    return x, w, b, res


def build_plan(ids, n_inst):
    L, lib = _lib()
    n = len(ids)
    coords = np.zeros((n, 4), np.int32)
    coords[:, 0] = ids
    coords[:, 1] = np.arange(n)
    nbytes = lib.eyoc_in_plan_bytes(n, n_inst)
    plan = torch.full((nbytes // 4,), -1, dtype=torch.int32, device="cuda")
    L.check(lib.eyoc_in_plan_build(L.ctx(), L.ptr(dev(coords)), n, n_inst, L.ptr(plan), nbytes, L.stream_ptr()), "eyoc_in_plan_build")
    return plan


def run_fp32(x, plan, n_inst, w, b, relu, res):
    L, lib = _lib()
    n, c = x.shape
    xd, rd, wd, bd = dev(x), None if res is None else dev(res), dev(w), dev(b)
    yd = torch.full((n, c), np.nan, dtype=torch.float32, device="cuda")
    stats = torch.full((n_inst, 2 * c), np.nan, dtype=torch.float32, device="cuda")
    need = lib.eyoc_in_workspace_bytes(n, c, n_inst)
    ws = L.workspace(max(need, 256), torch.device("cuda"))
    L.check(lib.eyoc_in_forward(L.ctx(), L.ptr(xd), n, c, c, L.ptr(plan), n_inst, L.ptr(wd), L.ptr(bd), EPS, int(relu), L.ptr(rd),
                                0 if rd is None else c, L.ptr(yd), c, L.ptr(stats), L.ptr(ws), need, L.stream_ptr()), "eyoc_in_forward")
    return yd.cpu().numpy(), stats.cpu().numpy()


def run_split16(xs, plan, n_inst, w, b, relu, rs, wide):
    """``wide``: x, residual and y each in a buffer of ``c + 32`` floats per row at column 32, the other 32 columns a sentinel that
    must survive; else y IS x (in place), rows of ``c`` floats"""
    L, lib = _lib()
    n, c = xs.shape
    ld, col = (c + 32, 32) if wide else (c, 0)

    def place(a):
        full = torch.full((n, ld), SENTINEL, dtype=torch.float32, device="cuda")
        full[:, col:col + c] = dev(a)
        return full
    xd = place(xs)
    rd = None if rs is None else place(rs)
    yd = torch.full((n, ld), SENTINEL, dtype=torch.float32, device="cuda") if wide else xd
    wd, bd = dev(w), dev(b)
    stats = torch.full((n_inst, 2 * c), np.nan, dtype=torch.float32, device="cuda")
    rng_words = torch.zeros(8, dtype=torch.int32, device="cuda")
    need = lib.eyoc_in_workspace_bytes(n, c, n_inst)
    ws = L.workspace(max(need, 256), torch.device("cuda"))
    off = lambda t: C.c_void_p(t.data_ptr() + 4 * col)
    L.check(lib.eyoc_in_forward_split16(L.ctx(), off(xd), n, c, ld, L.ptr(plan), n_inst, L.ptr(wd), L.ptr(bd), EPS, int(relu),
                                        None if rd is None else off(rd), 0 if rd is None else ld, off(yd), ld, L.ptr(stats), L.ptr(rng_words),
                                        L.ptr(ws), need, L.stream_ptr()), "eyoc_in_forward_split16")
    full = yd.cpu().numpy()
    if wide:
        assert (full[:, :col] == SENTINEL).all() and (xd.cpu().numpy()[:, :col] == SENTINEL).all(), "wrote outside its columns"
    assert not rng_words.cpu().numpy().any(), "the range guard fired on values far inside the range"
    return np.ascontiguousarray(full[:, col:col + c]), stats.cpu().numpy()


@pytest.mark.parametrize("wide", [True, False], ids=["ld=c+32,col=32", "in-place"])
@pytest.mark.parametrize("c", [32, 64, 128, 256])
def test_split16_kernel_is_the_fp32_kernel_between_decode_and_encode(c, wide):
    _, lib = _lib()
    R = int(lib.eyoc_in_chunk_rows())
    for k, sizes in enumerate(([1, R - 1, 0], [R, 0, R + 1])):       # n_inst = 3: 1, R - 1, R, R + 1 rows, an id without rows
        for shuffled in (False, True):                               # identity and non-identity plans
            for relu, with_res in ((False, False), (True, True), (True, False)):
                rng = np.random.default_rng([c, k, int(shuffled), int(relu), int(with_res)])
                ids = np.repeat(np.arange(3), sizes).astype(np.int32)
                if shuffled:
                    ids = ids[rng.permutation(len(ids))]
                x, w, b, res = kernel_input(rng, len(ids), c)
                xs, rs = s16_encode(x), s16_encode(res) if with_res else None
                plan = build_plan(ids, 3)
                y32, stats32 = run_fp32(s16_decode(xs), plan, 3, w, b, relu, None if rs is None else s16_decode(rs))
                got, stats = run_split16(xs, plan, 3, w, b, relu, rs, wide)
                assert np.isfinite(y32).all()
                np.testing.assert_array_equal(got.view(np.uint32), s16_encode(y32).view(np.uint32), err_msg=str((sizes, shuffled, relu, with_res)))
                assert stats.tobytes() == stats32.tobytes()
                assert np.isnan(stats[np.array(sizes) == 0]).all(), "an instance id without rows must touch nothing"


def test_split16_kernel_feeds_the_range_guard():
    """|y| reaches 6e4 (weight 1e5 on a normalised column): words 0 and 3 are raised - the flag of an arithmetic overflow, nothing faults"""
    L, lib = _lib()
    rng = np.random.default_rng(5)
    n, c = 200, 32
    ids = np.zeros(n, np.int32)
    x, w, b, _ = kernel_input(rng, n, c)
    w[4] = 1e5
    plan = build_plan(ids, 1)
    xd, wd, bd = dev(s16_encode(x)), dev(w), dev(b)
    stats = torch.empty((1, 2 * c), dtype=torch.float32, device="cuda")
    words = torch.zeros(8, dtype=torch.int32, device="cuda")
    need = lib.eyoc_in_workspace_bytes(n, c, 1)
    ws = L.workspace(max(need, 256), torch.device("cuda"))
    L.check(lib.eyoc_in_forward_split16(L.ctx(), L.ptr(xd), n, c, c, L.ptr(plan), 1, L.ptr(wd), L.ptr(bd), EPS, 0, None, 0, L.ptr(xd), c,
                                        L.ptr(stats), L.ptr(words), L.ptr(ws), need, L.stream_ptr()), "eyoc_in_forward_split16")
    assert words.cpu().numpy()[[0, 3]].tolist() == [1, 1]
    # refusals: channels and leading dimensions in whole 32-channel blocks
    assert lib.eyoc_in_forward_split16(L.ctx(), L.ptr(xd), n, 16, c, L.ptr(plan), 1, L.ptr(wd), L.ptr(bd), EPS, 0, None, 0, L.ptr(xd), c,
                                       L.ptr(stats), None, L.ptr(ws), need, L.stream_ptr()) == L.ERR_INVALID
    assert lib.eyoc_in_forward_split16(L.ctx(), L.ptr(xd), n, c, c + 4, L.ptr(plan), 1, L.ptr(wd), L.ptr(bd), EPS, 0, None, 0, L.ptr(xd), c,
                                       L.ptr(stats), None, L.ptr(ws), need, L.stream_ptr()) == L.ERR_INVALID


# ------------------------------------------------------------------------------------------------ 4. .. 6. the whole network
def packed_model(name, sd):
    model = M.build_model(name, sd).eval()
    model.packed_in = True
    return model


@pytest.fixture(scope="module")
def big():
    """ResUNetIN2C on the three-cloud input (8418 voxels) and its float64 eval restatement, computed once"""
    sd, coords, feats, target = M.make_inputs()
    assert len(coords) >= 8192
    ref, _, _, _ = M.restatement(sd, coords, feats, target, torch.float64, None, False, False)
    return packed_model("ResUNetIN2C", sd), sd, coords, feats, ref


def test_in2c_meets_the_bar_in_every_math(big):
    model, sd, coords, feats, ref = big
    L, lib = _lib()
    x = M.sparse(coords, feats)
    errs = {}
    with torch.no_grad():
        for math, ran in (("fp32", "fp32"), ("split16", "split16"), ("auto", "split16")):
            model.spconv_math = math
            got = model(x).F
            assert model.last_spconv_math == ran, math
            model.check_range()
            errs[math] = M.rel_err(got.cpu().numpy(), ref)
    assert x.coordinate_manager.row_order() is not None, "8418 voxels: the forward's own maps are Z-ordered"
    n_bn = 23
    assert lib.eyoc_model_num_layers(model._handle) == n_bn + 14
    print("ResUNetIN2C packed, error / largest entry: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < REL, errs
    # under enable_grad with parameters that require grad the layer-by-layer route stays (the only one with a backward)
    model.spconv_math = "auto"
    with_grad = model(x).F
    assert with_grad.requires_grad and M.rel_err(with_grad.detach().cpu().numpy(), ref) < REL
    # layer timing and the work table cover the new layers
    model.set_timing(True)
    with torch.no_grad():
        model(x)
    ms = model.layer_ms()
    work = model.layer_work(x)
    model.set_timing(False)
    assert len(ms) == len(work) == n_bn + 14 and all(t >= 0 for t in ms)
    norms = [w for w in work if ".norm" in w["name"] and w["name"].startswith("block")]
    assert len(norms) == 14 and all(w["pairs"] == 0 and w["compulsory_bytes"] > 0 for w in norms)
    assert work[1]["name"] == "block1.conv1" and work[2]["name"] == "block1.norm1" and ms[2] > 0


@pytest.mark.parametrize("name", ["ResUNetIN2", "ResUNetIN2B", "ResUNetIN2D", "ResUNetIN2E"])
def test_other_tables_meet_the_bar(name):
    sd, coords, feats, target = M.make_inputs(name)
    assert 1000 <= len(coords) <= 2500
    ref, _, _, _ = M.restatement(sd, coords, feats, target, torch.float64, None, False, False)
    model = packed_model(name, sd)
    x = M.sparse(coords, feats)
    errs = {}
    with torch.no_grad():
        for math in ("fp32", "split16"):
            model.spconv_math = math
            got = model(x).F
            assert model.last_spconv_math == math
            model.check_range()
            errs[math] = M.rel_err(got.cpu().numpy(), ref)
    print(f"{name} packed on {len(coords)} voxels, error / largest entry: fp32 {errs['fp32']:.2e}  split16 {errs['split16']:.2e}")
    assert max(errs.values()) < REL, errs


@pytest.mark.parametrize("math", ["fp32", "auto"])
def test_instances_do_not_leak_and_row_order_does_not_matter(big, math):
    model, sd, coords, feats, ref = big
    model.spconv_math = math
    third = coords[:, 0] == 2
    assert 0 < third.sum() < 100
    with torch.no_grad():
        base = model(M.sparse(coords, feats)).F.cpu().numpy()
        other = feats.copy()
        other[third] *= np.float32(3.0)
        got = model(M.sparse(coords, other)).F.cpu().numpy()
        assert base[~third].tobytes() == got[~third].tobytes(), "clouds 0 and 1 changed with the third cloud's features"
        assert (base[third] != got[third]).any()
        perm = np.random.default_rng(6).permutation(len(coords))
        shuffled = model(M.sparse(coords[perm], feats[perm])).F.cpu().numpy()
        e = M.rel_err(shuffled, base[perm])
        # maps that keep the caller's (shuffled) order: the instance plans are no identities (fp32 only - split16 wants its Z-order)
        if math == "fp32":
            xs = M.sparse(coords[perm], feats[perm])
            xs.coordinate_manager.maps(0)
            assert xs.coordinate_manager.row_order() is None
            e = max(e, M.rel_err(model(xs).F.cpu().numpy(), base[perm]))
    model.spconv_math = "auto"
    print(f"{math}: shuffled rows against the shuffled output {e:.2e}")
    assert e < 1e-5


@pytest.mark.parametrize("math", ["fp32", "auto"])
def test_sampled_rows_are_the_full_output_s_rows(big, math):
    model, sd, coords, feats, ref = big
    model.spconv_math = math
    x = M.sparse(coords, feats)
    rng = np.random.default_rng(4)
    r = torch.from_numpy(np.concatenate([rng.permutation(len(coords))[:700], [5, 5, 0, len(coords) - 1, 5]]))
    with torch.no_grad():
        full = model(x).F
        sampled = model(x, rows=r)
        empty = model(x, rows=torch.zeros(0, dtype=torch.int64))
    model.spconv_math = "auto"
    assert sampled.shape == (len(r), 32) and torch.equal(sampled, full[r.cuda()])
    assert empty.shape == (0, 32)


# ------------------------------------------------------------------------------------------------ 7. re-pack
def test_repack_device_gives_pack_host_s_bytes_after_in_place_edits(big):
    _, sd, coords, feats, ref = big
    model = packed_model("ResUNetIN2C", sd)
    model.pack()
    v0 = model._packed_version
    with torch.no_grad():
        model.block3.conv2.kernel.mul_(1.25)
        model.block2_tr.norm1.weight.add_(0.125)
        model.block4.norm2.bias.sub_(0.5)
        model.norm3.bn.weight.mul_(0.75)
        model.norm2_tr.bn.running_var.add_(0.25)
    assert model._weights_version() != v0, "an in-place edit of an instance norm's weight must trigger the re-pack"
    blob = model.repack_device()
    torch.cuda.synchronize()
    assert blob.cpu().numpy().tobytes() == model.pack_host().numpy().tobytes()
    # the forward's own re-pack after an edit (device_repack): the features of a freshly packed copy
    model.device_repack = True
    with torch.no_grad():
        model.block1.norm2.weight.mul_(1.5)
        x = M.sparse(coords, feats)
        got = model(x).F
        fresh = packed_model("ResUNetIN2C", {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
        assert torch.equal(got, fresh(x).F)
        # the receiving side of a weight broadcast adopts the blob
        adopted = packed_model("ResUNetIN2C", sd)
        adopted.pack(blob=model.weight_blob.clone(), from_blob=True)
        assert torch.equal(adopted(x).F, got)


def test_ema_sync_repacks_an_opted_in_labeler(big):
    from eyoc_amd.train import ema_sync
    _, sd, coords, feats, ref = big
    labeler = packed_model("ResUNetIN2C", sd)
    sd2 = {k: (np.asarray(v) * np.float32(1.125) if np.asarray(v).dtype == np.float32 else v) for k, v in sd.items()}
    model = M.build_model("ResUNetIN2C", sd2)
    x = M.sparse(coords, feats)
    with torch.no_grad():
        labeler(x)                                                   # packed: the sync below re-packs on the device
        assert labeler._handle is not None
        blob = ema_sync(labeler, model, 0.9, 1 - 0.9 ** 3)
        assert blob is not None and blob.data_ptr() == labeler.weight_blob.data_ptr()
        got = labeler(x).F
        fresh = packed_model("ResUNetIN2C", {k: v.detach().cpu().numpy() for k, v in labeler.state_dict().items()})
        assert torch.equal(got, fresh(x).F)
    # a labeler that did not opt in: as before
    plain = M.build_model("ResUNetIN2C", sd)
    assert ema_sync(plain, model, 0.9, 1 - 0.9 ** 3) is None


# ------------------------------------------------------------------------------------------------ 8. range guard
def test_a_block_convolution_beyond_fp16_raises_the_range_error():
    L, lib = _lib()
    name = "ResUNetIN2"
    sd, coords, feats, target = M.make_inputs(name)
    sd = dict(sd)
    sd["block1.conv1.kernel"] = np.asarray(sd["block1.conv1.kernel"]) * np.float32(2.0 ** 20)      # raw sums of ~1e6; the norm behind it undoes the scale
    ref, _, _, _ = M.restatement(sd, coords, feats, target, torch.float64, None, False, False)
    model = packed_model(name, sd)
    x = M.sparse(coords, feats)
    with torch.no_grad():
        model.spconv_math = "split16"
        with pytest.raises(L.EyocError) as e:
            model(x)
        assert e.value.code == L.ERR_RANGE
        model.range_check = False
        out = model(x).F
        assert bool(torch.isnan(out).all()), "an overflowed split16 forward must not return finite-looking rows"
        with pytest.raises(L.EyocError):
            model.check_range()
        model.range_check = True
        model.spconv_math = "fp32"
        got = model(x).F
        err = M.rel_err(got.cpu().numpy(), ref)
        # automatic mode on a forced-split16-capable input falls back by itself where it picks split16; here (1.5 k voxels) it picks fp32
        model.spconv_math = "auto"
        assert torch.equal(model(x).F, got) and model.last_spconv_math == "fp32"
    print(f"{name} with block1.conv1 x 2^20, fp32 math: {err:.2e}")
    assert err < REL


# ------------------------------------------------------------------------------------------------ 9. the pipeline
def test_registration_pipeline_takes_an_opted_in_model():
    from eyoc_amd import SparseTensor
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    from eyoc_amd.metrics import registration_errors
    pairs = [syn.make_pair(s, beams=32, azimuths=1000, band=None) for s in (3, 4)]
    sd = IR.in_state_dict(syn.make_weights())
    model = packed_model("ResUNetIN2C", sd)
    d = torch.device("cuda")
    batch = DeviceBatch(pairs, [3, 4], d, n_points=2000, descriptor=dict(inlier_ratio=0.3))
    pipe = RegistrationPipeline(model, RegistrationConfig(ransac_max_iteration=100000, n_points=2000, use_RANSAC=True))
    results = pipe.register(batch, seed=7)
    assert model._handle is not None, "the pipeline must run the packed plan"
    assert len(results) == 2
    for r, p in zip(results, pairs):
        rte, rre, ok = registration_errors(np.asarray(r.transformation, np.float32), np.asarray(p["T_gt"], np.float32), 2.0, 5.0)
        assert ok and r.status == 0, (rte, rre, r.status)
    records = pipe.register(batch, seed=7, return_device=True).cpu()
    model.check_range()
    for tail in (False, True):
        host, overflow = pipe.enqueue(batch, seed=7, slot=int(tail), tail_stream=tail).wait()
        assert not overflow
        np.testing.assert_array_equal(host.numpy().view(np.uint8), records.numpy().view(np.uint8))
    # the features the pipeline used: model(x).F on the same batch
    with torch.no_grad():
        full = model(SparseTensor(batch.feats, coordinates=batch.coords)).F
    assert torch.equal(pipe.features(batch).F, full)
    used, _ = pipe._features(batch, None, sampled=True)
    rows = torch.cat((batch.sel0.reshape(-1), batch.sel1.reshape(-1)))
    assert torch.equal(used, full[rows])
    # validate() runs on the same features
    v = pipe.validate(batch)
    assert v is not None
