"""Building blocks of per-pair failure isolation: the map build's per-batch fault masks (all three build paths), the batched RANSAC /
SC2-PCR back-ends with degenerate pairs, and ``fp32_retry_per_step`` - the split16 overflow of one step re-run in fp32 for that step only.

Degenerate inputs must not reach a back-end that does not know them: every such test first checks on the host that the entry
point or knob exists, before anything is launched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    from eyoc_amd import _lib as L
    lib = L.load()
    for name in ("eyoc_maps_last_fault_batches", "eyoc_registration_accept_degenerate"):
        assert hasattr(lib, name), f"{name} is missing: no launch on degenerate input"
    return L, lib


# ---- map build: which batch indices failed it

def _cloud_batches(batches, rows=3000, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for b in batches:
        xyz = np.unique(rng.integers(-60, 60, size=(rows, 3)), axis=0).astype(np.int32)
        out.append(np.concatenate([np.full((len(xyz), 1), b, np.int32), xyz], 1))
    return out


PATHS = {"caller_order": (0, 1), "zorder_fused": (1, 1), "zorder_levels": (1, 0)}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_map_build_reports_the_faulty_batch_indices(path):
    L, lib = _lib()
    import eyoc_amd
    order, fused = PATHS[path]
    parts = _cloud_batches([0, 3, 5, 700, 701])
    dup = np.concatenate(parts + [parts[1][10:11], parts[3][20:21]])     # duplicates in batches 3 and 700, far from their twins
    far = np.concatenate(parts)
    far[len(parts[0]) + len(parts[1]) + 7, 2] = 1 << 17                   # a row of batch 5 outside the key range
    prev_order = L.knob("eyoc_maps_internal_order", order) - 2
    prev_fused = L.knob("eyoc_maps_fused_levels", fused)
    try:
        with pytest.raises(eyoc_amd.EyocError) as ei:
            eyoc_amd.CoordinateManager(torch.from_numpy(dup).cuda()).maps()
        assert ei.value.code == L.ERR_DUPLICATE
        assert "eyoc_maps_build: 2 duplicate coordinate rows (a sparse tensor needs unique coordinates)" in str(ei.value)
        assert L.fault_batches() == ([3, 700], [])
        with pytest.raises(eyoc_amd.EyocError) as ei:
            eyoc_amd.CoordinateManager(torch.from_numpy(far).cuda()).maps()
        assert ei.value.code == L.ERR_RANGE
        assert "eyoc_maps_build: 1 coordinate rows outside the supported key range" in str(ei.value)
        assert L.fault_batches() == ([], [5])
        both = np.concatenate([far, parts[1][10:11]])                     # batch 3 duplicated, batch 5 out of range: the range error wins
        with pytest.raises(eyoc_amd.EyocError) as ei:
            eyoc_amd.CoordinateManager(torch.from_numpy(both).cuda()).maps()
        assert ei.value.code == L.ERR_RANGE and L.fault_batches() == ([], [5])
        eyoc_amd.CoordinateManager(torch.from_numpy(np.concatenate(parts)).cuda()).maps()    # the clean batch builds ...
        assert L.fault_batches() == ([], [])                                                # ... and clears the masks
    finally:
        L.knob("eyoc_maps_internal_order", prev_order)
        L.knob("eyoc_maps_fused_levels", prev_fused)


# ---- degenerate pairs in the batched back-ends

def _pairs(sizes, seed=0):
    """Packed correspondences of pairs with ``sizes`` rows: a rigid motion, 60 % inliers."""
    src, tgt = [], []
    for k, n in enumerate(sizes):
        rng = np.random.default_rng(100 * seed + k)          # a pair's rows do not depend on the other pairs
        a = rng.uniform(-20, 20, size=(n, 3)).astype(np.float32)
        ang = 0.1 + 0.05 * k
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], np.float32)
        b = a @ R.T + np.float32(0.5 * k)
        out = rng.random(n) < 0.4
        b[out] = rng.uniform(-20, 20, size=(int(out.sum()), 3))
        src.append(a)
        tgt.append(b.astype(np.float32))
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(src), np.concatenate(tgt), seg


SIZES = [600, 0, 500, 3, 700, 7, 650]


def layout(name, minimum):
    """``small``: SIZES.  ``wide``: 110 pairs - 66 degenerate ones first (more than one 64-entry batch of failed records), a run of 35
    normal pairs (across the RANSAC count bound's 32-pair threshold and two SC2-PCR 16-pair chunks), 3 degenerate, 6 normal."""
    if name == "small":
        return list(SIZES)
    return [k % minimum for k in range(66)] + [400 + 50 * (k % 5) for k in range(35)] + [0, minimum - 1, 1] + [450] * 6


def normal(sizes, minimum):
    """``sizes`` with the pairs below a back-end's minimum replaced by normal ones."""
    return [n if n >= minimum else 420 + 10 * (k % 50) for k, n in enumerate(sizes)]


def _ransac(L, sizes):
    from eyoc_amd import registration as reg
    src, tgt, seg = _pairs(sizes)
    corr = torch.from_numpy(np.concatenate([np.arange(n) for n in sizes]).astype(np.int64))
    res = reg.ransac_batched_from_correspondences(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), corr.cuda(), seg, seg,
                                                  0.3, 20000, seed=11)
    return res.cpu().numpy()


def _sc2(sizes):
    from eyoc_amd import registration as reg
    src, tgt, seg = _pairs(sizes, seed=1)
    m = reg.Matcher(inlier_threshold=0.6, num_node=8000, use_mutual=False, d_thre=0.1, num_iterations=20, ratio=0.2,
                    nms_radius=0.6, max_points=8000, k1=30, k2=20)
    T, fit, _ = m.SC2_PCR_packed(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), seg)
    return T.cpu().numpy(), fit.cpu().numpy()


@pytest.mark.parametrize("name", ["small", "wide"])
def test_ransac_gives_degenerate_pairs_a_failed_record(name):
    L, lib = _lib()
    sizes = layout(name, 4)
    prev = L.knob("eyoc_registration_accept_degenerate", 1)
    try:
        got = _ransac(L, sizes)
        want = _ransac(L, normal(sizes, 4))
    finally:
        L.knob("eyoc_registration_accept_degenerate", prev)
    for b, n in enumerate(sizes):
        r = L.RansacResult.from_buffer_copy(got[b].tobytes())
        if n < 4:
            assert np.isnan(np.array(r.T)).all() and r.best_hypothesis == -1 and r.survivors == 0 and r.inliers == 0, b
        else:
            np.testing.assert_array_equal(got[b], want[b], err_msg=f"pair {b}")
            assert r.survivors > 0 and np.isfinite(np.array(r.T)).all()


@pytest.mark.parametrize("name", ["small", "wide"])
def test_sc2pcr_gives_degenerate_pairs_a_failed_output(name):
    L, lib = _lib()
    sizes = layout(name, 8)
    prev = L.knob("eyoc_registration_accept_degenerate", 1)
    try:
        T, fit = _sc2(sizes)
        T_ref, fit_ref = _sc2(normal(sizes, 8))
    finally:
        L.knob("eyoc_registration_accept_degenerate", prev)
    assert sum(n < 8 for n in sizes) > 64 or name == "small"
    for b, n in enumerate(sizes):
        if n < 8:
            assert np.isnan(T[b]).all() and (fit[b] == 0).all(), b
        else:
            np.testing.assert_array_equal(T[b].view(np.uint32), T_ref[b].view(np.uint32), err_msg=f"pair {b}")
            k = int(0.2 * n)
            np.testing.assert_array_equal(fit[b, :k].view(np.uint32), fit_ref[b, :k].view(np.uint32), err_msg=f"pair {b}")


def test_degenerate_pairs_still_fail_the_call_without_the_knob():
    L, lib = _lib()
    assert L.knob("eyoc_registration_accept_degenerate", -1) == 0          # off by default
    with pytest.raises(L.EyocError, match="at least 4 correspondences"):
        _ransac(L, SIZES)
    # (an empty segment reaches the library and gets ITS error; Matcher._params used to divide by the empty pair's size first)
    with pytest.raises(L.EyocError, match=r"eyoc_sc2pcr: n 0 not in \[8,"):
        _sc2(SIZES)


# ---- split16 overflow of one step: that step again in fp32, the next one in split16

@pytest.fixture(scope="module")
def doctored():
    import test_gpu_range_guard as rg
    from eyoc_amd import synthetic as syn
    from oracle import coords as oc
    from oracle import resunet as orr
    p = syn.make_pair(3, beams=32, azimuths=1000, band=None)
    coords = syn.batch_coords([p["coords0"], p["coords1"]])
    feats = np.ones((len(coords), 1), np.float32)
    sd = syn.make_weights()
    _, inter, _ = orr.resunet_forward(sd, coords, feats, maps=oc.build_maps(coords, 5), return_intermediate=True)
    base = {k: v.numpy() for k, v in inter["stored"].items()}
    bad, _ = rg.doctor(sd, base, "block1.conv1")
    return rg.make_model, bad


@pytest.mark.parametrize("use_ransac", [True, False], ids=["ransac", "sc2pcr"])
def test_split16_overflow_reruns_only_that_step_in_fp32(doctored, use_ransac):
    _lib()
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import RETRIED_FP32, DeviceBatch, RegistrationConfig, RegistrationPipeline
    make_model, sd = doctored
    pairs = [syn.make_pair(s, beams=32, azimuths=1000, band=None) for s in (3, 4)]
    dev = torch.device("cuda")
    sc2 = dict(RegistrationConfig().sc2pcr, num_node=2000, max_points=2000)
    kw = dict(ransac_max_iteration=100000, n_points=2000, use_RANSAC=use_ransac, sc2pcr=sc2)
    batch = DeviceBatch(pairs, [3, 4], dev, n_points=2000, descriptor=dict(inlier_ratio=0.3))
    ref_pipe = RegistrationPipeline(make_model(sd, "fp32"), RegistrationConfig(**kw))
    ref = ref_pipe.register(batch, seed=7)
    ref_dev = ref_pipe.register(batch, seed=7, return_device=True).cpu()

    m = make_model(sd, "auto")
    pipe = RegistrationPipeline(m, RegistrationConfig(fp32_retry_per_step=True, **kw))
    got = pipe.register(batch, seed=7)
    assert m.spconv_math == "auto" and pipe.fp32_retries == 1
    for r0, r1 in zip(got, ref):
        assert r0.status == RETRIED_FP32
        np.testing.assert_array_equal(r0.transformation, r1.transformation)
    # the next step starts in split16 again - pipelined, on the tail stream; wait() re-runs it in fp32
    step = pipe.enqueue(batch, seed=7, tail_stream=True)
    assert m.last_spconv_math == "split16"
    host, overflow = step.wait()
    assert overflow and pipe.fp32_retries == 2 and m.spconv_math == "auto"
    assert (step.status == RETRIED_FP32).all() and len(step.status) == batch.P
    np.testing.assert_array_equal(host.numpy().view(np.uint8), ref_dev.numpy().view(np.uint8))
    m.check_range()                                        # nothing left behind in the guard


@pytest.mark.parametrize("use_ransac", [True, False], ids=["ransac", "sc2pcr"])
def test_retry_leaves_the_step_in_flight_alone(use_ransac):
    """Two steps in flight (the bench's schedule): step A overflows split16 (features of 1e5 in one cloud), step B - enqueued on the other
    slot before A is waited for - does not.  A's fp32 re-run inside ``wait`` must not touch B: B's records are its clean ones, bit for
    bit (on the SC2-PCR path B's index upload still sits in ITS slot's staging), and what the pipeline keeps about the last step stays B's."""
    _lib()
    import test_gpu_range_guard as rg
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import RETRIED_FP32, DeviceBatch, RegistrationConfig, RegistrationPipeline
    pairs = [syn.make_pair(s, beams=32, azimuths=1000, band=None) for s in (3, 4)]
    hot = [pairs[0], dict(pairs[1], feats0=pairs[1]["feats0"] * np.float32(1e5))]
    sd = syn.make_weights()
    dev = torch.device("cuda")
    sc2 = dict(RegistrationConfig().sc2pcr, num_node=2000, max_points=2000)
    kw = dict(ransac_max_iteration=100000, n_points=2000, use_RANSAC=use_ransac, sc2pcr=sc2)
    desc = dict(inlier_ratio=0.3)
    A = DeviceBatch(hot, [3, 4], dev, n_points=2000, descriptor=desc)
    B = DeviceBatch(pairs, [5, 6], dev, n_points=2000, descriptor=desc)
    ref_a = RegistrationPipeline(rg.make_model(sd, "fp32"), RegistrationConfig(**kw)).register(A, seed=7, return_device=True).cpu()
    clean = RegistrationPipeline(rg.make_model(sd, "auto"), RegistrationConfig(**kw))
    ref_b = clean.register(B, seed=9, return_device=True).cpu()
    clean.model.check_range()                                  # B alone does not overflow
    assert clean.model.last_spconv_math == "split16"

    m = rg.make_model(sd, "auto")
    pipe = RegistrationPipeline(m, RegistrationConfig(fp32_retry_per_step=True, **kw))
    step_a = pipe.enqueue(A, seed=7, slot=0, tail_stream=True)
    step_b = pipe.enqueue(B, seed=9, slot=1, tail_stream=True)
    featured, matched = pipe.featured, pipe.matched
    host_a, over_a = step_a.wait()
    assert over_a and pipe.fp32_retries == 1 and m.spconv_math == "auto"
    assert pipe.slot == 1 and pipe.featured is featured and pipe.matched is matched
    host_a = host_a.clone()
    host_b, over_b = step_b.wait()
    assert not over_b and pipe.fp32_retries == 1
    assert (step_a.status == RETRIED_FP32).all() and (step_b.status == 0).all()
    np.testing.assert_array_equal(host_a.numpy().view(np.uint8), ref_a.numpy().view(np.uint8))
    np.testing.assert_array_equal(host_b.numpy().view(np.uint8), ref_b.numpy().view(np.uint8))
    m.check_range()
