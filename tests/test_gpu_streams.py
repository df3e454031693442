"""Cross-stream use of coordinate maps and of the ctx scratch, made deterministic.

A producer is enqueued on stream A behind a self-terminating spin (``busy``) and a consumer on stream B right away: unless the
library orders B behind A, the consumer runs while the producer's work has not started.  Every race test first asserts that this
window is open (A still busy when the consumer is enqueued), then compares the results exactly with the oracle or with the same
computation run serially.

The maps workspace is filled with 0xFF bytes before every build: a [27][n] table the build left for a later fill then reads as all
-1 ("no neighbour") and the level-0 hash table as KEY_EMPTY, so a consumer that runs too early sees wrong values - never an
out-of-range index and never an unbounded probe loop.  (The reserved table regions are carved from the workspace on their own and
are never build temporaries: coordmap.hip eyoc_maps_build_ordered.)"""
import contextlib
import ctypes as C
import time
import weakref

import numpy as np
import pytest
import torch

import _inputs as gi

pytestmark = pytest.mark.gpu

BUSY_MS = 200                 # the window every race test holds open on A (each spin <= 300 ms)
_CYCLES_PER_MS = []


# ----------------------------------------------------------------------------------------------------------------- the harness
def _cycles_per_ms():
    """``torch.cuda._sleep`` cycles per millisecond, measured once per session with events (the counter's rate is the device's)."""
    if not _CYCLES_PER_MS:
        s = torch.cuda.Stream()
        cycles = 1 << 20
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                torch.cuda._sleep(cycles)
                e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 20.0:
                break
            cycles = int(cycles * min(64.0, 40.0 / max(ms, 0.01)))     # ~40 ms at most for the next measurement
        assert ms > 1.0, f"torch.cuda._sleep({cycles}) took {ms} ms: cannot calibrate the spin"
        _CYCLES_PER_MS.append(cycles / ms)
    return _CYCLES_PER_MS[0]


def busy(stream, ms=BUSY_MS):
    """Occupies ``stream`` for about ``ms`` milliseconds (at most 300) with a spin that ends by itself."""
    cycles = int(min(ms, 300) * _cycles_per_ms())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def independent_streams():
    """Two torch streams that really run concurrently on this device (with 4 hardware queues two pool streams can share one):
    A busy, a tiny op on B, B synchronised - A must still be busy.  At most 8 pool streams are tried for B."""
    a = torch.cuda.Stream()
    for _ in range(8):
        b = torch.cuda.Stream()
        torch.cuda.synchronize()
        busy(a, 100)
        with torch.cuda.stream(b):
            torch.empty(64, device="cuda").fill_(1.0)
        b.synchronize()
        concurrent = not a.query()
        a.synchronize()
        if concurrent:
            return a, b
    pytest.fail("no pool stream ran beside stream A in 8 tries: the race tests need two concurrent streams")


@pytest.fixture
def streams():
    return independent_streams()


def window_open(a):
    assert not a.query(), "stream A finished its spin before the consumer was enqueued: the race window is closed"


@contextlib.contextmanager
def knobs(**kv):
    from eyoc_amd import _lib
    prev = {}
    try:
        for k, v in kv.items():
            prev[k] = _lib.knob(k, v)
        yield
    finally:
        for k, v in prev.items():
            _lib.knob(k, v)


@pytest.fixture
def poisoned():
    """Every maps workspace (and only that) is filled with 0xFF bytes on the build's stream before the build."""
    from eyoc_amd import _lib
    from eyoc_amd.sparse_tensor import CoordinateManager
    real_build, real_ws = CoordinateManager._build, _lib.workspace

    def poisoned_ws(nbytes, device):
        t = real_ws(nbytes, device)
        t.fill_(0xFF)
        return t

    def build(self, order):
        _lib.workspace = poisoned_ws
        try:
            return real_build(self, order)
        finally:
            _lib.workspace = real_ws

    CoordinateManager._build = build
    try:
        yield
    finally:
        CoordinateManager._build = real_build
        _lib.workspace = real_ws


# ----------------------------------------------------------------------------------------------------------------- the scene
LAZY = dict(eyoc_spconv_upc_min_rows=8192)          # class-major records, and with them lazy tables, for a 2-cloud batch
GATHER = dict(eyoc_spconv_select_split16_kernel=0)  # every split16 layer on the gathering kernel: the forward fills the tables


def _model(sd, ks=5):
    import eyoc_amd
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=ks, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    m.range_check = False       # (the check synchronises the host; nothing here comes near the fp16 range)
    return m


@pytest.fixture(scope="module")
def scene():
    """Two clouds in one Z-ordered batch (>= 8192 rows) with lazy tables; the oracle's maps in the maps' internal row order; two
    models each for conv1 kernel sizes 5 (octree walk) and 7 (probes the level-0 hash table); the forward on eager maps."""
    from eyoc_amd import _lib, synthetic as syn
    from oracle import coords as oc
    p = syn.make_pair(2)
    coords = syn.batch_coords([p["coords0"], p["coords1"]])
    feats = np.random.default_rng(3).uniform(0.5, 1.5, size=(len(coords), 1)).astype(np.float32)
    sd5, sd7 = syn.make_weights(), syn.make_weights(seed=7, conv1_kernel_size=7)
    out = dict(coords=coords, feats=feats, m5=(_model(sd5), _model(sd5)), m7=(_model(sd7, 7), _model(sd7, 7)))
    with knobs(**LAZY):
        assert _lib.knob("eyoc_maps_lazy_tables", -7) == 1
        x = built(out)
        perm = x.coordinate_manager.row_order()
        assert perm is not None, "the scene must be Z-ordered"
        out["perm"] = perm.cpu().numpy()
        with knobs(eyoc_maps_lazy_tables=0):
            out["F_eager"] = out["m5"][0](sparse(out)).F.clone()
    out["want"] = oc.build_maps(coords[out["perm"]], 5)
    out["stats"] = oc.map_stats(out["want"])
    out["pairs_k7"] = oc.map_stats(oc.build_maps(coords, 7))["pairs_k5"]
    torch.cuda.synchronize()
    return out


def sparse(sc):
    import eyoc_amd
    return eyoc_amd.SparseTensor(torch.from_numpy(sc["feats"]).cuda(), coordinates=torch.from_numpy(sc["coords"]).cuda())


def built(sc):
    """``sparse`` with its maps built now, on the current stream, in the order the forward uses (Z-order here)."""
    x = sparse(sc)
    x.coordinate_manager.maps(-1)
    return x


def check_tables(cm, want):
    from eyoc_amd import _lib
    for l in range(4):
        np.testing.assert_array_equal(cm.table(_lib.MAP_S1, l, internal=True).cpu().numpy(), want["s1"][l], err_msg=f"s1 level {l}")
        if l < 3:
            np.testing.assert_array_equal(cm.table(_lib.MAP_UP, l, internal=True).cpu().numpy(), want["up"][l], err_msg=f"up level {l}")
            np.testing.assert_array_equal(cm.table(_lib.MAP_DOWN, l, internal=True).cpu().numpy(), want["down"][l],
                                          err_msg=f"down level {l}")


def check_info(info, stats, conv1=None):
    assert info["rows"] == stats["rows"]
    assert info["pairs_s1"] == stats["pairs_s1"], (info["pairs_s1"], stats["pairs_s1"])
    assert info["pairs_up"] == stats["pairs_up"], (info["pairs_up"], stats["pairs_up"])
    assert info["pairs_down"] == stats["pairs_down"], (info["pairs_down"], stats["pairs_down"])
    assert info["pairs_conv1"] == (stats["pairs_k5"] if conv1 is None else conv1)


def _take_scratch(stream):
    """Makes ``stream`` the last user of the ctx scratch (eyoc_ctx::ensure_scratch orders a user on another stream behind the last
    one): a consumer on B that takes the scratch must not be ordered behind A's producer by that alone."""
    from oracle import matching as om
    import eyoc_amd
    a, b = gi.unit_feats(700, 300), gi.unit_feats(701, 300)
    with torch.cuda.stream(stream):
        got = eyoc_amd.knn1_segmented(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), [0, 300], [0, 300], return_distance=False)
    np.testing.assert_array_equal(got.cpu().numpy(), om.find_nn(a, b))


# ----------------------------------------------------------------------------------------------------------------- poison control
def test_poisoned_workspace_builds_the_oracle_maps(scene, poisoned):
    """The control for the poison: an eager build and a lazy build (whose tables are filled on demand, on one stream) on a 0xFF
    workspace give the oracle's tables and pair counts."""
    for lazy in (0, 1):
        with knobs(eyoc_maps_lazy_tables=lazy, **LAZY):
            cm = built(scene).coordinate_manager
            np.testing.assert_array_equal(cm.row_order().cpu().numpy(), scene["perm"])
            check_tables(cm, scene["want"])
            check_info(cm.info(conv1_kernel_size=5), scene["stats"])


# ----------------------------------------------------------------------------------------------------------------- lazy tables
@pytest.mark.parametrize("consumer", ["table", "table_view", "forward", "info"])
def test_lazy_tables_filled_on_one_stream_read_on_another(scene, poisoned, streams, consumer):
    """A forward on A whose layers run the gathering kernel fills the level-0 stride-1 table and the transposed tables of lazy maps;
    a reader on B right after must see them filled: ``table`` (eyoc_maps_copy_table), ``table_view`` (the raw eyoc_maps_table
    pointer), a second forward with the same kernel, ``info`` (eyoc_maps_info)."""
    from eyoc_amd import _lib
    A, B = streams
    ma, mb = scene["m5"]
    with knobs(**LAZY, **GATHER):
        # serial warm-up of both sides on their streams (packing, allocator blocks per stream) and the serial reference
        x0 = sparse(scene)
        with torch.cuda.stream(A):
            F_serial = ma(x0).F
        torch.cuda.synchronize()
        with torch.cuda.stream(B):
            mb(x0)
            x0.coordinate_manager.table_view(_lib.MAP_UP, 0, internal=True).clone()
        torch.cuda.synchronize()
        if consumer == "info":
            _take_scratch(B)
        x = built(scene)
        cm = x.coordinate_manager
        torch.cuda.synchronize()
        busy(A)
        with torch.cuda.stream(A):
            F_a = ma(x).F
        window_open(A)
        with torch.cuda.stream(B):
            if consumer == "table":
                got = {(k, l): cm.table(k, l, internal=True) for l in range(4) for k in (_lib.MAP_S1, _lib.MAP_UP) if k == _lib.MAP_S1 or l < 3}
            elif consumer == "table_view":
                got = {(k, l): cm.table_view(k, l, internal=True).clone() for l in range(4) for k in (_lib.MAP_S1, _lib.MAP_UP)
                       if k == _lib.MAP_S1 or l < 3}
            elif consumer == "forward":
                F_b = mb(x).F
            else:
                info = cm.info(conv1_kernel_size=5)
        torch.cuda.synchronize()
    want = scene["want"]
    if consumer in ("table", "table_view"):
        for (k, l), t in got.items():
            np.testing.assert_array_equal(t.cpu().numpy(), want["s1" if k == _lib.MAP_S1 else "up"][l], err_msg=f"kind {k} level {l}")
    elif consumer == "forward":
        assert torch.equal(F_b, F_a), float((F_b - F_a).abs().max())
        assert torch.equal(F_a, F_serial)
        assert float((F_b - scene["F_eager"]).abs().max()) < 2e-5
    else:
        check_info(info, scene["stats"])
    check_tables(cm, want)                 # and the maps themselves are right afterwards


# ----------------------------------------------------------------------------------------------------------------- table[0]
def _gather7(cm, feats_internal):
    from eyoc_amd.train import gather_window
    return gather_window(cm, feats_internal, 7, internal=True)


@pytest.mark.parametrize("producer,consumer", [("forward7", "gather"), ("forward7", "info"), ("gather", "forward7"), ("gather", "info")])
def test_level0_hash_table_built_on_one_stream_read_on_another(scene, poisoned, streams, producer, consumer):
    """The level-0 hash table is built on first use - by a 7^3 first convolution (hash probing), by the window gather of the training
    path, by eyoc_maps_info(conv1_kernel_size > 0).  Built on A behind the spin, read on B right after: the same as serially."""
    A, B = streams
    m7a, m7b = scene["m7"]
    fi = torch.from_numpy(scene["feats"][scene["perm"]]).cuda()           # the window gather reads features in the maps' rows

    def run(what, x, model):
        if what == "forward7":
            return model(x).F
        if what == "gather":
            return _gather7(x.coordinate_manager, fi)
        return x.coordinate_manager.info(conv1_kernel_size=7)

    with knobs(**LAZY):
        serial = {}
        x0 = built(scene)
        with torch.cuda.stream(A):
            serial[producer] = run(producer, x0, m7a)
        torch.cuda.synchronize()
        x1 = built(scene)                                      # the consumer's serial result on maps of its own (it builds the table)
        with torch.cuda.stream(B):
            serial[consumer] = run(consumer, x1, m7b)
        torch.cuda.synchronize()
        if consumer == "info":
            _take_scratch(B)
        x = built(scene)
        torch.cuda.synchronize()
        busy(A)
        with torch.cuda.stream(A):
            got_p = run(producer, x, m7a)
        window_open(A)
        with torch.cuda.stream(B):
            got_c = run(consumer, x, m7b)
        torch.cuda.synchronize()
    for what, got in ((producer, got_p), (consumer, got_c)):
        if what == "info":
            check_info(got, scene["stats"], conv1=scene["pairs_k7"])
            check_info(serial[what], scene["stats"], conv1=scene["pairs_k7"])
        else:
            assert torch.equal(got, serial[what]), f"{what}: max |diff| {float((got - serial[what]).abs().max())}"


# ----------------------------------------------------------------------------------------------------------------- workspace lifetime
@pytest.mark.parametrize("reader", ["forward", "lazy_fill"])
def test_maps_workspace_is_not_reused_while_another_stream_reads_it(scene, streams, reader):
    """Maps built on S (``prepare_maps``' side stream), read on M, dropped while M is still busy: the next allocation of the same size
    on S must not get the workspace back (torch's caching allocator hands a block out on its own stream at once unless the block was
    recorded on the streams that use it).  ``lazy_fill``: the reader is a forward that fills lazy tables into the workspace."""
    M, S = streams
    ma = scene["m5"][0]
    kn = dict(LAZY, **GATHER) if reader == "lazy_fill" else LAZY
    with knobs(**kn):
        with torch.cuda.stream(M):                              # warm-up: the forward's allocations on M
            ma(sparse(scene))
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            x = built(scene)
        base = x.coordinate_manager._ws.untyped_storage()
        lo, size = base.data_ptr(), base.nbytes()
        del base
        # a free block on S a little larger than the workspace: the allocation below is then served from S's cache whether or not the
        # workspace is held back - no device allocation, which may synchronise the device (and close the window) when memory is short -,
        # while best fit still prefers the workspace's own block if the allocator were free to hand it out
        with torch.cuda.stream(S):
            spare = torch.empty(size + (4 << 20), dtype=torch.uint8, device="cuda")
        del spare
        cm_alive = weakref.ref(x.coordinate_manager)
        torch.cuda.synchronize()
        allocs = torch.cuda.memory_stats()["num_device_alloc"]
        busy(M, 300)
        with torch.cuda.stream(M):
            F = ma(x).F
        if reader == "lazy_fill":
            busy(M, 150)                                        # dropping the maps waits for their pending fills: M stays busy after
        window_open(M)
        t0 = time.perf_counter()
        del x
        assert cm_alive() is None, "the coordinate manager outlived its SparseTensor"
        with torch.cuda.stream(S):
            blk = torch.empty(size, dtype=torch.uint8, device="cuda")
        still_busy = not M.query()
        dt = time.perf_counter() - t0
        p = blk.data_ptr()
        allocs = torch.cuda.memory_stats()["num_device_alloc"] - allocs
        torch.cuda.synchronize()
    assert still_busy, (f"M finished before the new block was allocated ({1e3 * dt:.1f} ms for the drop and the allocation, {allocs} "
                        f"device allocations since the spin started): the test proves nothing")
    assert p + size <= lo or lo + size <= p, (f"the maps workspace [{lo:#x}, +{size}) was handed out again on the build stream "
                                              f"({p:#x}) while a forward on another stream still read it")
    assert F.shape == (len(scene["coords"]), 32)


def test_pipeline_two_steps_in_flight_dropping_the_maps_at_once(scene):
    """bench.py's ``pipelined_extra`` in tail mode: ``enqueue(tail_stream=True)`` and the maps handle dropped right away, the next
    step's maps (the same batch) built at once on the side stream.  Every step's records are byte-identical to the serial
    ``register``'s."""
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    import eyoc_amd
    cfg = RegistrationConfig(ransac_max_iteration=100000, n_points=2000)
    batch = DeviceBatch([syn.make_pair(s, beams=32, azimuths=1000, band=None) for s in (3, 4)], [3, 4], torch.device("cuda"),
                        n_points=cfg.n_points, descriptor=dict(inlier_ratio=0.3))
    sd = syn.make_weights()
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    m.spconv_math = "split16"
    pipe = RegistrationPipeline(m, cfg)
    want = pipe.register(batch, seed=7, return_device=True).cpu().numpy()
    maps, pend, seen = pipe.prepare_maps(batch), None, 0
    for s in range(6):
        p = pipe.enqueue(batch, seed=7, maps=maps, slot=s & 1, tail_stream=True)
        maps = pipe.prepare_maps(batch)                          # the old handle goes at once
        if pend is not None:
            host, over = pend.wait()
            assert not over
            np.testing.assert_array_equal(host.numpy(), want, err_msg=f"step {s - 1}")
            seen += 1
        pend = p
    host, over = pend.wait()
    assert not over
    np.testing.assert_array_equal(host.numpy(), want, err_msg="last step")
    assert seen == 5


# ----------------------------------------------------------------------------------------------------------------- ctx scratch
def _scratch_op(name, k):
    """(enqueue on the current stream -> device result, check of the result against the oracle): problem ``k`` of each kind."""
    import eyoc_amd
    from eyoc_amd import _lib
    from oracle import labels as ol
    from oracle import matching as om
    if name == "knn1":                                          # no distances asked for: the MFMA pre-filter path (knob 2: always)
        a, b = gi.unit_feats(800 + 2 * k, 5000), gi.unit_feats(801 + 2 * k, 5000)
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        return (lambda: eyoc_amd.knn1_segmented(da, db, [0, 5000], [0, 5000], return_distance=False),
                lambda got: np.testing.assert_array_equal(got.cpu().numpy(), om.find_nn(a, b)))
    if name == "lowe_topk":
        rng = np.random.default_rng(90 + k)
        d1 = rng.uniform(0, 1.5, 6000).astype(np.float32)
        d2 = (d1 + rng.uniform(0, 0.5, 6000).astype(np.float32)).astype(np.float32)
        d1[:40] = 0.0
        t1, t2 = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda()

        def check(got):
            ri, _, rw = ol.topk_matches(ol.lowe_weights(d1, d2), np.arange(6000), 5000)
            np.testing.assert_array_equal(got[0].cpu().numpy(), ri)
            np.testing.assert_array_equal(got[1].cpu().numpy(), rw)
        return (lambda: eyoc_amd.lowe_topk(t1, t2, 5000)), check
    if name == "maps_info":
        from eyoc_amd import synthetic as syn
        from oracle import coords as oc
        rng = np.random.default_rng(60 + k)
        c = syn.batch_coords([np.unique(rng.integers(-30, 30, size=(3000, 3)), axis=0).astype(np.int32)])
        cm = eyoc_amd.CoordinateManager(torch.from_numpy(c).cuda())
        cm.maps()
        st = oc.map_stats(oc.build_maps(c, 5))
        return (lambda: cm.info(conv1_kernel_size=5)), (lambda got: check_info(got, st))
    if name == "ransac":                                        # eyoc_ransac: the ctx-owned scratch entry point
        from oracle import ransac as orn
        T = gi.rigid(0.02, -0.01, 0.3, 1.5, -0.7, 0.1)
        p0, p1, _ = gi.corr_case(300 + k, 1500, T, 0.3, noise=0.03)
        s, t = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
        corr = torch.arange(1500, dtype=torch.int64, device="cuda")
        prm = _lib.RansacParams(0.3, 0.9, 50000, 11 + k)
        lib = _lib.load()

        def run():
            res = torch.zeros(C.sizeof(_lib.RansacResult), dtype=torch.uint8, device="cuda")
            _lib.check(lib.eyoc_ransac(_lib.ctx(), _lib.ptr(s), _lib.ptr(t), _lib.ptr(corr), 1500, C.byref(prm), _lib.ptr(res),
                                       _lib.stream_ptr()), "eyoc_ransac")
            return res

        def check(got):
            r = _lib.RansacResult.from_buffer_copy(got.cpu().numpy().tobytes())
            ref = orn.ransac(p0, p1, np.arange(1500), 0.3, 50000, seed=11 + k)
            assert (r.survivors, r.inliers, r.best_hypothesis) == (ref["survivors"], ref["inliers"], ref["best_h"])
            assert r.survivors > 0 and r.inliers > 0
            assert np.abs(np.array(list(r.T)).reshape(4, 4) - ref["T"]).max() < 1e-5
        return run, check
    raise ValueError(name)


@pytest.mark.parametrize("producer,consumer", [("knn1", "knn1"), ("lowe_topk", "lowe_topk"), ("knn1", "maps_info"), ("ransac", "ransac")])
def test_ctx_scratch_is_handed_between_streams_in_order(streams, producer, consumer):
    """eyoc_ctx::ensure_scratch: a call on B that takes the ctx's scratch while A's call still owns it is ordered behind A's call
    (event on A's stream) - so B is done only after A's spin and call are, and both results equal the oracle's.  The scratch is
    grown serially first: B never has to grow it while A's use is pending."""
    A, B = streams
    with knobs(eyoc_knn_prefilter=2):
        (run_p, check_p), (run_c, check_c) = _scratch_op(producer, 0), _scratch_op(consumer, 1)
        for run, st in ((run_p, A), (run_c, B), (run_p, A)):   # serial: sizes the scratch; the last user is A
            with torch.cuda.stream(st):
                run()
            torch.cuda.synchronize()
        busy(A)
        with torch.cuda.stream(A):
            got_p = run_p()
        window_open(A)
        with torch.cuda.stream(B):
            got_c = run_c()
        B.synchronize()
        ordered = A.query()
        torch.cuda.synchronize()
    assert ordered, "the consumer on B finished before the producer on A: the scratch was not handed over in stream order"
    check_p(got_p)
    check_c(got_c)
