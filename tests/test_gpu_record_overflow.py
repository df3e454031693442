"""Real map builds whose tile records overflow, and the forward after them (coordmap.hip ``MapBuild::read_back_records``, model.hip
``eyoc_model_forward``): the clouds of tests/record_overflow_cases.py, each built Z-ordered with every record family requested.  What
the build kept (``eyoc_maps_records``) must be the numpy prediction bit for bit, and the forward - whose layers of a dropped family
run on the gathering kernels and fill a lazily skipped table on first use - must meet the oracle, repeat its bits, not depend on the
lazy tables, and leave every table equal to the oracle's."""
import numpy as np
import pytest
import torch

import record_overflow_cases as roc

pytestmark = pytest.mark.gpu

REL = 1e-4                                                       # the project's gate of a forward against the oracle


def _lib():
    from eyoc_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def net():
    from test_gpu_round2 import _model
    model, sd = _model()
    model.spconv_math = "split16"                                # the record kernels are split16 kernels; some clouds are below 8192 rows
    return model, sd


@pytest.fixture
def every_family_requested():
    """Z-order whatever the size, and the batch paths - class-major records, lazy tables, strided and wide stride-1 records - from
    the first row on."""
    L = _lib()
    prev_order = L.knob("eyoc_maps_internal_order", 1) - 2
    prev_min = L.knob("eyoc_spconv_upc_min_rows", 0)
    prev_up = L.knob("eyoc_spconv_select_up_kernel", -1)
    prev_lazy = L.knob("eyoc_maps_lazy_tables", -1)
    assert L.knob("eyoc_spconv_select_down_kernel", -7) == 1, "strided records are requested by default"
    yield
    L.knob("eyoc_maps_lazy_tables", prev_lazy)
    L.knob("eyoc_spconv_select_up_kernel", prev_up)
    L.knob("eyoc_spconv_upc_min_rows", prev_min)
    L.knob("eyoc_maps_internal_order", prev_order)


_REF = {}


def _reference(name, sd):
    """Per case, once: the cloud, its features, the oracle's maps of the Morton-ordered cloud, the oracle's forward."""
    if name not in _REF:
        from oracle import coords as oc, resunet as orr
        coords = roc.cloud(name)
        feats = np.random.default_rng(len(coords)).uniform(0.5, 1.5, size=(len(coords), 1)).astype(np.float32)
        order = roc.morton_order(coords[:, 1:])
        maps = oc.build_maps(coords[order])
        want = np.asarray(orr.resunet_forward(sd, coords, feats))
        assert np.isfinite(want).all()
        want.setflags(write=False)
        _REF[name] = dict(coords=coords, feats=feats, order=order, maps=maps, want=want, peaks=roc.peaks(maps))
    return _REF[name]


def _tensor(ref):
    import eyoc_amd
    return eyoc_amd.SparseTensor(torch.from_numpy(ref["feats"]).cuda(), coordinates=torch.from_numpy(ref["coords"]).cuda())


def _dropped(table, req):
    return {roc.FAMILIES[f]: [l for l in range(roc.LEVELS) if req[f, l] and not table[f, l]] for f in range(len(roc.FAMILIES))
            if (req[f] > table[f]).any()}


@pytest.mark.parametrize("up", [2, 1])
@pytest.mark.parametrize("name", list(roc.CASES))
def test_build_keeps_what_the_prediction_says_and_the_forward_meets_the_oracle(net, every_family_requested, name, up):
    L = _lib()
    model, sd = net
    ref = _reference(name, sd)
    cfg = dict(up=up, down=1, s1w=1)
    want_records = roc.predict(None, cfg, ref["maps"])
    np.testing.assert_array_equal(want_records, roc.intended(name, cfg))
    L.knob("eyoc_spconv_select_up_kernel", up)
    outs = []
    for lazy in (1, 0):
        L.knob("eyoc_maps_lazy_tables", lazy)
        x = _tensor(ref)
        out = model(x).F
        assert model.last_spconv_math == "split16"
        cm = x.coordinate_manager
        # what the build kept
        np.testing.assert_array_equal(cm.row_order().cpu().numpy(), ref["order"])
        got_records = np.asarray(cm.records(internal=True))
        print(f"{name}, up kernel {up}, lazy {lazy}: {len(ref['coords'])} rows, dropped {_dropped(got_records, roc.requested(cfg))}")
        np.testing.assert_array_equal(got_records, want_records, err_msg=f"families {roc.FAMILIES} x levels")
        # parity, then the same bits again
        f = out.cpu().numpy()
        err = float(np.abs(f - ref["want"]).max())
        print(f"    forward vs oracle: {err / np.abs(ref['want']).max():.2e} of max |oracle|")
        assert np.isfinite(f).all() and err <= REL * np.abs(ref["want"]).max()
        assert torch.equal(model(x).F, out), "a second forward on the same maps gives other bits"
        # every table, the ones the build skipped and a fallback had to fill included
        for l in range(roc.LEVELS):
            np.testing.assert_array_equal(cm.table(L.MAP_S1, l, internal=True).cpu().numpy(), ref["maps"]["s1"][l], err_msg=f"s1 {l}")
            if l + 1 < roc.LEVELS:
                np.testing.assert_array_equal(cm.table(L.MAP_UP, l, internal=True).cpu().numpy(), ref["maps"]["up"][l], err_msg=f"up {l}")
                np.testing.assert_array_equal(cm.table(L.MAP_DOWN, l, internal=True).cpu().numpy(), ref["maps"]["down"][l], err_msg=f"down {l}")
        assert torch.equal(model(x).F, out), "the forward after the accessors filled the tables gives other bits"
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "lazy tables change the forward's bits"


@pytest.mark.parametrize("name", list(roc.CASES))
def test_listed_rows_equal_the_full_forward_on_clouds_that_fall_back(net, every_family_requested, name):
    """``model(x, rows=r) == model(x).F[r]`` bit for bit (the criterion of tests/test_gpu_sampled_tail.py): the sampled-rows layer and
    the tail in the epilogue both need the stride-1 records of level 0, which four of the clouds lose."""
    L = _lib()
    model, sd = net
    ref = _reference(name, sd)
    n = len(ref["coords"])
    rng = np.random.default_rng(17)
    rows = np.concatenate([rng.permutation(n)[:300], ref["order"][:3], ref["order"][-3:], ref["order"][(n // 256) * 256:][:8], [0, n - 1]])
    rows = np.concatenate([rows, rows[:20]]).astype(np.int64)   # duplicates allowed
    x = _tensor(ref)
    full = model(x).F.cpu().numpy()
    kept_s1 = x.coordinate_manager.records(internal=True)[roc.S1][0]
    assert kept_s1 == (0 if "s1" in roc.CASES[name][1] else 1)
    prev = L.knob("eyoc_model_sampled_tail", -1)
    try:
        for sampled in (1, 0):
            L.knob("eyoc_model_sampled_tail", sampled)
            got = model(x, rows=torch.from_numpy(rows).cuda()).cpu().numpy()
            assert got.shape == (len(rows), 32) and got.dtype == np.float32
            np.testing.assert_array_equal(got, full[rows], err_msg=f"sampled tail {sampled}")
    finally:
        L.knob("eyoc_model_sampled_tail", prev)
    assert np.abs(full[rows] - ref["want"][rows]).max() <= REL * np.abs(ref["want"]).max()


@pytest.mark.parametrize("kernel", [0, 1, 3])
def test_first_convolution_without_level_1_records(net, every_family_requested, kernel):
    """``carpet_s1`` loses the level-1 stride-1 records the staged first convolutions read (``a.local1``): whatever
    eyoc_spconv_select_conv1_kernel asks for - the values tests/test_gpu_conv1_persistent.py exercises - the probing kernel runs, so
    the features are those of setting 0 bit for bit, and they meet the oracle."""
    L = _lib()
    model, sd = net
    ref = _reference("carpet_s1", sd)
    assert L.knob("eyoc_spconv_select_conv1_kernel", -1) == 3          # the default, which the first test of this file ran under
    x0 = _tensor(ref)
    prev = L.knob("eyoc_spconv_select_conv1_kernel", 0)
    try:
        base = model(x0).F
        L.knob("eyoc_spconv_select_conv1_kernel", kernel)
        x = _tensor(ref)
        out = model(x).F
    finally:
        L.knob("eyoc_spconv_select_conv1_kernel", prev)
    assert np.asarray(x.coordinate_manager.records(internal=True))[roc.S1].tolist() == [0, 0, 0, 0]
    assert torch.equal(out, base)
    assert np.abs(out.cpu().numpy() - ref["want"]).max() <= REL * np.abs(ref["want"]).max()


def test_accessor_refuses_bad_arguments(every_family_requested):
    L = _lib()
    lib = L.load()
    import eyoc_amd
    coords = roc.cloud("stars")
    cm = eyoc_amd.CoordinateManager(torch.from_numpy(coords).cuda())
    m = cm.maps(1)
    assert [lib.eyoc_maps_records(m, roc.UPC, l) for l in range(4)] == [0, 1, 1, 0]
    for family, level in ((-1, 0), (5, 0), (0, -1), (0, 4)):
        assert lib.eyoc_maps_records(m, family, level) == -1
    assert lib.eyoc_maps_records(None, 0, 0) == -1
