"""Whole-forward parity of EVERY ResUNet channel table (``eyoc_amd.load_model``'s BN2, BN2B, BN2D, BN2E, FatBN and the 3-in / 64-out
BN2C variant) on every kernel path of ``eyoc_model_forward`` against ``oracle.resunet.resunet_forward``, which reads the shapes from
the state dict and is itself pinned by tests/test_oracle_channel_tables.py.  Which layer of which model takes which kernel is
written down in tests/channel_tables.py (``EXPECT``); the switches below show that the path under test really ran.

Clouds (the smallest at which each path still has more than one tile or a ragged one; features uniform(0.5, 1.5)):
  S  two clouds of 2269 rows together, levels 2269 / 1698 / 430 / 128 - ragged last tiles, a coarsest level of exactly one 128-row tile;
     every batch path forced onto it (Z-order, class-major transposed records, lazy tables, 128-row strided tiles, wide workgroups)
  M  two clouds of 14291 rows together (>= 8192: automatic mode itself picks Z-order and split16)
  F  cloud S with no knob set: fp32 MFMAs on the caller's row order

Bars (the project's own): max |got - want| <= 1e-4 max |want| and, for unit-norm features, row cosine >= 1 - 1e-6; against the
float64 oracle e_split16 <= 2 e_fp32 + 1e-7 and e_fp32 < 1e-5; a permutation of the caller's rows permutes the output (< 1e-5);
the same forward twice gives the same bits.  No row is masked out: the oracle answers every table on S and M with finite rows."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from channel_tables import EXPECT, TABLES, features, weights

pytestmark = pytest.mark.gpu

REL = 1e-4
NAMES = list(TABLES)
FUSED = [n for n in NAMES if EXPECT[n][3]]              # the 96 -> 64 -> 32 tails: fused epilogue and sampled rows
assert FUSED == ["BN2B", "BN2D"]
FORCED = dict(spconv_upc_min_rows=0, maps_internal_order=1, spconv_st_split_below=0)      # cloud S


@contextlib.contextmanager
def knobs(**kv):
    """Set ``eyoc_<name>`` switches of the device's ctx for the block; the previous values come back whatever happens inside."""
    from eyoc_amd import _lib
    prev = []
    try:
        for k, v in kv.items():
            p = _lib.knob("eyoc_" + k, v)
            prev.append((k, p - 2 if k == "maps_internal_order" else p))       # (that setter answers previous + 2)
        yield
    finally:
        for k, p in reversed(prev):
            _lib.knob("eyoc_" + k, p)


@functools.lru_cache(maxsize=None)
def cloud(which):
    from eyoc_amd import synthetic as syn
    if which == "S":
        rng = np.random.default_rng(4)
        c = np.unique(rng.integers(-12, 12, size=(2500, 3)), axis=0).astype(np.int32)
        rng.shuffle(c)
        coords = syn.batch_coords([c[:1200], c[1200:]])
        assert len(coords) == 2269
    else:
        p = syn.make_pair(5, beams=24, azimuths=700, band=None)
        coords = syn.batch_coords([p["coords0"], p["coords1"]])
        assert len(coords) == 14291
    return coords


@functools.lru_cache(maxsize=None)
def oracle_maps(which, ks):
    from oracle import coords as oc
    maps = oc.build_maps(cloud(which), ks)
    if which == "S":
        assert [len(c) for c in maps["cm"]] == [2269, 1698, 430, 128]
    return maps


@functools.lru_cache(maxsize=None)
def oracle(name, which, f64=False):
    """-> {"unit": normalised features, "raw": the same before the row normalisation}; once per (table, cloud, dtype)."""
    from oracle import resunet as orr
    ks = TABLES[name][5]
    coords = cloud(which)
    out, inter, _ = orr.resunet_forward(weights(name), coords, features(name, len(coords)), conv1_kernel_size=ks, maps=oracle_maps(which, ks),
                                        return_intermediate=True, dtype=torch.float64 if f64 else torch.float32)
    ref = {"unit": out.numpy(), "raw": inter["pre_norm"].numpy()}
    assert np.isfinite(ref["unit"]).all() and np.isfinite(ref["raw"]).all(), "a non-finite oracle row: change the seed, mask nothing"
    return ref


@functools.lru_cache(maxsize=None)
def model(name, normalize=True):
    import eyoc_amd
    cls, _C, _T, cin, cout, ks, _seed = TABLES[name]
    m = eyoc_amd.load_model(cls)(cin, cout, bn_momentum=0.05, conv1_kernel_size=ks, normalize_feature=normalize)
    missing = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights(name).items()})
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.cuda().eval()


def sparse(name, which, perm=None):
    """A fresh tensor: its maps are built under the switches set at this moment."""
    import eyoc_amd
    coords = cloud(which)
    feats = features(name, len(coords))
    if perm is not None:
        coords, feats = coords[perm], feats[perm]
    return eyoc_amd.SparseTensor(torch.from_numpy(feats).cuda(), coordinates=torch.from_numpy(coords).cuda())


def forward(m, name, which, perm=None):
    return m(sparse(name, which, perm)).F.clone()


def err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def worst_cos(got, want):
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(((g * w).sum(1) / (np.linalg.norm(g, axis=1) * np.linalg.norm(w, axis=1))).min())


def meets_bar(got, name, which, unit=True, what=""):
    """The oracle bar on EVERY row; prints the realised figures first."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    want = oracle(name, which)["unit" if unit else "raw"]
    assert got.shape == want.shape and np.isfinite(got).all()
    e, c = err(got, want), worst_cos(got, want)
    print(f"{name} {which} {what}: err {e:.2e} worst cosine 1 - {1 - c:.1e}")
    assert e <= REL, (name, which, what, e)
    if unit:
        assert c >= 1 - 1e-6, (name, which, what, c)
        np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    return e


def permuted(m, name, which, base, seed=3):
    """Row-order contract: permuting the caller's rows permutes the output."""
    perm = np.random.default_rng(seed).permutation(len(cloud(which)))
    got = forward(m, name, which, perm).cpu().numpy()
    want = base.cpu().numpy()[perm]
    assert err(got, want) < 1e-5


# ------------------------------------------------------------------------------------------------ S: every batch path forced
@pytest.mark.parametrize("name", NAMES)
def test_forced_batch_paths_on_a_small_cloud(name):
    """Cloud S with the knobs of test_gpu_down.py::test_batch_kernels_on_small_and_odd_inputs: Z-ordered rows, class-major transposed
    records with lazy tables, 128-row strided tiles, 128-row x 128-channel workgroups on the coarsest level (one tile), 64-channel
    workgroups on the stride-1 layers - so that the tail rides in block2_tr.conv2's epilogue where the table allows it.  Then the
    record kernels off (eyoc_spconv_select_split16_kernel 0: every layer on the wave-private gathering kernel) and on (2)."""
    m = model(name)
    m.spconv_math = "split16"
    try:
        with knobs(**FORCED):
            base = forward(m, name, "S")
            assert m.last_spconv_math == "split16"
            meets_bar(base, name, "S", what="forced batch paths")
            assert torch.equal(base, forward(m, name, "S")), "not reproducible"
            permuted(m, name, "S", base)
            outs = {}
            for sel in (0, 2):
                with knobs(spconv_select_split16_kernel=sel):
                    outs[sel] = forward(m, name, "S")
                    assert m.last_spconv_math == "split16"
                meets_bar(outs[sel], name, "S", what=f"split16 kernel selection {sel}")
            assert not torch.equal(outs[0], outs[2]), "both selections took the same kernels - the switch did nothing"
            # the fused tail: 0 two launches, 1 spconv_tail.hip, 2 the epilogue of block2_tr.conv2 (64-channel workgroups: it runs here)
            tails = {}
            for fuse in (0, 1, 2):
                with knobs(model_fuse_tail=fuse):
                    tails[fuse] = forward(m, name, "S")
                meets_bar(tails[fuse], name, "S", what=f"fuse_tail {fuse}")
            assert torch.equal(tails[2], base)                                   # 2 is the default
            if EXPECT[name][3]:
                assert not torch.equal(tails[0], tails[1]), "the fused tail did not run"
                assert torch.equal(tails[2], tails[1])                           # the same products in the same order
            else:                                                                # tail_fusable says no: one path whatever the switch
                assert torch.equal(tails[0], tails[1]) and torch.equal(tails[1], tails[2])
            if TABLES[name][4] == 64:                                            # the unnormalised 64-channel output
                mr = model(name, normalize=False)
                mr.spconv_math = "split16"
                try:
                    meets_bar(forward(mr, name, "S"), name, "S", unit=False, what="forced batch paths, unnormalised")
                finally:
                    mr.spconv_math = "auto"
    finally:
        m.spconv_math = "auto"


# ------------------------------------------------------------------------------------------------ F: fp32 on the caller's rows
@pytest.mark.parametrize("kernel", [0, 1], ids=["tiled", "wave"])
@pytest.mark.parametrize("name", NAMES)
def test_fp32_forward_in_the_callers_row_order(name, kernel):
    m = model(name)
    with knobs(spconv_select_kernel=kernel):
        x = sparse(name, "S")
        base = m(x).F.clone()
        assert m.last_spconv_math == "fp32" and x.coordinate_manager.row_order() is None
        meets_bar(base, name, "S", what=f"fp32, spconv kernel {kernel}")
        assert torch.equal(base, forward(m, name, "S")), "not reproducible"
        permuted(m, name, "S", base)
        if TABLES[name][4] == 64:
            meets_bar(forward(model(name, normalize=False), name, "S"), name, "S", unit=False, what=f"fp32, spconv kernel {kernel}, unnormalised")


# ------------------------------------------------------------------------------------------------ M: what automatic mode picks
@pytest.fixture
def batch_kernels_from_8192_rows():
    """class-major transposed records, lazy tables and the staged strided kernel start at 2^17 rows in production: lowered as in
    test_gpu_down.py so that cloud M runs them"""
    with knobs(spconv_upc_min_rows=8192):
        yield


@pytest.mark.parametrize("name", NAMES)
def test_automatic_paths_on_a_batch(batch_kernels_from_8192_rows, name):
    m = model(name)
    assert m.spconv_math == "auto"
    x = sparse(name, "M")
    base = m(x).F.clone()
    assert m.last_spconv_math == "split16" and x.coordinate_manager.row_order() is not None
    meets_bar(base, name, "M", what="automatic")
    assert torch.equal(base, forward(m, name, "M")), "not reproducible"
    permuted(m, name, "M", base)
    # error growth against the float64 oracle, next to the fp32-MFMA forward of the same maps
    want64 = oracle(name, "M", f64=True)["unit"]
    m.spconv_math = "fp32"
    try:
        f32 = forward(m, name, "M")
        assert m.last_spconv_math == "fp32"
    finally:
        m.spconv_math = "auto"
    meets_bar(f32, name, "M", what="fp32 on Z-ordered rows")
    e16, e32 = err(base.cpu().numpy(), want64), err(f32.cpu().numpy(), want64)
    print(f"{name} M vs float64 oracle: fp32 {e32:.2e} split16 {e16:.2e}")
    assert e32 < 1e-5 and e16 <= 2 * e32 + 1e-7, (name, e32, e16)
    if TABLES[name][4] == 64:
        meets_bar(forward(model(name, normalize=False), name, "M"), name, "M", unit=False, what="automatic, unnormalised")
        assert model(name, normalize=False).last_spconv_math == "split16"


@pytest.mark.parametrize("name", NAMES)
def test_record_kernel_families_off_and_on(batch_kernels_from_8192_rows, name):
    """Each family of record kernels switched off and on by its selector on cloud M: every setting meets the oracle bar; the outputs
    differ in their bits where the table has a layer the switched kernel accepts (another summation order - the switch did something)
    and are bit-identical where the dispatch must decline (channel_tables.EXPECT)."""
    m = model(name)

    def run(**kv):
        with knobs(**kv):
            out = forward(m, name, "M")
        assert m.last_spconv_math == "split16"
        meets_bar(out, name, "M", what=str(kv))
        return out

    # strided convolutions conv2 / conv3 / conv4: gathering kernel / 128-row tiles (every table: outputs of 64, 128, 256 channels);
    # the selector also decides whether block4's 256-channel layers get their 128-row x 128-channel workgroups
    down = {v: run(spconv_select_down_kernel=v) for v in (0, 1)}
    assert not torch.equal(down[0], down[1]), "strided layers: the switch did nothing"
    # transposed convolutions: gathering / spconv_up.hip / spconv_upc.hip (every table: outputs of 64, 128 or 256 channels).  Off
    # against either record kernel: other bits.  Under 2 the maps hold class-major records ONLY (coordmap.hip: use_up is false once
    # use_upc is true), so bits that differ from the gathering kernel's are spconv_upc.hip's.  The two record kernels against each
    # other prove nothing either way: both sum a row's products block by block over its class's offsets in ascending order, so they
    # agree bit for bit unless a class tile stages in two passes (none does on this cloud) - printed, not asserted
    up = {v: run(spconv_select_up_kernel=v) for v in (0, 1, 2)}
    assert not torch.equal(up[0], up[1]) and not torch.equal(up[0], up[2]), "transposed layers: a switch did nothing"
    print(f"{name} M spconv_up.hip and spconv_upc.hip agree bit for bit: {torch.equal(up[1], up[2])}")
    assert torch.equal(up[2], down[1])                                          # both are the defaults
    # the 1x1 tail.  Cloud M has 56 level-0 tiles: 32-channel workgroups, so mode 2 runs the tail kernel of mode 1 (the epilogue
    # itself is forced on cloud S above)
    tail = {v: run(model_fuse_tail=v) for v in (0, 1, 2)}
    assert torch.equal(tail[2], tail[1]) and torch.equal(tail[2], down[1])
    if EXPECT[name][3]:
        assert not torch.equal(tail[0], tail[1]), "the fused tail did not run"
    else:
        assert torch.equal(tail[0], tail[1]), "a tail that is not 96 -> 64 -> 32 was fused"


# ------------------------------------------------------------------------------------------------ model(x, rows=...)
@pytest.mark.parametrize("name", NAMES)
def test_listed_rows(batch_kernels_from_8192_rows, name):
    """700 rows drawn with duplicates plus the first and the last row of cloud M.  BN2B / BN2D: block2_tr.conv2 and the tail run for
    the listed rows only (spconv_rows.hip) and ``layer_work`` reports it; every other table: the full output goes to the workspace and
    its rows are copied out, whatever eyoc_model_sampled_tail says.  Either way the rows are the full forward's, bit for bit."""
    m = model(name)
    n = len(cloud("M"))
    rng = np.random.default_rng(17)
    idx = rng.integers(0, n, 700)
    idx[100:200] = idx[:100]
    idx = np.concatenate([idx, [0, n - 1]]).astype(np.int64)
    rows = torch.from_numpy(idx).cuda()
    x = sparse(name, "M")
    full = m(x).F.clone()
    assert m.last_spconv_math == "split16"
    plain = m.layer_work(x)
    names = [w["name"] for w in plain]
    li = names.index("block2_tr.conv2")
    assert names[li + 1:] == ["conv1_tr", "final"]
    s1 = oracle_maps("M", TABLES[name][5])["s1"][0]
    assert plain[li]["pairs"] == int((s1 >= 0).sum()) and plain[li + 1]["pairs"] == plain[li + 2]["pairs"] == n
    for sampled in (1, 0):
        with knobs(model_sampled_tail=sampled):
            got = m(x, rows=rows)
            work = m.layer_work(x)
        assert got.shape == (len(idx), TABLES[name][4])
        assert torch.equal(got, full[rows]), f"sampled_tail {sampled}"
        if EXPECT[name][3] and sampled:
            c = EXPECT[name][5]
            assert work[li]["pairs"] == int((s1[:, idx] >= 0).sum())
            assert work[li + 1]["pairs"] == work[li + 2]["pairs"] == len(idx)
            assert work[li]["flop"] == 2.0 * work[li]["pairs"] * c * c and work[:li] == plain[:li]
        else:
            assert work == plain, "the rows kernel ran for a layer it must decline"
    want = oracle(name, "M")["unit"]
    e = float(np.abs(got.cpu().numpy() - want[idx]).max() / np.abs(want).max())
    print(f"{name} M listed rows: err {e:.2e}")
    assert e <= REL and worst_cos(got.cpu().numpy(), want[idx]) >= 1 - 1e-6
    m(x)
    assert m.layer_work(x) == plain


# ------------------------------------------------------------------------------------------------ refusals
def test_a_normalised_128_channel_output_has_no_split16_forward(batch_kernels_from_8192_rows):
    """``normalize_feature=True, out_channels=128``: the row normalisation needs the whole row in one tile, which only the fp32
    workgroup-tiled kernel has (``split_ok`` in forward_math, model.hip).  Asking for split16 raises; automatic mode runs fp32 on cloud M and
    meets the bar."""
    import eyoc_amd
    from eyoc_amd import _lib, synthetic as syn
    from oracle import resunet as orr
    sd = syn.make_weights(27, out_channels=128)
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 128, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    coords = cloud("M")
    feats = features("BN2", len(coords))
    x = eyoc_amd.SparseTensor(torch.from_numpy(feats).cuda(), coordinates=torch.from_numpy(coords).cuda())
    m.spconv_math = "split16"
    with pytest.raises(_lib.EyocError):
        m(x)
    m.spconv_math = "auto"
    got = m(x).F.cpu().numpy()
    assert m.last_spconv_math == "fp32"
    want = orr.resunet_forward(sd, coords, feats, maps=oracle_maps("M", 5)).numpy()
    assert np.isfinite(want).all()
    e, c = err(got, want), worst_cos(got, want)
    print(f"BN2C out 128 normalised, M, automatic -> fp32: err {e:.2e} worst cosine 1 - {1 - c:.1e}")
    assert e <= REL and c >= 1 - 1e-6
