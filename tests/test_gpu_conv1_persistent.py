"""The persistent first convolution (conv1_bfp_kernel, eyoc_spconv_select_conv1_kernel(3)) against conv1_bf_kernel (1): the same
products in the same order, so the network's features and the range-guard words must agree BIT FOR BIT - on every shape at which
the persistent kernel takes another path: one partial tile, exactly one tile, one row more, twenty tiles walked by 1, 2, 3, all or
more workgroups than there are tiles (both LDS buffers reused many times), a cloud with a single parity class (seven idle waves),
a tile whose stage needs its second pass, a tile that crosses the batch boundary, and an input that trips the range guard.

The library has no entry point for the first layer alone; every later layer reads its output, so equal features of the whole
forward are the comparison.  Each case also shows that the tile-record kernels really ran (a cloud whose records overflow would put
both settings on the probing kernel and compare it with itself): setting 0, the probing kernel, sums the same products in another
order and must differ in some bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ST_TILE, ST_UMAX, ST_UCAP2 = 256, 639, 1278


def _lib():
    from eyoc_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------- clouds (level-0 voxel coordinates; level-1 cell = coordinate >> 1)
def _children(cells, rng, p=0.3):
    """Level-0 voxels of the given level-1 cells: every child with probability p, at least one per cell."""
    out = []
    for c in cells:
        m = rng.random(8) < p
        if not m.any():
            m[rng.integers(8)] = True
        for q in np.flatnonzero(m):
            out.append((2 * c[0] + (q & 1), 2 * c[1] + ((q >> 1) & 1), 2 * c[2] + (q >> 2)))
    return np.asarray(out, np.int32)


def _ball_cells(n1, origin=(8, 8, 8)):
    """The n1 cells of a cubic grid nearest to its centre: a compact lump with exactly n1 level-1 rows."""
    s = int(np.ceil(n1 ** (1 / 3))) + 4
    g = np.stack(np.meshgrid(*[np.arange(s)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = ((g - (s - 1) / 2.0) ** 2).sum(1)
    return g[np.argsort(d, kind="stable")[:n1]] + np.asarray(origin)


def _lump(n1, seed):
    return _children(_ball_cells(n1), np.random.default_rng(seed))


def _even_only(n1):
    return (2 * _ball_cells(n1)).astype(np.int32)                    # child 0 of every cell: parity class 0 alone


def _two_planes(seed):
    """Two full 64 x 64 planes of level-1 cells at z = 31 and z = 32 (level-0 z = 62..63 | 64..65).  The two sides of z = 64 differ in
    bit 6, so inside every 64^3 block of voxels Z-order lists the lower plane's 32 x 32 cells before the upper plane's: 256-row tiles
    are 16 x 16 cells of ONE plane, and an interior tile's 3^3 neighbourhood holds 2 x 18 x 18 = 648 > 639 distinct rows."""
    xy = np.stack(np.meshgrid(np.arange(64), np.arange(64), indexing="ij"), -1).reshape(-1, 2)
    cells = np.concatenate([np.concatenate([xy, np.full((len(xy), 1), z)], 1) for z in (31, 32)])
    return _children(cells, np.random.default_rng(seed), p=0.25)


def _batched(clouds):
    from eyoc_amd import synthetic as syn
    return syn.batch_coords(clouds)


def _case(name):
    """-> (coords int32 [N,4], expected level-1 rows or None)"""
    if name == "partial-tile":
        return _batched([_lump(100, 1)]), 100
    if name == "one-tile":
        return _batched([_lump(256, 2)]), 256
    if name == "one-tile-plus-one":
        return _batched([_lump(257, 3)]), 257
    if name == "twenty-tiles":
        return _batched([_lump(20 * 256 - 57, 4)]), 20 * 256 - 57
    if name == "class-0-only":
        return _batched([_even_only(700)]), 700
    if name == "second-pass":
        return _batched([_two_planes(5)]), 2 * 64 * 64
    if name == "two-batches":
        return _batched([_lump(300, 6), _lump(330, 7)]), 630            # tile 1 holds rows of both batch indices
    raise KeyError(name)


def _feats(n, seed):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.25, 2.0, size=(n, 1)).astype(np.float32)
    f[rng.random(n) < 0.05] = 0.0
    return f


# ---------------------------------------------------------------- models and runs
_MODELS = {}


def _model(ks):
    if ks not in _MODELS:
        import eyoc_amd
        from eyoc_amd import synthetic as syn
        sd = syn.make_weights(seed=11, in_channels=1, conv1_kernel_size=ks)
        m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=ks, normalize_feature=True)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        m = m.cuda().eval()
        m.spconv_math = "split16"
        m.range_check = False                                            # the tests read the guard's words themselves
        _MODELS[ks] = m
    return _MODELS[ks]


def _run(m, coords, feats, kernel, workgroups=0):
    """One forward under the given first-convolution kernel -> (features, the guard's words {this forward, running max |x| bits, probe,
    sticky}, the coordinates of levels 0-3 in the forward's own row order)."""
    import eyoc_amd
    L, lib = _lib()
    prev_order = L.knob("eyoc_maps_internal_order", 1) - 2               # Z-ordered maps whatever the size
    prev_c1 = L.knob("eyoc_spconv_select_conv1_kernel", kernel)
    prev_wg = L.knob("eyoc_spconv_conv1_workgroups", workgroups)
    words = torch.zeros(4, dtype=torch.int32).pin_memory()
    try:
        m.probe_activations(True)                                        # (again before every forward: restarts the running maximum)
        x = eyoc_amd.SparseTensor(torch.from_numpy(feats).cuda(), coordinates=torch.from_numpy(coords).cuda())
        out = m(x).F
        m.range_snapshot(words)
        torch.cuda.synchronize()
        assert m.last_spconv_math == "split16"
        c1 = [x.coordinate_manager.level_coordinates(l, internal=True).cpu().numpy() for l in range(4)]
        assert x.coordinate_manager.row_order() is not None
        try:
            m.check_range()                                              # clears the sticky word for the next run
        except L.EyocError:
            pass
        return out.cpu().numpy(), words.numpy().copy(), c1
    finally:
        L.knob("eyoc_spconv_select_conv1_kernel", prev_c1)
        L.knob("eyoc_spconv_conv1_workgroups", prev_wg)
        L.knob("eyoc_maps_internal_order", prev_order)


def _distinct_rows_per_tile(c1, stride=2):
    """n_unique of every 256-row tile of a level (level 1: stride 2), restated on the CPU: the distinct existing cells in the 3^3
    neighbourhoods (same batch index) of the tile's rows."""
    key = lambda c: (c[:, 0].astype(np.int64) << 54) | ((c[:, 1].astype(np.int64) + (1 << 17)) << 36) | \
                    ((c[:, 2].astype(np.int64) + (1 << 17)) << 18) | (c[:, 3].astype(np.int64) + (1 << 17))
    have = np.sort(key(c1))
    offs = np.asarray([(0, stride * dx, stride * dy, stride * dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    out = []
    for t in range(0, len(c1), ST_TILE):
        k = key((c1[t:t + ST_TILE, None, :] + offs[None]).reshape(-1, 4))
        k = np.unique(k)
        pos = np.minimum(np.searchsorted(have, k), len(have) - 1)
        out.append(int((have[pos] == k).sum()))
    return out


_REF = {}


def _reference(ks, name):
    """(coords, feats, features and words under conv1_bf_kernel, distinct rows per level-1 tile): computed once per case, never changed."""
    if (ks, name) not in _REF:
        coords, n1 = _case(name)
        feats = _feats(len(coords), ks)
        m = _model(ks)
        out1, w1, cl = _run(m, coords, feats, 1)
        assert len(cl[1]) == n1, (name, len(cl[1]))
        n_u = _distinct_rows_per_tile(cl[1])
        # the tile records exist: the maps are Z-ordered (_run) and no 256-row tile of ANY level has more distinct rows than two stage
        # passes hold - one such tile takes the records of all levels away (eyoc_maps_build) ...
        for l in range(4):
            assert max(_distinct_rows_per_tile(cl[l], 1 << l)) <= ST_UCAP2, (name, l)
        # ... and the record kernels ran: the probing kernel's other summation order shows in the bits.  (One case has no other
        # order: the 3^3 window of a voxel whose coordinates are all even holds that voxel alone - a single product per output.)
        out0, _, _ = _run(m, coords, feats, 0)
        assert np.isfinite(out1).all()
        assert np.array_equal(out0, out1) == (name == "class-0-only" and ks == 3), name
        assert np.abs(out0 - out1).max() < 1e-4
        for a in (out1, w1):
            a.setflags(write=False)
        _REF[(ks, name)] = (coords, feats, out1, w1, n_u)
    return _REF[(ks, name)]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, want.view(np.uint32) if want.dtype == np.float32 else want), what


@pytest.mark.parametrize("ks", [5, 3])
@pytest.mark.parametrize("name", ["partial-tile", "one-tile", "one-tile-plus-one", "class-0-only", "two-batches"])
def test_persistent_first_convolution_is_bit_identical(ks, name):
    coords, feats, out1, w1, n_u = _reference(ks, name)
    out3, w3, _ = _run(_model(ks), coords, feats, 3)
    print(f"{name}, {ks}^3: {len(coords)} voxels, {len(n_u)} level-1 tiles, distinct rows per tile {n_u}, max |x| bits {w1[1]:#x}")
    _same(out3, out1, "features")
    _same(w3, w1, "range words")
    assert w1[0] == 0 and w1[3] == 0 and w1[1] != 0


def test_single_class_cloud_has_only_class_zero():
    """The all-even cloud: every voxel is child 0 of its cell, so waves 1-7 of the persistent kernel have no rows in any tile."""
    coords, _ = _case("class-0-only")
    assert (coords[:, 1:] % 2 == 0).all()


@pytest.mark.parametrize("ks", [5, 3])
@pytest.mark.parametrize("workgroups", [1, 2, 3, 0, 1000])
def test_twenty_tiles_under_every_grid(ks, workgroups):
    """20 level-1 tiles: one workgroup walks all 20 (both buffers ten times), two walk 10 each, three 7 / 7 / 6; 0 = one per CU and
    1000 > 20 both give every tile its own workgroup (a single tile each: the prologue and one pass of the loop)."""
    coords, feats, out1, w1, n_u = _reference(ks, "twenty-tiles")
    assert len(n_u) == 20
    out3, w3, _ = _run(_model(ks), coords, feats, 3, workgroups)
    print(f"20 tiles, {ks}^3, workgroups {workgroups}: {len(coords)} voxels, distinct rows per tile {n_u}")
    _same(out3, out1, "features")
    _same(w3, w1, "range words")


@pytest.mark.parametrize("ks", [5, 3])
@pytest.mark.parametrize("workgroups", [1, 3, 0])
def test_second_stage_pass(ks, workgroups):
    """Two adjacent planes of level-1 cells on the two sides of z = 64: tiles of one plane whose neighbourhood spans both.  The
    distinct rows of every tile are counted on the CPU from the forward's own level-1 row order: some tile has more than 639 (its
    neighbours beyond slot 638 sit in the second pass), none more than 1278 (the records exist)."""
    coords, feats, out1, w1, n_u = _reference(ks, "second-pass")
    two_pass = [u for u in n_u if u > ST_UMAX]
    print(f"second pass, {ks}^3, workgroups {workgroups}: {len(coords)} voxels, {len(n_u)} tiles, {len(two_pass)} with two passes (max {max(n_u)})")
    assert len(two_pass) >= 4 and any(u <= ST_UMAX for u in n_u)
    out3, w3, _ = _run(_model(ks), coords, feats, 3, workgroups)
    _same(out3, out1, "features")
    _same(w3, w1, "range words")


@pytest.mark.parametrize("workgroups", [1, 0])
def test_range_guard_trips_alike(workgroups):
    """One input feature beyond fp16: the first convolution's epilogue raises the forward's word and the sticky word under either
    kernel, and the NaN rows are the same rows."""
    coords, _ = _case("two-batches")
    feats = _feats(len(coords), 9)
    feats[len(feats) // 2] = 1e8
    m = _model(5)
    out1, w1, _ = _run(m, coords, feats, 1)
    out3, w3, _ = _run(m, coords, feats, 3, workgroups)
    print(f"range guard, workgroups {workgroups}: words {w1.tolist()} | {w3.tolist()}, NaN rows {int(np.isnan(out1).any(1).sum())}")
    assert w1[0] != 0 and w1[3] != 0
    _same(w3, w1, "range words")
    _same(out3, out1, "features")
    clean, wc, _ = _run(m, coords, _feats(len(coords), 9), 3, workgroups)          # the guard is per forward: the next one is clean
    assert wc[0] == 0 and wc[3] == 0 and np.isfinite(clean).all()
