"""The three tile-record kernel families - 256-row staged tiles (spconv_st.hip), the same kernel on 128-row tiles
(launch_spconv_st128) and class-major transposed tiles (spconv_upc.hip) - on crafted tables (tests/rulebook_cases.py) whose tiles sit
exactly at the edges geometry never lands on: U = 639 | 640 distinct input rows (one stage pass | a second pass of one row),
1278 | 1279 (last usable | refused), 2048 | 2049 (the builder's hash full | its give-up path), ragged last tiles, empty (chunk,
offset) blocks, empty classes.

Builders: the records are decoded entry by entry against the table.  Layers: integer data makes every sum exact, so whatever the pass,
chunk or summation order the output must equal an integer reference bit for bit; one real-data run per family holds the fp64 bars of
tests/test_gpu_split16.py and tests/test_gpu_upc.py.  Every layer call gets an all -1 DECOY table where the entry takes `nbr_dev`: the
record kernels never read it, a gathering kernel that took the layer instead would leave bias-only rows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rulebook_cases as rc

pytestmark = pytest.mark.gpu

K = 27
COL, PAD = 32, 64                                       # the output is columns [COL, COL + cout) of a buffer PAD floats wider


def _lib():
    from eyoc_amd import _lib as L
    return L, L.load()


@pytest.fixture(autouse=True, scope="module")
def record_kernels_selected():
    """eyoc_spconv_select_split16_kernel at its default: at 0 no record kernel is ever chosen (spconv_record_path)."""
    L, lib = _lib()
    prev = L.knob("eyoc_spconv_select_split16_kernel", 1)
    yield
    L.knob("eyoc_spconv_select_split16_kernel", prev)


class knobs:
    """Sets switches of the ctx and puts them back.  eyoc_spconv_select_down_kernel(2 / 3) sets the width of the 128-row workgroups
    and cannot be queried: it goes back to its default, 3."""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        L, _ = _lib()
        self.prev = {}
        for name, v in self.kv.items():
            p = L.knob("eyoc_spconv_" + name, v)
            self.prev[name] = 3 if name == "select_down_kernel" else p

    def __exit__(self, *exc):
        L, _ = _lib()
        for name, v in self.prev.items():
            L.knob("eyoc_spconv_" + name, v)


@functools.lru_cache(maxsize=None)
def _cases():
    by = {}
    for tile in (256, 128):
        for c in rc.edges(tile) + rc.sparse(tile) + rc.ragged(tile):
            by[c.name] = c
    for c in rc.upc_edges() + rc.upc_classes():
        by[c.name] = c
    return by


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _build_st(c, tile):
    """Records of a 256- / 128-row builder in a zeroed buffer: (device bytes, overflow)."""
    L, lib = _lib()
    nd = _dev(c.nbr)
    local = torch.zeros(int(lib.eyoc_spconv_local_rulebook_bytes(c.n_out * (256 // tile))), dtype=torch.uint8, device="cuda")
    ovf = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    build = lib.eyoc_spconv_build_local_rulebook if tile == 256 else lib.eyoc_spconv_build_local_rulebook128
    L.check(build(L.ctx(), L.ptr(nd), K, c.n_out, L.ptr(local), L.ptr(ovf), L.stream_ptr()))
    torch.cuda.synchronize()
    return local, int(ovf.item())


def _build_upc(c):
    """Workspace of the class-major builder: (device bytes, aligned address, host bytes from there, info[19])."""
    L, lib = _lib()
    nd = _dev(c.nbr)
    ws = torch.zeros(int(lib.eyoc_spconv_upc_bytes(c.n_out)) + 256, dtype=torch.uint8, device="cuda")
    al = (ws.data_ptr() + 255) & ~255
    info = np.zeros(19, np.int32)
    L.check(lib.eyoc_spconv_upc_build(L.ctx(), L.ptr(nd), c.n_out, C.c_void_p(al), info.ctypes.data, L.stream_ptr()))
    torch.cuda.synchronize()
    return ws, al, ws.cpu().numpy()[al - ws.data_ptr():], info


def _upc_kept(raw, n, n_tiles):
    max_tiles = (n + 127) // 128 + 8
    return raw[:rc.UPC_HDR + (max_tiles * 4 + 255) // 256 * 256 + n_tiles * rc.UPC_LR]


@functools.lru_cache(maxsize=None)
def _records(family, name):
    """The device builder's records of a case, checked, for the layer tests: (keep-alive tensors, pointer, n_unique per tile)."""
    c = _cases()[name]
    if family == "upc":
        ws, al, raw, info = _build_upc(c)
        over, tiles = rc.check_upc_workspace(raw, c.nbr)
        assert over == 0 and [u for _, u in tiles] == c.U
        return ws, C.c_void_p(al), c.U
    tile = int(family)
    local, ovf = _build_st(c, tile)
    assert ovf == 0 and rc.check_st_records(local.cpu().numpy(), c.nbr, tile) == c.U
    return local, C.c_void_p(local.data_ptr()), c.U


# ------------------------------------------------------------------------------------------------------------------- builders
ST_SETS = {"edges": rc.edges, "sparse": rc.sparse, "ragged": rc.ragged}


@pytest.mark.parametrize("which", list(ST_SETS))
@pytest.mark.parametrize("tile", [256, 128])
def test_builder_records_decode_to_the_table(tile, which):
    """Every entry of every record names its table entry through U, in exactly one pass; masks, row map and inverse map hold; n_unique
    is the crafted U; with and without row grouping."""
    for c in ST_SETS[which](tile):
        for group in (1, 0):
            with knobs(st_group_rows=group):
                local, ovf = _build_st(c, tile)
            raw = local.cpu().numpy()
            n_u = rc.check_st_records(raw, c.nbr, tile)
            assert ovf == 0 and n_u == c.U, (c.name, group, n_u)
            if group == 0:                                                   # rows in their own order
                n_tiles = (c.n_out + tile - 1) // tile
                rm = raw[:n_tiles * rc.ST_LR].reshape(n_tiles, rc.ST_LR)[:, rc.ST_RM_OFF:rc.ST_RM_OFF + 256]
                rm = rm.reshape(n_tiles, 4, 16, 4).transpose(0, 1, 3, 2).reshape(n_tiles, 256)[:, :tile]
                assert (rm == np.arange(tile)).all()
        print(f"{tile}-row builder, {c.name}: n_unique per tile {n_u}")


@pytest.mark.parametrize("tile", [256, 128])
def test_builder_refuses_tiles_above_two_passes(tile):
    """U = 1279 (one row too many; the hash 62 % full), 2047 and 2048 (the hash nearly and exactly full: the canonical numbering walks
    one probe cluster of the whole table), 2049 and all-distinct (the hash gives up): the builder returns, counts the tile and marks
    exactly that one with n_unique = -1; its neighbours build as usual."""
    for c, over in rc.overflow(tile):
        for group in (1, 0):
            with knobs(st_group_rows=group):
                local, ovf = _build_st(c, tile)
            n_u = rc.check_st_records(local.cpu().numpy(), c.nbr, tile)
            assert ovf == over == sum(u > 1278 for u in c.U), (c.name, ovf)
            assert n_u == [u if u <= 1278 else -1 for u in c.U], (c.name, n_u)
        print(f"{tile}-row builder, {c.name}: U per tile {c.U} -> n_unique {n_u}, overflow count {ovf}")


def test_class_major_builder_partition_records_and_overflow():
    """Counts, tile_start, every row in exactly one slot of a tile of its class, the launch order a permutation, every record decoded -
    with empty classes, a class ending on a tile edge and one row behind it, n = 1; tiles above 1278 counted in info[18]."""
    for c, over in [(c, 0) for c in rc.upc_edges() + rc.upc_classes()] + rc.upc_overflow():
        ws, al, raw, info = _build_upc(c)
        overflow, tiles = rc.check_upc_workspace(raw, c.nbr)
        assert int(info[18]) == overflow == over and int(info[0]) == len(c.U)
        assert tiles == [(b, u if u <= 1278 else -1) for b, u in zip(c.tile_class, c.U)], (c.name, tiles)
        print(f"class-major builder, {c.name}: n {c.n_out} counts {info[10:18].tolist()} (class, n_unique) per tile {tiles}, overflow count {overflow}")


# ------------------------------------------------------------------------------------------------------------- layers, exact
@functools.lru_cache(maxsize=2)
def _exact_problem(name, cin, cout):
    """Integer layer on a case: x in 0..3, W in -1..1, |bias|, |res| <= 8.  Every product and partial sum is an integer below
    27 * 256 * 3 * 2^8 < 2^24 times the power-of-two weight scale: exact in the fp16 halves, in the fp32 accumulators and in the split16
    store (|out| <= 27 * 256 * 3 + 16 < 6e4).  The sums in float64 (exact, and BLAS), kept as int64."""
    L, lib = _lib()
    c = _cases()[name]
    rng = np.random.default_rng(cin * 1000 + cout + len(name))
    x = rng.integers(0, 4, (c.n_in, cin)).astype(np.float32)
    W = rng.integers(-1, 2, (K, cin, cout)).astype(np.float32)
    bias = rng.integers(-8, 9, cout).astype(np.float32)
    res = rng.integers(-8, 9, (c.n_out, cout)).astype(np.float32)
    acc = np.zeros((c.n_out, cout))
    for k in range(K):
        v = c.nbr[k] >= 0
        acc[v] += x[c.nbr[k][v]].astype(np.float64) @ W[k].astype(np.float64)
    pre = acc.astype(np.int64)
    assert (pre == acc).all() and np.abs(pre).max() <= K * cin * 3
    packed, osc = np.zeros(W.size, np.float32), np.zeros(1, np.float32)
    assert lib.eyoc_spconv_pack_weights_split16(W.ctypes.data, None, K, cin, cout, packed.ctypes.data, osc.ctypes.data) == 0
    assert osc[0] > 0 and np.frexp(osc[0])[0] == 0.5, f"out_scale {osc[0]} is no power of two"
    xd, rd = _dev(x), _dev(res)
    xs, rs = torch.empty_like(xd), torch.empty_like(rd)
    L.check(lib.eyoc_split16_encode(L.ctx(), L.ptr(xd), c.n_in, cin, cin, L.ptr(xs), cin, L.stream_ptr()))
    L.check(lib.eyoc_split16_encode(L.ctx(), L.ptr(rd), c.n_out, cout, cout, L.ptr(rs), cout, L.stream_ptr()))
    torch.cuda.synchronize()
    dev = SimpleDev(xs=xs, rs=rs, wd=_dev(packed), osd=_dev(osc), bd=_dev(bias), decoy=torch.full((K, c.n_out), -1, dtype=torch.int32, device="cuda"))
    return pre, bias.astype(np.int64), res.astype(np.int64), dev


class SimpleDev:
    def __init__(self, **kv):
        self.__dict__.update(kv)


def _run(family, c, rec_ptr, d, cin, cout, use_res, relu, out_split, nbr_dev=None):
    """One layer into columns [COL, COL + cout) of a NaN-filled buffer; returns the slice as fp32 (decoded) after checking that nothing
    else was written and no NaN is left inside."""
    L, lib = _lib()
    ld = cout + PAD
    out = torch.full((c.n_out, ld), float("nan"), device="cuda")
    op = C.c_void_p(out.data_ptr() + 4 * COL)
    nbr = L.ptr(d.decoy if nbr_dev is None else nbr_dev)
    if family == "upc":
        assert not use_res
        L.check(lib.eyoc_spconv_upc(L.ctx(), nbr, rec_ptr, c.n_out, c.n_in, L.ptr(d.xs), cin, cin, L.ptr(d.wd), cout, L.ptr(d.bd), relu, op, ld,
                                    out_split, L.ptr(d.osd), L.stream_ptr()), "eyoc_spconv_upc")
    else:
        fn = lib.eyoc_spconv_staged if family == "256" else lib.eyoc_spconv_staged128
        L.check(fn(L.ctx(), nbr, rec_ptr, c.n_out, c.n_in, L.ptr(d.xs), cin, cin, L.ptr(d.wd), cout, L.ptr(d.bd), L.ptr(d.rs) if use_res else None,
                   cout if use_res else 0, relu, op, ld, out_split, L.ptr(d.osd), L.stream_ptr()), "eyoc_spconv_staged" + family)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:, :COL]).all()) and bool(torch.isnan(out[:, COL + cout:]).all()), "columns outside the layer were written"
    got = out[:, COL:COL + cout].contiguous()
    assert not bool(torch.isnan(got).any()), "a NaN is left inside the layer's columns"
    if out_split:
        dec = torch.empty_like(got)
        L.check(lib.eyoc_split16_decode(L.ctx(), L.ptr(got), c.n_out, cout, cout, L.ptr(dec), cout, L.stream_ptr()))
        torch.cuda.synchronize()
        got = dec
    return got.cpu().numpy()


def _exact_layer(family, name, cin, cout, settings):
    c = _cases()[name]
    keep, rec_ptr, n_u = _records(family, name)
    pre, bias, res, d = _exact_problem(name, cin, cout)
    runs = 0
    for kn in settings:
        with knobs(**kn):
            for use_res in ((0, 1) if family != "upc" else (0,)):
                for relu in (0, 1):
                    want = pre + bias[None] + (res if use_res else 0)
                    want = (np.maximum(want, 0) if relu else want).astype(np.float32)
                    for out_split in (0, 1):
                        got = _run(family, c, rec_ptr, d, cin, cout, use_res, relu, out_split)
                        bad = got != want
                        assert not bad.any(), (f"{family} {name} {cin}->{cout} {kn} res {use_res} relu {relu} split-out {out_split}: {int(bad.sum())} "
                                               f"entries differ, first rows {np.unique(np.nonzero(bad)[0])[:8].tolist()}")
                        runs += 1
    print(f"{family}-family layer {cin}->{cout} on {name}: {runs} runs equal the integer reference bit for bit; n_unique per tile {n_u}")


ST256_TABLES = ["edges256", "sparse256", "ragged256-0x256+15", "ragged256-7x256+255", "ragged256-8x256+1", "ragged256-8x256+65"]
ST128_TABLES = ["edges128", "sparse128", "ragged128-0x128+17", "ragged128-7x128+64", "ragged128-8x128+1", "ragged128-8x128+63"]
UPC_TABLES = ["upc_edges", "upc_only0", "upc_only7", "upc_R_and_R+1", "upc_n1", "upc_n100"]


@pytest.mark.parametrize("name", ST256_TABLES)
@pytest.mark.parametrize("cin,cout", [(32, 32), (32, 64), (64, 64), (128, 128), (256, 256)])
def test_staged_256_row_layer_is_exact(cin, cout, name):
    """32- and 64-channel workgroups (eyoc_spconv_st_split_below at its default: tables this small take the narrow ones; 0: the wide
    ones), the C++ loop, the assembly loop and the one without empty-block branches."""
    L, _ = _lib()
    default = L.knob("eyoc_spconv_st_split_below", -1)
    _exact_layer("256", name, cin, cout, [dict(st_split_below=s, select_st_kernel=v) for s in (default, 0) for v in (0, 1, 2)])


@pytest.mark.parametrize("name", ST128_TABLES)
@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 128), (256, 256)])
def test_staged_128_row_layer_is_exact(cin, cout, name):
    """64- and 128-channel workgroups (eyoc_spconv_select_down_kernel 2 / 3), the four 64-row-wave loops (variants 1, 4, 5, 6)."""
    _exact_layer("128", name, cin, cout, [dict(select_down_kernel=w, select_st_kernel=v) for w in (2, 3) for v in (1, 4, 5, 6)])


@pytest.mark.parametrize("name", UPC_TABLES)
@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 64), (256, 128), (32, 128)])
def test_class_major_layer_is_exact(cin, cout, name):
    _exact_layer("upc", name, cin, cout, [dict()])


# --------------------------------------------------------------------------------------------------------- layers, real data
@pytest.mark.parametrize("family,name,cin,cout", [("256", "edges256", 64, 64), ("128", "edges128", 64, 128), ("upc", "upc_edges", 128, 64)])
def test_layer_on_real_data_holds_the_fp64_bars(family, name, cin, cout):
    """|N(0,1)| inputs, N / sqrt(9 cin) weights against the fp64 restatement: below 2e-6 of the largest output (the bar of
    test_staged_kernel_vs_fp64), no worse than 3 x the gathering kernel's error + 2e-7 (the rule of tests/test_gpu_upc.py; eyoc_spconv_ex
    with math = 1 on the same table), and the same bytes in a second run - tiles that stage in two passes included."""
    from test_gpu_split16 import layer_f64
    L, lib = _lib()
    c = _cases()[name]
    keep, rec_ptr, n_u = _records(family, name)
    assert {639, 640, 1278} <= set(n_u)
    rng = np.random.default_rng(cin + cout)
    x = np.abs(rng.normal(size=(c.n_in, cin))).astype(np.float32)
    W = (rng.normal(size=(K, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    bias = rng.normal(size=cout).astype(np.float32)
    res = rng.normal(size=(c.n_out, cout)).astype(np.float32)
    use_res = family != "upc"
    want = layer_f64(c.nbr, x, W, bias=bias, res=res if use_res else None, relu=True)
    scale = np.abs(want).max()
    packed, osc = np.zeros(W.size, np.float32), np.zeros(1, np.float32)
    assert lib.eyoc_spconv_pack_weights_split16(W.ctypes.data, None, K, cin, cout, packed.ctypes.data, osc.ctypes.data) == 0
    xd, rd = _dev(x), _dev(res)
    xs, rs = torch.empty_like(xd), torch.empty_like(rd)
    L.check(lib.eyoc_split16_encode(L.ctx(), L.ptr(xd), c.n_in, cin, cin, L.ptr(xs), cin, L.stream_ptr()))
    L.check(lib.eyoc_split16_encode(L.ctx(), L.ptr(rd), c.n_out, cout, cout, L.ptr(rs), cout, L.stream_ptr()))
    d = SimpleDev(xs=xs, rs=rs, wd=_dev(packed), osd=_dev(osc), bd=_dev(bias), decoy=torch.full((K, c.n_out), -1, dtype=torch.int32, device="cuda"))
    nd = _dev(c.nbr)
    for out_split in (0, 1):
        got = _run(family, c, rec_ptr, d, cin, cout, use_res, 1, out_split)
        again = _run(family, c, rec_ptr, d, cin, cout, use_res, 1, out_split)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two runs differ"
        # the device reference: a gathering kernel on the real table
        ld = cout + PAD
        gat = torch.full((c.n_out, ld), float("nan"), device="cuda")
        L.check(lib.eyoc_spconv_ex(L.ctx(), L.ptr(nd), K, c.n_out, c.n_in, L.ptr(xs), cin, cin, L.ptr(d.wd), cout, L.ptr(d.bd), L.ptr(rs) if use_res else None,
                                   cout if use_res else 0, 1, C.c_void_p(gat.data_ptr() + 4 * COL), ld, 1, out_split, L.ptr(d.osd), L.stream_ptr()))
        g = gat[:, COL:COL + cout].contiguous()
        if out_split:
            dec = torch.empty_like(g)
            L.check(lib.eyoc_split16_decode(L.ctx(), L.ptr(g), c.n_out, cout, cout, L.ptr(dec), cout, L.stream_ptr()))
            g = dec
        torch.cuda.synchronize()
        e = float(np.abs(got - want).max() / scale)
        eg = float(np.abs(g.cpu().numpy() - want).max() / scale)
        print(f"{family}-family {cin}->{cout} on {name}, split-out {out_split}: record kernel {e:.2e}, gathering kernel {eg:.2e} of the largest output; "
              f"n_unique per tile {n_u}")
        assert e < 2e-6 and e <= 3 * eg + 2e-7


# ------------------------------------------------------------------------------------------------- two builds, the same bytes
def _st_regions(tile_no, a, b):
    names = [("n_unique", 0, 16), ("U", rc.ST_U_OFF, rc.ST_LOC_OFF), ("loc", rc.ST_LOC_OFF, rc.ST_MASK_OFF), ("masks", rc.ST_MASK_OFF, rc.ST_RM_OFF),
             ("row map", rc.ST_RM_OFF, rc.ST_INV_OFF), ("inv", rc.ST_INV_OFF, rc.ST_LR)]
    return [f"tile {tile_no}: {n}" for n, lo, hi in names if not np.array_equal(a[lo:hi], b[lo:hi])]


@pytest.mark.parametrize("tile", [256, 128])
def test_second_build_gives_the_same_bytes(tile):
    """The records of two builds of one table into zeroed buffers are the same bytes, one-pass tiles included: the builder's hash keeps
    the larger key in a slot and carries the smaller one on (ordered linear probing), so the same keys end in the same slots whatever
    order its atomics ran in.  (With a compare-and-swap for empty slots only, `U` and `loc` of one-pass tiles - U = 638, 639 here -
    changed from build to build; two-pass tiles were already numbered canonically.)"""
    for c in rc.edges(tile) + rc.sparse(tile) + rc.ragged(tile):
        for group in (1, 0):
            with knobs(st_group_rows=group):
                a, b = (_build_st(c, tile)[0].cpu().numpy()[:len(c.U) * rc.ST_LR].reshape(-1, rc.ST_LR) for _ in range(2))
            diff = [d for t in range(len(c.U)) for d in _st_regions(t, a[t], b[t])]
            assert not diff, f"{c.name} (U per tile {c.U}), grouping {group}: two builds differ in {diff}"


def test_second_class_major_build_gives_the_same_bytes():
    """As above for the class-major workspace: header, launch order and records (before: the record of upc_edges' tile 1, class 1,
    U = 200, differed between two builds)."""
    for c in rc.upc_edges() + rc.upc_classes():
        raw, raw2 = _build_upc(c)[2], _build_upc(c)[2]
        a, b = _upc_kept(raw, c.n_out, len(c.U)), _upc_kept(raw2, c.n_out, len(c.U))
        rec0 = len(a) - len(c.U) * rc.UPC_LR
        diff = [] if np.array_equal(a[:rec0], b[:rec0]) else ["header or launch order"]
        diff += [f"tile {t} (class {c.tile_class[t]}, U {c.U[t]})" for t in range(len(c.U))
                 if not np.array_equal(a[rec0 + t * rc.UPC_LR:rec0 + (t + 1) * rc.UPC_LR], b[rec0 + t * rc.UPC_LR:rec0 + (t + 1) * rc.UPC_LR])]
        assert not diff, f"{c.name}: two builds differ in {diff}"
