"""GPU parity of the plain voxeliser (eyoc_voxelize, eyoc_voxelize_batched, eyoc_voxelize_batched_isolating) with its restatement
(tests/voxelize_restatement.py) on the inputs of tests/voxelize_cases.py: cell borders, the ends of the key range, the smallest
magnitudes, non-finite points, runs of equal keys against the wave and the workgroup, cloud boundaries, probing chains that wrap.
Integer work and copies: every comparison is byte for byte."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import voxelize_cases as cases
import voxelize_restatement as V

pytestmark = pytest.mark.gpu

F32 = np.float32


def _host(out):
    return [o.cpu().numpy() if isinstance(o, torch.Tensor) else o for o in out]


def _same(got, want, what):
    names = ("coords", "sel", "xyz", "offsets", "faults")
    dtypes = (np.int32, np.int64, np.float32, np.int64, np.int32)
    for g, w, name, dt in zip(got, want, names, dtypes):
        assert g.dtype == dt and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {name}"


def single(cloud, voxel, batch=0):
    import eyoc_amd
    cloud = np.asarray(cloud, F32)
    coords, sel = _host(eyoc_amd.sparse_quantize(cloud, voxel, batch))
    return coords, sel, cloud[sel][:, :3], np.asarray([0, len(sel)], np.int64)


def batched(clouds, voxel, base=0, isolate=False):
    import eyoc_amd
    return _host(eyoc_amd.sparse_quantize_batch(clouds, voxel, base, isolate=isolate))


def raw4(clouds, voxel, base=0):
    """One ``eyoc_voxelize_batched`` call on rows of four floats whose fourth is NaN throughout."""
    from eyoc_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", torch.cuda.current_device())
    off = np.zeros(len(clouds) + 1, np.int64)
    np.cumsum([len(c) for c in clouds], out=off[1:])
    n, B = int(off[-1]), len(clouds)
    rows = np.full((max(n, 1), 4), np.nan, F32)
    if n:
        rows[:n, :3] = np.concatenate([np.asarray(c, F32)[:, :3] for c in clouds])
    packed = torch.from_numpy(rows).to(dev)
    sel = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    coords = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
    xyz = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    vox = np.zeros(B + 1, np.int64)
    i64 = C.POINTER(C.c_int64)
    ws = _lib.workspace(lib.eyoc_voxelize_batched_workspace_bytes(n, B), dev)
    _lib.check(lib.eyoc_voxelize_batched(_lib.ctx(dev.index), _lib.ptr(packed), 4, off.ctypes.data_as(i64), B, n, float(voxel), int(base),
                                         _lib.ptr(sel), _lib.ptr(coords), _lib.ptr(xyz), vox.ctypes.data_as(i64), _lib.ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), "eyoc_voxelize_batched")
    m = int(vox[-1])
    return _host((coords[:m], sel[:m].long(), xyz[:m], vox))


def check_all(clouds, voxel, base=0, what="", singles=True):
    """Every entry point against the restatement -> the restatement's answer."""
    want = V.quantize(clouds, voxel, base)
    assert not want[4].any()
    _same(batched(clouds, voxel, base), want, f"{what}: sparse_quantize_batch")
    _same(batched(clouds, voxel, base, isolate=True), want, f"{what}: sparse_quantize_batch(isolate=True)")
    _same(raw4(clouds, voxel, base), want, f"{what}: eyoc_voxelize_batched, stride 4")
    if singles:
        off = want[3]
        for b, c in enumerate(clouds):
            if len(c):
                mine = tuple(a[off[b]:off[b + 1]] for a in want[:3]) + (np.asarray([0, off[b + 1] - off[b]], np.int64),)
                _same(single(c, voxel, base + b), mine, f"{what}: sparse_quantize of cloud {b}")
    return want


def refused(clouds, voxel, first, what=""):
    """The plain calls fail with EYOC_ERR_RANGE and name the first faulty cloud."""
    from eyoc_amd import _lib
    for call in (batched, raw4):
        with pytest.raises(_lib.EyocError) as e:
            call(clouds, voxel)
        assert e.value.code == _lib.ERR_RANGE, what
        if len(clouds) > 1:
            assert re.search(rf"cloud {first}\b", str(e.value)), (what, str(e.value))
    if len(clouds) == 1:
        with pytest.raises(_lib.EyocError) as e:
            single(clouds[0], voxel)
        assert e.value.code == _lib.ERR_RANGE, what


def isolated(clouds, voxel, base=0, what=""):
    """The isolating call against the restatement; the live clouds' rows are those of the plain call without the faulty clouds."""
    want = V.quantize(clouds, voxel, base, isolate=True)
    got = batched(clouds, voxel, base, isolate=True)
    _same(got, want, f"{what}: isolating")
    live = [c if not want[4][b].any() else np.zeros((0, 3), F32) for b, c in enumerate(clouds)]
    if sum(map(len, live)):
        _same(batched(live, voxel, base), got[:4], f"{what}: the plain call without the faulty clouds")
    else:
        assert got[0].shape == (0, 4) and not got[3].any()
    return got


# ---- 1. borders
@pytest.mark.parametrize("voxel", cases.VOXELS)
def test_borders(voxel):
    inside, _ = cases.border_split(voxel)
    check_all([np.concatenate(inside)], voxel, what=f"borders at {voxel}, one cloud")
    check_all(inside, voxel, base=5, what=f"borders at {voxel}, three clouds", singles=False)


def test_hand_written_answers():
    clouds, coords, sel, xyz, offsets = cases.hand_points()
    want = check_all(clouds, cases.HAND_VOXEL, what="by hand")
    _same(want[:4], (coords, sel, xyz, offsets), "the restatement itself")


@pytest.mark.parametrize("voxel", cases.VOXELS)
def test_small_magnitudes(voxel):
    pts, cells = cases.small_magnitudes(voxel)
    want = check_all([pts], voxel, what=f"small magnitudes at {voxel}")
    assert want[0][:, 1:].tolist() == cells[want[1]].tolist()
    assert want[1].tolist() == [0, 1, 5, 6, 10, 11]          # per axis -0.0 (cell 0) and the subnormal (cell -1) are kept: first of their cells


# ---- 2. the range's edge
@pytest.mark.parametrize("voxel", cases.EDGE_VOXELS)
def test_range_edge(voxel):
    edge = cases.range_edge(voxel)
    good = np.concatenate([pts for _, _, accepted, pts in edge if accepted])
    bad = np.concatenate([pts for _, _, accepted, pts in edge if not accepted])
    assert len(good) >= 6 and len(bad) >= 6
    want = check_all([good], voxel, what=f"accepted edge cells at {voxel}")
    assert set(np.unique(want[0][:, 1:])) >= {-V.LIM, V.LIM - 1}
    for p in bad:
        refused([p[None]], voxel, 0, f"{p} at {voxel}")
    clouds = [good, bad[:1], good[:3], np.zeros((0, 3), F32), bad[1:], good]
    refused(clouds, voxel, 1, f"edge batch at {voxel}")
    refused(clouds[2:], voxel, 2, f"edge batch at {voxel}, later")
    got = isolated(clouds, voxel, what=f"edge batch at {voxel}")
    assert got[4].tolist() == [[0, 0], [1, 0], [0, 0], [0, 0], [len(bad) - 1, 0], [0, 0]]
    check_all([good], voxel, what="the context afterwards", singles=False)


@pytest.mark.parametrize("voxel", cases.VOXELS)
def test_refused_border_points(voxel):
    """Every refused point of the border set as a cloud of its own: one count each; a few of them alone."""
    _, outside = cases.border_split(voxel)
    clouds = [p[None] for p in outside]
    got = isolated(clouds, voxel, what=f"refused border points at {voxel}")
    assert got[4].tolist() == [[1, 0]] * len(clouds)
    refused(clouds, voxel, 0)
    for p in outside[:: max(1, len(outside) // 6)]:
        refused([p[None]], voxel, 0, f"{p} at {voxel}")


# ---- 3. non-finite points
def test_non_finite_points_are_refused():
    voxel = 0.3
    inside, _ = cases.border_split(voxel)
    body = inside[1][:300]
    for p, counts in cases.nonfinite_points(voxel):
        refused([p[None]], voxel, 0, f"{p} alone")
        cloud = np.concatenate([body[:130], p[None], body[130:]])
        refused([cloud], voxel, 0, f"{p} in a cloud")
        refused([body, np.zeros((0, 3), F32), cloud, body], voxel, 2, f"{p} in cloud 2")
        got = isolated([body, cloud, p[None], body], voxel, what=f"{p}")
        assert got[4].tolist() == [[0, 0], list(counts), list(counts), [0, 0]], p
    check_all([body, body], voxel, what="the context afterwards")


def test_fourth_column_is_never_read():
    import eyoc_amd
    voxel = 0.3
    inside, _ = cases.border_split(voxel)
    clean, dirty = cases.fourth_column(inside[2][:3000])
    want = V.quantize([clean], voxel)
    _same(want, V.quantize([dirty], voxel), "restatement")
    for rows in (clean, dirty):
        _same(single(rows, voxel), want, "sparse_quantize")
        _same(batched([rows, rows[:100]], voxel), V.quantize([rows, rows[:100]], voxel), "sparse_quantize_batch")
        _same(batched([rows, rows[:100]], voxel, isolate=True), V.quantize([rows, rows[:100]], voxel), "isolating")
    a, b = (eyoc_amd.sparse_quantize(torch.from_numpy(r).cuda(), voxel, 2) for r in (clean, dirty))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. run patterns, cloud boundaries, wrap-around
@pytest.mark.parametrize("n", cases.RUN_LENGTHS)
def test_run_patterns(n):
    mine = [p for p in cases.run_patterns() if len(p[2]) == n]
    assert len(mine) >= 7
    for name, _, pts in mine:
        want = check_all([pts], cases.RUN_VOXEL, what=name)
        _same(single(pts, cases.RUN_VOXEL), want, f"{name}: again")
        _same(batched([pts], cases.RUN_VOXEL), want, f"{name}: again")
    clouds = [p[2] for p in mine]                             # ... and all of them as one batch: the runs at other lanes
    want = check_all(clouds, cases.RUN_VOXEL, base=1, what=f"all patterns of {n} points", singles=False)
    _same(batched(clouds, cases.RUN_VOXEL, 1), want, "again")


def test_cloud_boundaries():
    clouds = cases.boundary_batch()
    want = check_all(clouds, cases.RUN_VOXEL, what="boundaries")
    _same(batched(clouds, cases.RUN_VOXEL), want, "boundaries: again")
    _same(batched(clouds, cases.RUN_VOXEL, isolate=True), want, "boundaries: again, isolating")
    check_all(clouds, cases.RUN_VOXEL, base=1024 - len(clouds), what="boundaries at the last batch indices", singles=False)


def test_faulty_clouds_at_the_boundaries():
    for name, clouds, faulty in cases.isolating_batches():
        got = isolated(clouds, cases.RUN_VOXEL, base=3, what=name)
        assert [b for b in range(len(clouds)) if got[4][b].any()] == list(faulty), name
        _same(batched(clouds, cases.RUN_VOXEL, 3, isolate=True), got, f"{name}: again")
        refused(clouds, cases.RUN_VOXEL, faulty[0], name)
    assert got[0].shape == (0, 4)                             # the last one: every cloud faulty


def test_probing_chains_that_wrap():
    cells, pts = cases.wrap_cloud()
    want = check_all([pts], cases.RUN_VOXEL, what="wrap-around")
    assert want[0][:, 1:].tolist() == cases.wrap_cells().tolist() and want[1].tolist() == list(range(40))
    _same(single(pts, cases.RUN_VOXEL), want, "wrap-around: again")
    _same(batched([pts], cases.RUN_VOXEL), want, "wrap-around: again")


def test_wrapping_cells_in_the_map_build():
    from eyoc_amd import _lib
    from test_gpu_maps import check_against_oracle
    coords = np.concatenate([np.zeros((40, 1), np.int64), cases.wrap_cells()], 1).astype(np.int32)
    _lib.load()
    prev = _lib.knob("eyoc_maps_order_min_rows", 0)          # (test_gpu_maps.order_small_levels)
    try:
        check_against_oracle(coords)
    finally:
        _lib.knob("eyoc_maps_order_min_rows", prev)


# ---- 5. the posed route keeps its own rule
def test_posed_route_and_plain_route_keep_their_own_rules():
    """Identity pose, no scale, the 0.3 border values with every point in a voxel of its own, so that both routes return every point's
    cell: the posed route divides in fp64 by the fp64 voxel size, the plain one in fp32 by the fp32 one.  Each equals its restatement,
    and their cells differ a thousand times over - neither has silently taken the other's rule."""
    import trainbatch_restatement as R
    from eyoc_amd import trainbatch as tb
    voxel = 0.3
    cloud = cases.border_cloud_apart(voxel)
    cell = np.floor(cloud.astype(np.float64) / np.float64(voxel))
    inside = ((cell >= -V.LIM) & (cell < V.LIM)).all(1) & ~V.classify(cloud, voxel)[1]      # accepted under both rules
    assert len(cloud) - 30 < inside.sum() < len(cloud)
    cloud = cloud[inside]
    dev = torch.device("cuda", torch.cuda.current_device())
    pose = torch.eye(4, dtype=torch.float64, device=dev)[None].contiguous()
    posed = _host(tb.voxelize_posed(torch.from_numpy(cloud).to(dev), np.asarray([0, len(cloud)], np.int64), pose, None, voxel))
    _same(posed, R.quantize_posed([cloud], [np.eye(4)], None, voxel)[:4], "posed route")
    plain = single(cloud, voxel)
    _same(plain, V.quantize([cloud], voxel), "plain route")
    everyone = np.arange(len(cloud)).tolist()
    assert plain[1].tolist() == everyone and posed[1].tolist() == everyone
    differ = int((plain[0] != posed[0]).any(1).sum())
    print(f"{len(cloud)} points, the two routes' cells differ on {differ}")
    assert differ >= 1000
