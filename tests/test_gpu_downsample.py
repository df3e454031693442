"""``eyoc_voxel_downsample_batched`` against tests/downsample_restatement.py, byte for byte: the contract (include/eyoc_hip.h) fixes the
order of every operation, so the tolerance is zero for every output - xyz, attrs, first, count, inverse, seg_out, status.

The workspace promises run under the instrument of tests/workspace_contract.py through the three test bodies of
tests/test_gpu_workspace_contract.py: this module adds its case to that table with the table's own ``case`` decorator (nothing at
module level touches a GPU), as tests/test_gpu_ransac_confidence.py does.  That is also what names the new sizing function and
allocation site for the completeness test of tests/test_workspace_contract_host.py: the registration happens whenever pytest collects
the tests directory; run by its path alone, that test reports eyoc_voxel_downsample_workspace_bytes as uncovered."""
import ctypes as C

import numpy as np
import pytest
import torch

import downsample_cases as DC
import downsample_restatement as DR
import test_gpu_workspace_contract as G

pytestmark = pytest.mark.gpu

OUTPUTS = ("xyz", "attrs", "first", "count", "inverse")
DIRTY = 0x5A


def raw_call(pts, seg, voxel, attrs=None, null=(), ws_fill=None, ws_short=0, ws_skew=0, dirty_out=False):
    """The C call itself on host arrays: ``pts [n, 3 or 4]``; ``null``: outputs handed over as NULL; ``ws_fill``: the byte the
    workspace holds before the call; ``ws_short`` bytes under-reported, ``ws_skew`` bytes off the alignment (of a buffer that is really
    there); ``dirty_out``: the outputs hold ``DIRTY`` bytes before the call.  -> ``(rc, dict of numpy outputs cut to the rows written)``;
    after a refusal the dict holds the whole buffers."""
    from eyoc_amd import _lib
    lib = _lib.load()
    pts = np.ascontiguousarray(pts, np.float32)
    n, stride = pts.shape
    B = len(seg) - 1
    dev = torch.device("cuda", torch.cuda.current_device())
    p = torch.from_numpy(pts).to(dev)
    n_attr = 0 if attrs is None else attrs.shape[1]
    a = None if attrs is None else torch.from_numpy(np.ascontiguousarray(attrs, np.float32)).to(dev)

    def buf(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dev)
        if dirty_out or ws_short or ws_skew:
            t.view(torch.uint8).fill_(DIRTY)
        return t
    out = dict(xyz=buf((n, 3), torch.float32), attrs=buf((n, n_attr), torch.float32) if n_attr and "attrs" not in null else None,
               first=None if "first" in null else buf(n, torch.int32), count=None if "count" in null else buf(n, torch.int32),
               inverse=None if "inverse" in null else buf(n, torch.int32))
    status = buf(B, torch.int32) if n else torch.zeros(B, dtype=torch.int32, device=dev)
    need = lib.eyoc_voxel_downsample_workspace_bytes(n, B, n_attr)
    ws = torch.empty(max(need, 256) + 512, dtype=torch.uint8, device=dev)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    off = (-ws.data_ptr()) % 256 + ws_skew
    pt_off, vox_off = np.asarray(seg, np.int64), np.full(B + 1, -7, np.int64)
    i64 = C.POINTER(C.c_int64)
    rc = lib.eyoc_voxel_downsample_batched(_lib.ctx(dev.index), _lib.ptr(p), stride, pt_off.ctypes.data_as(i64), B, n, float(voxel),
                                           _lib.ptr(a) if "attrs" not in null else None, n_attr if "attrs" not in null else 0,
                                           _lib.ptr(out["xyz"]), _lib.ptr(out["attrs"]), _lib.ptr(out["first"]), _lib.ptr(out["count"]),
                                           _lib.ptr(out["inverse"]), _lib.ptr(status), vox_off.ctypes.data_as(i64),
                                           C.c_void_p(ws.data_ptr() + off), need - ws_short, _lib.stream_ptr())
    torch.cuda.synchronize()
    host = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    host["status"] = status.cpu().numpy()
    if rc == 0:
        m = int(vox_off[-1])
        for k in ("xyz", "attrs", "first", "count"):
            if host[k] is not None:
                host[k] = host[k][:m]
        host["seg_out"] = [int(v) for v in vox_off]
    return rc, host


def same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got != want).sum())} of {got.size} values differ"


def check(pts, seg, voxel, attrs=None, null=(), want=None, **kw):
    """One call against the restatement of the same input; NULL outputs are skipped, every other one is compared."""
    rc, got = raw_call(pts, seg, voxel, attrs, null, **kw)
    assert rc == 0
    want = DR.restate_batch(pts, seg, voxel, None if "attrs" in null else attrs) if want is None else want
    assert got["seg_out"] == want["seg_out"]
    same_bytes(got["status"], want["status"], "status")
    for k in OUTPUTS:
        if k in null or want[k] is None:
            assert got[k] is None
        else:
            same_bytes(got[k], want[k], k)
    return got, want


# ---- the smallest clouds, cell edges, far and negative coordinates
def test_one_point():
    got, _ = check(np.array([[1.5, -2.0, 3.25]], np.float32), [0, 1], 0.3)
    assert got["xyz"].tolist() == [[1.5, -2.0, 3.25]] and got["count"].tolist() == [1] and got["inverse"].tolist() == [0]


def test_two_points_in_one_voxel():
    got, _ = check(np.array([[0.0, 0.0, 0.0], [0.1, 0.05, 0.02]], np.float32), [0, 2], 0.3)
    assert got["count"].tolist() == [2] and got["first"].tolist() == [0] and got["inverse"].tolist() == [0, 0]


def test_all_points_identical():
    got, _ = check(np.tile(np.array([[3.1, -7.7, 0.3]], np.float32), (300, 1)), [0, 300], 0.3)
    assert got["count"].tolist() == [300] and got["xyz"].tolist() == [[np.float32(3.1), np.float32(-7.7), np.float32(0.3)]]


def test_cell_edges_with_exact_quotients():
    """voxel 0.25: every quotient is exact.  The minimum lands in cell 0 (quotient 0.5), a point exactly at min + voxel / 2 in cell 1
    (quotient 1.0), a hair below it in cell 0."""
    v = 0.25
    below = np.nextafter(np.float32(1.125), np.float32(0.0))
    x = np.array([1.0, 1.125, below, 1.375, 1.0 + 0.124], np.float32)      # cells 0, 1, 0, 2, 0
    pts = np.stack([x, np.full(5, -3.0, np.float32), np.full(5, 8.0, np.float32)], 1)
    got, _ = check(pts, [0, 5], v)
    assert got["inverse"].tolist() == [0, 1, 0, 2, 0] and got["first"].tolist() == [0, 1, 3] and got["count"].tolist() == [3, 1, 1]


def test_negative_coordinates():
    pts, seg = DC.random_clouds(11, [700], 2.0, (-50.0, -30.0, -120.0))
    got, _ = check(pts, seg, 0.5)
    assert (pts < 0).all() and got["count"].max() > 1


def test_cloud_ten_kilometres_out():
    pts, seg = DC.random_clouds(12, [900], 2.0, (1.0e4, -1.0e4, 7.0e3))
    got, _ = check(pts, seg, 0.5)
    assert got["count"].max() > 1 and 1 < len(got["count"]) < 900


# ---- the order of the sum
def test_sum_order_at_wave_and_workgroup_edges():
    """One voxel of 1, 63, 64, 65 and 257 points whose fp64 sum depends on the order; the restatement summed in reverse differs for at
    least one of them, so a kernel that splits the sum cannot pass by luck."""
    teeth = 0
    for n in DC.RUN_LENGTHS:
        p, a = DC.order_sensitive(n)
        got, want = check(p, [0, n], DC.HUGE_VOXEL, a)
        assert got["count"].tolist() == [n]
        rev = DR.restate_cloud(p, DC.HUGE_VOXEL, a, reverse=True)
        teeth += int(rev["xyz"].tobytes() != want["xyz"].tobytes() or rev["attrs"].tobytes() != want["attrs"].tobytes())
    assert teeth >= 1


@pytest.mark.parametrize("n", [15, 16, 17, 128, 129])
def test_sum_order_where_the_kernel_changes_its_path(n):
    """Runs of up to 16 points are summed by one lane, longer ones by a wave in chunks of 64: the lengths around both edges."""
    p, a = DC.order_sensitive(n, seed=2)
    got, _ = check(p, [0, n], DC.HUGE_VOXEL, a)
    assert got["count"].tolist() == [n]


def test_many_long_runs_in_one_wave():
    pts, seg = DC.random_clouds(14, [3000, 2000], 2.0)
    attrs = (np.random.default_rng(14).normal(size=(5000, 8)) * 10.0 ** np.arange(-3, 5)).astype(np.float32)
    got, _ = check(pts, seg, 1.5, attrs)
    assert (got["count"] > 16).sum() > 64 and got["count"].max() > 64 and (got["count"] <= 16).sum() > 64


def test_long_runs_beside_short_ones_in_a_batch():
    p0, a0 = DC.order_sensitive(257)
    p1, a1 = DC.order_sensitive(65, seed=1)
    r, seg = DC.random_clouds(13, [300])
    pts = np.concatenate([p0, r * 1.0e6, p1])              # the middle cloud: spread over a few voxels of this size
    attrs = np.concatenate([a0, np.ones((300, 3), np.float32), a1])
    got, _ = check(pts, [0, 257, 557, 622], DC.HUGE_VOXEL, attrs)
    assert got["seg_out"][1] == 1 and got["seg_out"][3] - got["seg_out"][2] == 1


# ---- sizes, empties, strides, attributes, NULL outputs
@pytest.mark.parametrize("total", [1, 255, 256, 257, 5000, 9000])     # 9000: bounds tiles (2048 points) inside one cloud and across two
def test_total_point_counts(total):
    a = total // 3
    pts, seg = DC.random_clouds(20 + total, [a, (total - a) // 2, total - a - (total - a) // 2])
    attrs = np.random.default_rng(total).normal(size=(total, 2)).astype(np.float32)
    check(pts, seg, 0.5, attrs)


@pytest.mark.parametrize("sizes", [[0, 0, 300, 200], [300, 0, 0, 200], [300, 200, 0, 0], [0, 300, 0, 200, 0], [0, 0, 0]])
def test_empty_clouds(sizes):
    pts, seg = DC.random_clouds(31, sizes)
    got, _ = check(pts, seg, 0.5)
    assert got["status"].tolist() == [0] * len(sizes)


def test_stride_4_input():
    pts, seg = DC.random_clouds(32, [400, 300])
    four = np.concatenate([pts, np.full((700, 1), np.nan, np.float32)], 1)      # the fourth float is never read
    check(four, seg, 0.5, want=DR.restate_batch(pts, seg, 0.5))


@pytest.mark.parametrize("c", [1, 3, 8])
def test_attribute_columns(c):
    pts, seg = DC.random_clouds(33 + c, [500, 1, 400])
    attrs = (np.random.default_rng(c).normal(size=(901, c)) * 10.0 ** np.arange(c)).astype(np.float32)
    got, _ = check(pts, seg, 0.6, attrs)
    assert got["attrs"].shape[1] == c


@pytest.mark.parametrize("null", [("attrs",), ("first",), ("count",), ("inverse",), ("attrs", "first", "count", "inverse")])
def test_null_outputs(null):
    pts, seg = DC.random_clouds(40, [600, 300])
    attrs = np.random.default_rng(40).normal(size=(900, 3)).astype(np.float32)
    check(pts, seg, 0.5, attrs, null=null)


def test_batch_invariance():
    cloud, _ = DC.random_clouds(50, [777], 2.0, (5.0, -2.0, 1.0))
    attrs = np.random.default_rng(50).normal(size=(777, 3)).astype(np.float32)
    rc, alone = raw_call(cloud, [0, 777], 0.5, attrs)
    assert rc == 0
    others, _ = DC.random_clouds(51, [300, 1, 450, 260], 3.0)
    o_attr = np.random.default_rng(51).normal(size=(1011, 3)).astype(np.float32)
    o_seg = [0, 300, 301, 751, 1011]
    for place in (0, 2, 4):
        parts = [others[o_seg[i]:o_seg[i + 1]] for i in range(4)]
        aparts = [o_attr[o_seg[i]:o_seg[i + 1]] for i in range(4)]
        parts.insert(place, cloud)
        aparts.insert(place, attrs)
        seg = [0] + [int(v) for v in np.cumsum([len(q) for q in parts])]
        got, _ = check(np.concatenate(parts), seg, 0.5, np.concatenate(aparts))
        rows = slice(got["seg_out"][place], got["seg_out"][place + 1])
        for k in ("xyz", "attrs", "first", "count"):
            same_bytes(got[k][rows], alone[k], f"{k} at place {place}")
        same_bytes(got["inverse"][seg[place]:seg[place + 1]], alone["inverse"], f"inverse at place {place}")


# ---- refusals of one cloud
@pytest.mark.parametrize("bad", ["nan", "inf", "extent"])
def test_a_bad_cloud_is_refused_alone(bad):
    pts, seg = DC.random_clouds(60, [400, 350, 500])
    pts = pts.copy()
    if bad == "extent":
        pts[500, 2] = pts[400:750, 2].min() + 0.5 * ((1 << 17) + 3)
    else:
        pts[500, 2] = np.nan if bad == "nan" else np.inf
    attrs = np.random.default_rng(60).normal(size=(1250, 2)).astype(np.float32)
    got, _ = check(pts, seg, 0.5, attrs, dirty_out=True)
    assert got["status"].tolist() == [0, DR.RANGE, 0] and got["seg_out"][1] == got["seg_out"][2]
    assert (got["inverse"][400:750] == -1).all()
    rc, clean = raw_call(np.concatenate([pts[:400], pts[750:]]), [0, 400, 900], 0.5, np.concatenate([attrs[:400], attrs[750:]]))
    assert rc == 0
    for k in ("xyz", "attrs", "first", "count"):
        same_bytes(got[k], clean[k], k)                     # the other clouds' rows: what they are without the bad cloud
    same_bytes(np.concatenate([got["inverse"][:400], got["inverse"][750:]]), clean["inverse"], "inverse")


def test_the_extent_limit_exactly():
    edge = np.zeros((2, 3), np.float32)
    edge[1, 0] = ((1 << 17) - 1) * 0.25
    got, _ = check(edge, [0, 2], 0.25)
    assert got["status"].tolist() == [0] and len(got["count"]) == 2
    edge[1, 0] = (1 << 17) * 0.25 - 0.125
    got, _ = check(edge, [0, 2], 0.25)
    assert got["status"].tolist() == [DR.RANGE]


# ---- workspace and stream
def _ws_input():
    pts, seg = DC.random_clouds(70, [900, 0, 1300, 400])    # crosses a scan tile (2048 flags) and a 256-thread block
    pts = pts.copy()
    pts[2300, 0] = np.nan                                  # the last cloud is refused
    attrs = np.random.default_rng(70).normal(size=(2600, 3)).astype(np.float32)
    return pts, seg, attrs


def test_dirty_workspace_and_dirty_outputs():
    pts, seg, attrs = _ws_input()
    check(pts, seg, 0.5, attrs, ws_fill=0xFF, dirty_out=True)
    check(pts, seg, 0.5, attrs, ws_fill=0x00)


@pytest.mark.parametrize("kw", [dict(ws_short=1), dict(ws_skew=128), dict(ws_skew=16)])
def test_short_or_misaligned_workspace_is_refused_and_nothing_is_written(kw):
    from eyoc_amd import _lib
    pts, seg, attrs = _ws_input()
    rc, got = raw_call(pts, seg, 0.5, attrs, ws_fill=0xFF, **kw)
    assert rc == _lib.ERR_WORKSPACE
    for k in OUTPUTS + ("status",):
        assert (got[k].view(np.uint8) == DIRTY).all(), f"{k} was written by a refused call"


@G.case("voxel_downsample", covers=["eyoc_voxel_downsample_workspace_bytes", "downsample.py:voxel_down_sample_batched"])
class _WorkspaceCase:
    def setup():
        pts, seg, attrs = _ws_input()
        return dict(pts=torch.from_numpy(pts).cuda(), host=pts, seg=seg, attrs=torch.from_numpy(attrs).cuda(), host_attrs=attrs)

    def run(s):
        import eyoc_amd
        return eyoc_amd.voxel_down_sample_batched(s["pts"], s["seg"], 0.5, s["attrs"], return_trace=True)

    def sizes(s):
        from eyoc_amd import _lib
        return [_lib.load().eyoc_voxel_downsample_workspace_bytes(2600, 4, 3)]

    def reference(s, out):
        xyz, seg_out, status, attrs, (first, count, inverse) = out
        want = DR.restate_batch(s["host"], s["seg"], 0.5, s["host_attrs"])
        assert seg_out == want["seg_out"]
        for got, k in ((xyz, "xyz"), (status, "status"), (attrs, "attrs"), (first, "first"), (count, "count"), (inverse, "inverse")):
            same_bytes(got.cpu().numpy(), want[k], k)


@pytest.mark.parametrize("promise", ["exact_under_every_fill", "short_is_refused", "misaligned_is_refused"])
def test_workspace_contract(promise):
    """Exactly the stated size under the fills 0x00, 0xFF, 0x7F and noise gives the same bytes and writes nothing outside it; one byte
    short or 16 bytes off is refused before anything runs (tests/test_gpu_workspace_contract.py's bodies on this module's case)."""
    {"exact_under_every_fill": G.test_exact_workspace_under_every_fill, "short_is_refused": G.test_short_workspace_is_refused_before_anything_runs,
     "misaligned_is_refused": G.test_misaligned_workspace_is_refused_before_anything_runs}[promise]("voxel_downsample")


def test_misaligned_workspace_through_the_wrapper_is_err_workspace():
    import workspace_contract as W
    from eyoc_amd import _lib
    s = G.CASES["voxel_downsample"].state()
    with W.Instrumented(0xFF, "misaligned") as ins:
        with pytest.raises(_lib.EyocError) as ei:
            G.CASES["voxel_downsample"].run(s)
    assert ei.value.code == _lib.ERR_WORKSPACE
    ins.check()


def test_non_default_stream():
    import eyoc_amd
    pts, seg, attrs = _ws_input()
    want = DR.restate_batch(pts, seg, 0.5, attrs)
    p, a = torch.from_numpy(pts).cuda(), torch.from_numpy(attrs).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xyz, seg_out, status, att, (first, count, inverse) = eyoc_amd.voxel_down_sample_batched(p, seg, 0.5, a, return_trace=True)
        host = [t.cpu().numpy() for t in (xyz, status, att, first, count, inverse)]
    stream.synchronize()
    assert seg_out == want["seg_out"]
    for got, k in zip(host, ("xyz", "status", "attrs", "first", "count", "inverse")):
        same_bytes(got, want[k], k)


# ---- the wrappers
def test_wrapper_shapes_and_the_single_cloud_call():
    import eyoc_amd
    from eyoc_amd import _lib
    pts, seg = DC.random_clouds(80, [500, 0, 300])
    want = DR.restate_batch(pts, seg, 0.5)
    xyz, seg_out, status = eyoc_amd.voxel_down_sample_batched(pts, seg, 0.5)
    assert seg_out == want["seg_out"] and xyz.is_cuda and status.is_cuda
    same_bytes(xyz.cpu().numpy(), want["xyz"], "xyz")
    one = eyoc_amd.voxel_down_sample(pts[:500], 0.5)
    same_bytes(one.cpu().numpy(), want["xyz"][:seg_out[1]], "one cloud")
    xyz, seg_out, status = eyoc_amd.voxel_down_sample_batched(np.zeros((0, 3), np.float32), [0, 0, 0], 0.5)
    assert xyz.shape == (0, 3) and seg_out == [0, 0, 0] and status.tolist() == [0, 0]
    bad = pts[:500].copy()
    bad[7, 1] = np.inf
    with pytest.raises(_lib.EyocError) as ei:
        eyoc_amd.voxel_down_sample(bad, 0.5)
    assert ei.value.code == _lib.ERR_RANGE
