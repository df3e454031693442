"""The instance-norm kernels alone (csrc/inorm.hip: ``eyoc_in_plan_build``, ``eyoc_in_forward``, ``eyoc_in_backward``), through the raw
C ABI, against the float64 restatement of tests/inorm_restatement.py.

Bars: those of ``bn_check`` (tests/test_gpu_train_kernels.py), applied per instance with n -> n_b and eps = 1e-8 - the per-element
arithmetic of the kernels is the same, so the derivation carries over.  u = 2^-24; everything on the right from the float64
restatement (invstd = 1 / sqrt(var + eps), xhat = (x - mean) invstd, per instance):

forward   |y - y64| <= 8u (|xhat weight| + |bias|) + 2u |mean| invstd |weight|  [+ u |y64| with a residual: y = fl(a + res) is one more
          rounding].  mean and var of every instance within 1 ulp of the float64 value rounded to fp32.  ReLU decisions may differ only
          where |y64| <= that bound.
xhat      e_xhat = 6u |xhat| + 2u |mean| invstd
sums      per instance (n_b rows) and over all rows (n rows; dbias, dweight):  E_b = u |sum g| + rows 2^-53 sum |g|,
          E_g = sum |g| e_xhat + u |sum g xhat| + rows 2^-53 sum |g xhat|
dx        E_B = E_b / n_b + 2u |sb| / n_b + (e_xhat |sg| + |xhat| E_g) / n_b + 3u |xhat sg| / n_b + u (|g| + |sb| / n_b) + u |B|,
          E_dx = |weight| invstd E_B + 6u |dx|     (sb = sum_b g, sg = sum_b g xhat, B the bracket)
dres      = g exactly.
The backward restatement is given the GPU's own y for the ReLU mask (the forward's decisions are checked above).  No tolerance in this
file comes from the code under test.

Shapes: c in {32, 64, 128, 256}; instance sizes from {0, 1, 2, R-1, R, R+1, 3R+1} (R = ``eyoc_in_chunk_rows()``) mixed in batches of
1, 2 and 7 instances; ids grouped, shuffled row-wise and reversed; ld = c and c + 4; relu x residual; one constant column."""
import ctypes as C

import numpy as np
import pytest
import torch

import inorm_restatement as IR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
SENTINEL = -777.0
EPS = float(np.float32(1e-8))               # (the ABI takes a float: the restatement gets the same number)
ORDERS = ("grouped", "shuffled", "reversed")


def _lib():
    from eyoc_amd import _lib as L
    return L, L.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(a, pad, fill=NAN):
    a = np.ascontiguousarray(a, np.float32)
    full = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float32, device="cuda")
    full[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return full


def nan_workspace(nbytes):
    L, _ = _lib()
    ws = L.workspace(nbytes, torch.device("cuda"))
    ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(NAN)
    return ws


def chunk_rows():
    return int(_lib()[1].eyoc_in_chunk_rows())


def make_ids(sizes, order, rng):
    ids = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    if order == "shuffled":
        ids = ids[rng.permutation(len(ids))]
    elif order == "reversed":
        ids = ids[::-1].copy()
    return ids


def build_plan(ids, n_inst, expect=0):
    """-> (plan device tensor, header, seg, perm) - the last three as numpy, read through ``eyoc_in_plan_layout``."""
    L, lib = _lib()
    n = len(ids)
    coords = np.zeros((n, 4), np.int32)
    coords[:, 0] = ids
    coords[:, 1] = np.arange(n)
    nbytes = lib.eyoc_in_plan_bytes(n, n_inst)
    assert nbytes > 0
    plan = torch.full((nbytes // 4,), -1, dtype=torch.int32, device="cuda")
    rc = lib.eyoc_in_plan_build(L.ctx(), L.ptr(dev(coords)), n, n_inst, L.ptr(plan), nbytes, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.eyoc_last_error())
    if rc:
        return rc
    off = (C.c_int64 * 4)()
    L.check(lib.eyoc_in_plan_layout(n, n_inst, off), "eyoc_in_plan_layout")
    host = plan.cpu().numpy()
    seg = host[off[1] // 4: off[1] // 4 + n_inst + 1]
    perm = host[off[2] // 4: off[2] // 4 + n]
    return plan, host[:4], seg, perm


def in_input(rng, n, c, constant_column):
    """Columns with mean / std cycling through 0, 1, 1e3, 1e5 and a per-column std in [0.1, 10] (``bn_input`` of the batch-norm test);
    column 0 (ratio 0, weight 1, bias 0) straddles zero after the norm; ``constant_column`` holds one value in every row."""
    ratio = np.array([0.0, 1.0, 1e3, 1e5])[np.arange(c) % 4]
    std = 10.0 ** rng.uniform(-1.0, 1.0, c)
    x = (std * (ratio + rng.normal(size=(n, c)))).astype(np.float32)
    if constant_column is not None:
        x[:, constant_column] = np.float32(3.7 * std[constant_column])
    w = rng.uniform(0.5, 1.5, c).astype(np.float32)
    b = rng.normal(size=c).astype(np.float32)
    w[0], b[0] = 1.0, 0.0
    scale = 10.0 ** rng.uniform(-2.0, 2.0, c)
    dy = (rng.normal(size=(n, c)) * scale).astype(np.float32)
    res = rng.normal(size=(n, c)).astype(np.float32)
    return x, w, b, dy, res


def forward_gpu(x, plan, n_inst, w, b, relu, res, pad, ld_x=None, ws_bytes=None, expect=0, c_arg=None):
    L, lib = _lib()
    n, c = x.shape
    c_arg = c if c_arg is None else c_arg
    xd = padded(x, pad)
    rd = None if res is None else padded(res, pad)
    yd = torch.full((n, c + pad), SENTINEL, dtype=torch.float32, device="cuda")
    yd[:, :c] = NAN
    wd, bd = dev(w), dev(b)
    stats = torch.full((n_inst, 2 * c), NAN, dtype=torch.float32, device="cuda")
    need = lib.eyoc_in_workspace_bytes(n, c, n_inst)
    ws = nan_workspace(max(need, 256))
    rc = lib.eyoc_in_forward(L.ctx(), L.ptr(xd), n, c_arg, xd.stride(0) if ld_x is None else ld_x, L.ptr(plan), n_inst, L.ptr(wd), L.ptr(bd), EPS,
                             1 if relu else 0, L.ptr(rd), 0 if rd is None else rd.stride(0), L.ptr(yd), yd.stride(0), L.ptr(stats), L.ptr(ws),
                             need if ws_bytes is None else ws_bytes, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.eyoc_last_error())
    if rc:
        assert bool(torch.isnan(stats).all()) and bool(torch.isnan(yd[:, :c]).all())
        return rc
    full = yd.cpu().numpy()
    assert (full[:, c:] == SENTINEL).all(), "wrote into the pad columns of y"
    return full[:, :c].copy(), stats.cpu().numpy().reshape(n_inst, 2, c), yd


def backward_gpu(x, yd, dy, plan, n_inst, w, stats, pad, want_dres):
    """``yd``: the forward's own device output (with its pads) when a ReLU was fused, else None."""
    L, lib = _lib()
    n, c = x.shape
    xd, dyd = padded(x, pad), padded(dy, pad)
    if yd is not None:
        yd = yd.clone()
        yd[:, c:] = NAN
    outs = []
    for _ in range(2 if want_dres else 1):
        t = torch.full((n, c + pad), SENTINEL, dtype=torch.float32, device="cuda")
        t[:, :c] = NAN
        outs.append(t)
    dxd, drd = outs[0], (outs[1] if want_dres else None)
    wd, sd = dev(w), dev(stats.reshape(n_inst, 2 * c))
    dw, db = torch.full((c,), NAN, device="cuda"), torch.full((c,), NAN, device="cuda")
    need = lib.eyoc_in_workspace_bytes(n, c, n_inst)
    ws = nan_workspace(need)
    L.check(lib.eyoc_in_backward(L.ctx(), L.ptr(xd), xd.stride(0), L.ptr(yd), 0 if yd is None else yd.stride(0), L.ptr(dyd), dyd.stride(0), n, c,
                                 L.ptr(plan), n_inst, L.ptr(wd), L.ptr(sd), EPS, L.ptr(dxd), dxd.stride(0), L.ptr(drd),
                                 0 if drd is None else drd.stride(0), L.ptr(dw), L.ptr(db), L.ptr(ws), need, L.stream_ptr()), "eyoc_in_backward")
    torch.cuda.synchronize()
    res = []
    for t in outs:
        full = t.cpu().numpy()
        assert (full[:, c:] == SENTINEL).all(), "wrote into the pad columns of dx / dres"
        res.append(full[:, :c].copy())
    return res[0], (res[1] if want_dres else None), dw.cpu().numpy(), db.cpu().numpy()


def within_one_ulp(got, want64):
    w = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64)


def in_compare(x, w, b, dy, res, ids, sizes, relu, constant_column, y, stats, dx, dres, dweight, dbias, what=""):
    """The results of one forward (``stats [n_inst, 2, c]``) and one backward against the restatement under the bars of the module
    docstring; ``res``: the residual or None (``dres`` is then not looked at).  Returns the worst err / bound."""
    n_inst, n, c = len(sizes), len(ids), x.shape[1]
    with_res = res is not None
    y64, mean, var = IR.in_forward(x, ids, n_inst, w, b, EPS, False, res)
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    present = np.array(sizes) > 0
    assert np.isnan(stats[~present]).all(), "an instance id without rows must touch nothing"
    assert within_one_ulp(stats[present, 0], mean[present]).all(), ("mean", sizes, c)
    assert within_one_ulp(stats[present, 1], var[present]).all(), ("var", sizes, c)
    if constant_column is not None:
        assert (var[present][:, constant_column] == 0.0).all() and (stats[present, 1][:, constant_column] == 0.0).all()
    invstd_i = 1.0 / np.sqrt(var + EPS)
    mean_r, invstd = mean[ids], invstd_i[ids]
    xhat = (x.astype(np.float64) - mean_r) * invstd
    bound = 8 * U * (np.abs(xhat * w64) + np.abs(b64)) + 2 * U * np.abs(mean_r) * invstd * np.abs(w64)
    if with_res:
        bound = bound + U * np.abs(y64)
    err = np.abs(y - (np.maximum(y64, 0.0) if relu else y64))
    r_y = float((err / bound).max())
    assert np.isfinite(y).all() and (err <= bound).all(), ("y", sizes, what, c, relu, with_res, r_y)
    for i in np.flatnonzero(np.array(sizes) == 1):                      # one row: y = bias (+ residual), exactly
        rows = ids == i
        want = b[None, :] + (res[rows] if with_res else 0.0)
        np.testing.assert_array_equal(y[rows], np.maximum(want, 0.0) if relu else want)
    if relu:
        flipped = (y > 0) != (y64 > 0)
        assert (np.abs(y64[flipped]) <= bound[flipped]).all()
    dx64, g, dw64, db64 = IR.in_backward(x, y if relu else None, dy, ids, n_inst, w, mean, var, EPS)
    if with_res:
        np.testing.assert_array_equal(dres, g.astype(np.float32))
    e_xhat = 6 * U * np.abs(xhat) + 2 * U * np.abs(mean_r) * invstd
    E_b = U * np.abs(db64) + n * 2.0 ** -53 * np.abs(g).sum(0)
    E_g = (np.abs(g) * e_xhat).sum(0) + U * np.abs(dw64) + n * 2.0 ** -53 * np.abs(g * xhat).sum(0)
    E_dx = np.zeros_like(dx64)
    for i in np.flatnonzero(present):
        rows = np.flatnonzero(ids == i)
        nb = len(rows)
        gi, xh, ex = g[rows], xhat[rows], e_xhat[rows]
        sb, sg = gi.sum(0), (gi * xh).sum(0)
        Eb_i = U * np.abs(sb) + nb * 2.0 ** -53 * np.abs(gi).sum(0)
        Eg_i = (np.abs(gi) * ex).sum(0) + U * np.abs(sg) + nb * 2.0 ** -53 * np.abs(gi * xh).sum(0)
        B = gi - sb / nb - xh * sg / nb
        E_B = (Eb_i / nb + 2 * U * np.abs(sb) / nb + (ex * np.abs(sg) + np.abs(xh) * Eg_i) / nb + 3 * U * np.abs(xh * sg) / nb
               + U * (np.abs(gi) + np.abs(sb) / nb) + U * np.abs(B))
        E_dx[rows] = np.abs(w64) * invstd_i[i] * E_B + 6 * U * np.abs(dx64[rows])
    ratios = {}
    for name, got, want, E in (("dbias", dbias, db64, E_b), ("dweight", dweight, dw64, E_g), ("dx", dx, dx64, E_dx)):
        e = np.abs(got - want)
        assert np.isfinite(got).all() and (e <= E).all(), (name, sizes, what, c, relu, with_res, float(np.max(e / np.maximum(E, 1e-300))))
        ratios[name] = float(np.max(np.divide(e, E, out=np.zeros_like(e), where=E > 0), initial=0.0))
    print(f"in sizes={sizes} {what} c={c} relu={int(relu)} res={int(with_res)}: max err / bound  y {r_y:.3g}  "
          f"dbias {ratios['dbias']:.3g}  dweight {ratios['dweight']:.3g}  dx {ratios['dx']:.3g}")
    return max(r_y, *ratios.values())


def in_check(sizes, order, c, relu, with_res, pad, constant_column, seed):
    """One forward + backward through the raw entry points, each twice (the same bits), under ``in_compare``."""
    rng = np.random.default_rng([c, int(relu), int(with_res), seed, len(sizes)])
    n_inst = len(sizes)
    ids = make_ids(sizes, order, rng)
    x, w, b, dy, res = in_input(rng, len(ids), c, constant_column)
    if not with_res:
        res = None
    plan, hdr, seg, perm = build_plan(ids, n_inst)
    y, stats, yd = forward_gpu(x, plan, n_inst, w, b, relu, res, pad)
    y2, stats2, _ = forward_gpu(x, plan, n_inst, w, b, relu, res, pad)
    assert y.tobytes() == y2.tobytes() and stats.tobytes() == stats2.tobytes()
    dx, dres, dweight, dbias = backward_gpu(x, yd if relu else None, dy, plan, n_inst, w, stats, pad, with_res)
    dx2, dres2, dweight2, dbias2 = backward_gpu(x, yd if relu else None, dy, plan, n_inst, w, stats, pad, with_res)
    assert dx.tobytes() == dx2.tobytes() and dweight.tobytes() == dweight2.tobytes() and dbias.tobytes() == dbias2.tobytes()
    return in_compare(x, w, b, dy, res, ids, sizes, relu, constant_column, y, stats, dx, dres, dweight, dbias, what=f"{order} pad={pad}")


def batches():
    """Instance sizes from {0, 1, 2, R-1, R, R+1, 3R+1} in batches of 7, 2, 2 and 1 instances."""
    R = chunk_rows()
    return [[R + 1, 0, 1, 3 * R + 1, 2, R - 1, R], [3 * R + 1, R - 1], [1, R], [3 * R + 1]]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("c", [32, 64, 128, 256])
def test_in_kernels_against_the_restatement(c, order):
    worst = 0.0
    for k, sizes in enumerate(batches()):
        for relu in (False, True):
            for with_res in (False, True):
                pad = 4 if (int(relu) + int(with_res) + k) % 2 == 0 else 0          # ld = c + 4 and ld = c, each with every combination somewhere
                worst = max(worst, in_check(sizes, order, c, relu, with_res, pad, c - 3, k))
    print(f"in c={c} {order}: worst max err / bound = {worst:.3g}")


@pytest.mark.parametrize("c", [32, 256])
def test_both_leading_dimensions_with_every_combination(c):
    sizes = batches()[0]
    for relu in (False, True):
        for with_res in (False, True):
            for pad in (0, 4):
                in_check(sizes, "shuffled", c, relu, with_res, pad, c - 3, 40 + pad)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("c", [32, 64, 128, 256])
def test_an_instance_alone_gives_the_bytes_of_the_batched_call(c, order):
    """stats, y and dx rows of every instance: the same bytes from the call on the whole batch and from a call on that instance alone
    (n_inst = 1, its rows in the same relative order), whatever the order of the batch's rows."""
    sizes = batches()[0]
    rng = np.random.default_rng([c, 77])
    ids = make_ids(sizes, order, rng)
    x, w, b, dy, res = in_input(rng, len(ids), c, c - 3)
    plan, hdr, _, _ = build_plan(ids, len(sizes))
    assert hdr[0] == (1 if order == "grouped" else 0)
    y, stats, yd = forward_gpu(x, plan, len(sizes), w, b, True, res, 4)
    dx, dres, _, _ = backward_gpu(x, yd, dy, plan, len(sizes), w, stats, 4, True)
    for i, nb in enumerate(sizes):
        if nb == 0:
            continue
        rows = np.flatnonzero(ids == i)
        plan1, hdr1, seg1, _ = build_plan(np.zeros(nb, np.int32), 1)
        assert hdr1[0] == 1 and list(seg1) == [0, nb]
        y1, stats1, yd1 = forward_gpu(x[rows], plan1, 1, w, b, True, res[rows], 4)
        dx1, dres1, _, _ = backward_gpu(x[rows], yd1, dy[rows], plan1, 1, w, stats1, 4, True)
        assert stats1[0].tobytes() == stats[i].tobytes(), ("stats", i, nb)
        assert y1.tobytes() == y[rows].tobytes(), ("y", i, nb)
        assert dx1.tobytes() == dx[rows].tobytes() and dres1.tobytes() == dres[rows].tobytes(), ("dx", i, nb)


def test_the_three_orders_of_one_batch_agree_per_instance():
    """The same instances grouped, shuffled ACROSS instances (relative order inside an instance kept) and interleaved round-robin:
    every instance's statistics and rows come out with the same bytes."""
    c = 64
    sizes = batches()[0]
    rng = np.random.default_rng(5)
    grouped = make_ids(sizes, "grouped", rng)
    x, w, b, dy, res = in_input(rng, len(grouped), c, c - 3)
    results = []
    for trial in range(3):
        # a permutation of the rows that is stable inside every instance
        round_robin = np.argsort(np.concatenate([np.arange(s) for s in sizes]), kind="stable")
        ids = (grouped, rng.permutation(grouped), grouped[round_robin])[trial]
        seen, starts, order = np.zeros(len(sizes), np.int64), np.concatenate([[0], np.cumsum(sizes)]), []
        for i in ids:                                       # the k-th row of an instance stays its k-th row
            order.append(starts[i] + seen[i])
            seen[i] += 1
        order = np.array(order)
        rows_of = [order[ids == i] for i in range(len(sizes))]
        assert all((np.diff(r) > 0).all() for r in rows_of)
        plan, _, _, _ = build_plan(ids, len(sizes))
        y, stats, yd = forward_gpu(x[order], plan, len(sizes), w, b, True, res[order], 0)
        dx, _, dw, db = backward_gpu(x[order], yd, dy[order], plan, len(sizes), w, stats, 0, False)
        back = np.argsort(order)
        results.append((stats.tobytes(), y[back].tobytes(), dx[back].tobytes(), dw.tobytes(), db.tobytes()))
    assert results[0] == results[1] == results[2]


@pytest.mark.parametrize("n,n_inst", [(389, 7), (5000, 7), (3000, 1024), (1, 1), (1025, 2)])
def test_plans(n, n_inst):
    """Grouped ids report identity; shuffled ids give ``np.argsort(ids, kind="stable")`` and the ``np.bincount`` prefix sums exactly
    (5000 and 3000 rows: several workgroups of the counting sort; 1024 instances: the limit)."""
    rng = np.random.default_rng([n, n_inst])
    ids = np.sort(rng.integers(0, n_inst, n)).astype(np.int32)
    want_seg = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=n_inst))])
    _, hdr, seg, perm = build_plan(ids, n_inst)
    assert list(hdr) == [1, n, n_inst, 0]
    np.testing.assert_array_equal(seg, want_seg)
    np.testing.assert_array_equal(perm, np.arange(n))
    shuffled = ids[rng.permutation(n)]
    _, hdr, seg, perm = build_plan(shuffled, n_inst)
    np.testing.assert_array_equal(seg, want_seg)
    np.testing.assert_array_equal(perm, np.argsort(shuffled, kind="stable"))
    assert hdr[0] == (1 if (np.diff(shuffled) >= 0).all() else 0)


def test_refusals():
    L, lib = _lib()
    rng = np.random.default_rng(3)
    ids = np.repeat(np.arange(2), 50).astype(np.int32)
    plan, _, _, _ = build_plan(ids, 2)
    ones, zeros = np.ones(32, np.float32), np.zeros(32, np.float32)
    x = rng.normal(size=(100, 32)).astype(np.float32)
    x12 = rng.normal(size=(100, 12)).astype(np.float32)
    assert lib.eyoc_in_workspace_bytes(100, 12, 2) == 0
    assert forward_gpu(x12, plan, 2, ones[:12], zeros[:12], False, None, 4, expect=L.ERR_INVALID) == L.ERR_INVALID          # c = 12
    assert forward_gpu(x, plan, 2, ones, zeros, False, None, 4, ld_x=28, expect=L.ERR_INVALID) == L.ERR_INVALID            # ld < c
    assert forward_gpu(x, plan, 2, ones, zeros, False, None, 4, ld_x=34, expect=L.ERR_INVALID) == L.ERR_INVALID            # misaligned ld
    need = lib.eyoc_in_workspace_bytes(100, 32, 2)
    assert need > 0
    assert forward_gpu(x, plan, 2, ones, zeros, False, None, 4, ws_bytes=need - 1, expect=L.ERR_WORKSPACE) == L.ERR_WORKSPACE
    assert build_plan(ids, 1, expect=L.ERR_INVALID) == L.ERR_INVALID                                                      # an id equal to n_inst
    assert b"instance id" in lib.eyoc_last_error()
    bad = ids.copy()
    bad[7] = -1
    assert build_plan(bad, 2, expect=L.ERR_INVALID) == L.ERR_INVALID
    assert lib.eyoc_in_plan_bytes(100, 1025) == 0 and lib.eyoc_in_plan_bytes(0, 1) == 0
    y, stats, _ = forward_gpu(x, plan, 2, ones, zeros, False, None, 4)                                                     # and the good call works
    assert np.isfinite(y).all()
