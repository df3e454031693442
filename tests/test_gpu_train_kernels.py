"""The training-side kernels alone, through the raw C ABI, against the float64 restatements of tests/train_restatement.py:
``eyoc_spconv_grad_weight`` (csrc/spconv_grad.hip), ``eyoc_spconv_sum`` with its offset split (csrc/spconv.hip), the batch-norm kernels
and the window gather (csrc/bn.hip), and one training step on a batch small enough for the coarse levels to have a few dozen rows.

Two kinds of data.  INTEGER cases: operands from -4 .. 4 (about 30 % zeros), so every product and partial sum is an integer far below
2^24 and fp32 arithmetic is exact in any order - the GPU result must be BIT-EQUAL to the restatement (one dropped, doubled or misplaced
pair changes an integer).  FLOAT cases: N(0, 1) times a per-column log-uniform scale in [1e-2, 1e2]; the bar is
``|got - want64| <= (P + 2) u S`` (u = 2^-24, P products summed into the entry, S the sum of their absolute values): the standard
bound of a length-P fp32 sum in any order plus one rounding each for the product and the store.  The realised ``max err / bound`` is
printed; nothing is asserted on it beyond ``<= 1``.  Pad columns, outputs and workspaces start out as NaN wherever the ABI allows it.
No tolerance in this file comes from the code under test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import train_restatement as R

pytestmark = pytest.mark.gpu

U = R.U32
NAN = float("nan")
SENTINEL = -777.0


# ---------------------------------------------------------------- plumbing

def _lib():
    from eyoc_amd import _lib as L
    return L, L.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(a, pad, fill=NAN):
    """``a`` in the first columns of a ``[rows, cols + pad]`` device tensor whose other columns hold ``fill``; the leading dimension is
    ``stride(0)``."""
    a = np.ascontiguousarray(a, np.float32)
    full = torch.full((max(a.shape[0], 1), a.shape[1] + pad), fill, dtype=torch.float32, device="cuda")
    if a.shape[0]:
        full[:a.shape[0], :a.shape[1]] = torch.from_numpy(a).cuda()
    return full


def nan_workspace(nbytes):
    L, _ = _lib()
    ws = L.workspace(nbytes, torch.device("cuda"))
    ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(NAN)
    return ws


def check_float(got, want, S, P, what):
    bound = R.rounding_bound(S, P)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0), initial=0.0))
    print(f"{what}: max |err| / bound = {ratio:.3g}")
    assert np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, ratio, float(err.max()))
    return ratio


# ================================================================ (a) eyoc_spconv_grad_weight

def grad_weight(nbr, n_out, x, dy, K, pads=(0, 0), ws_bytes=None, ws_offset=0, expect=0):
    """One call with a test-owned NaN workspace; ``dW`` starts out as NaN.  Returns ``dW`` (numpy) or the refusal's return code."""
    L, lib = _lib()
    cin, cout = x.shape[1], dy.shape[1]
    xd, dyd = padded(x, pads[0]), padded(dy, pads[1])
    nd = None if nbr is None else dev(np.ascontiguousarray(nbr if nbr.size else np.full((nbr.shape[0], 1), -1), np.int32))
    need = lib.eyoc_spconv_grad_weight_workspace_bytes(K, n_out, cin, cout)
    ws = nan_workspace(need + 256)
    assert ws.data_ptr() % 256 == 0 and need > 0
    dw = torch.full((K, cin, cout), NAN, dtype=torch.float32, device="cuda")
    rc = lib.eyoc_spconv_grad_weight(L.ctx(), L.ptr(nd), K, n_out, L.ptr(xd), xd.stride(0), cin, L.ptr(dyd), dyd.stride(0), cout,
                                     L.ptr(dw), C.c_void_p(ws.data_ptr() + ws_offset), need if ws_bytes is None else ws_bytes, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.eyoc_last_error())
    if rc:
        assert bool(torch.isnan(dw).all()), "a refused call wrote dW"
        return rc
    return dw.cpu().numpy()


def gw_check(nbr, n_out, x, dy, K, integer, what, layouts=((0, 0), (4, 12))):
    want, S, P = R.conv_grad_weight(nbr, x, dy)
    ratio = 0.0
    for pads in layouts:
        got = grad_weight(nbr, n_out, x, dy, K, pads)
        if integer:
            np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=f"{what} pads {pads}")
        else:
            ratio = max(ratio, check_float(got, want, S, P, f"{what} pads {pads}"))
    return ratio


@pytest.mark.parametrize("cin,cout", R.GW_PAIRS_NINE + R.GW_PAIRS_WIDE, ids=lambda v: str(v))
def test_grad_weight_channel_tiles_and_row_boundaries(cin, cout):
    """Every ``k_grad_weight<TI,TJ>`` ({16, 32, 64}^2) and several channel tiles in grid.z, at row counts on the four-pair MFMA step,
    the 64-row batch, the four waves of a workgroup and the 1024-row block; contiguous and ``ld_in = cin + 4`` / ``ld_dout = cout + 12``
    with NaN pads.  Integer data bit-equal, float data within ``(P + 2) u S``."""
    worst = 0.0
    for n_out in R.gw_sizes(cin, cout):
        nbr, x, dy = R.gw_case(cin, cout, n_out, True)
        gw_check(nbr, n_out, x, dy, 27, True, f"dW {cin}x{cout} n_out={n_out} integer")
        nbr, x, dy = R.gw_case(cin, cout, n_out, False)
        worst = max(worst, gw_check(nbr, n_out, x, dy, 27, False, f"dW {cin}x{cout} n_out={n_out} float", layouts=((4, 12),)))
    print(f"grad_weight {cin}x{cout}: worst max |err| / bound over the sizes = {worst:.3g}")


@functools.lru_cache(maxsize=None)
def _gw_large():
    nbr, x, dy = R.gw_case(256, 256, 9217, True, density=3 / 27)
    return nbr, x, dy, R.conv_grad_weight(nbr, x, dy)[0].astype(np.float32)


def test_grad_weight_halved_block_count_and_repeatability():
    """256 x 256 channels, K = 27, 9217 rows at about three neighbours per row: ``grad_weight_blocks`` halves its 10 row blocks to 5.
    Two calls give the same bits."""
    nbr, x, dy, want = _gw_large()
    assert R.grad_weight_rows_per_block(9217, 27, 256, 256)[0] == 5
    got = grad_weight(nbr, 9217, x, dy, 27)
    np.testing.assert_array_equal(got, want)
    again = grad_weight(nbr, 9217, x, dy, 27)
    assert got.tobytes() == again.tobytes()
    nbr, x, dy = R.gw_case(64, 32, 1025, False)
    a, b = grad_weight(nbr, 1025, x, dy, 27, (4, 12)), grad_weight(nbr, 1025, x, dy, 27, (4, 12))
    assert a.tobytes() == b.tobytes()


def test_grad_weight_rulebooks():
    """Real stride-1 / down / up tables of a small cloud (``n_in != n_out``), the synthetic table with the planted patterns (an offset
    without pairs, rows without neighbours, an empty row block of one offset, batches with P % 4 = 1, 2, 3: asserted by its builder),
    and ``nbr = NULL`` with K = 1."""
    rng = np.random.default_rng(17)
    t = R.real_tables(R.small_cloud(rng, 257))
    n0, n1 = t["n"]
    assert n0 == 257 and 1 < n1 < n0
    planted, n_in = R.gw_planted_table()
    cases = [("s1", t["s1"], n0, 27), ("down", t["down"], n0, 27), ("up", t["up"], n1, 27), ("planted", planted, n_in, 27), ("identity", None, 300, 1)]
    for name, nbr, rows_in, K in cases:
        n_out = rows_in if nbr is None else nbr.shape[1]
        for cin, cout in ((32, 32), (16, 64)):
            for integer in (True, False):
                draw = R.integer_data if integer else R.float_data
                x, dy = draw(rng, (rows_in, cin)), draw(rng, (n_out, cout))
                gw_check(nbr, n_out, x, dy, K, integer, f"dW {name} {cin}x{cout} {'integer' if integer else 'float'}")


def test_grad_weight_zero_rows_and_refusals():
    L, lib = _lib()
    rng = np.random.default_rng(1)
    x, dy = R.integer_data(rng, (5, 32)), R.integer_data(rng, (5, 32))
    nbr = R.synthetic_table(rng, 27, 5, 5, 0.5)
    got = grad_weight(nbr[:, :0], 0, x, dy, 27)                       # n_out = 0: an all-zero dW (not NaN, not skipped)
    assert got.shape == (27, 32, 32) and not got.any()
    # refusals: the return code, and dW still NaN (nothing launched)
    need = lib.eyoc_spconv_grad_weight_workspace_bytes(27, 5, 32, 32)
    assert grad_weight(nbr, 5, R.integer_data(rng, (5, 24)), dy, 27, expect=L.ERR_INVALID) == L.ERR_INVALID          # cin = 24
    assert grad_weight(nbr, 5, x, dy, 27, ws_offset=64, expect=L.ERR_WORKSPACE) == L.ERR_WORKSPACE                  # unaligned workspace
    assert grad_weight(nbr, 5, x, dy, 27, ws_bytes=need - 1, expect=L.ERR_WORKSPACE) == L.ERR_WORKSPACE             # too small
    assert grad_weight(None, 5, x, dy, 27, expect=L.ERR_INVALID) == L.ERR_INVALID                                   # NULL table, K = 27


# ================================================================ (b) eyoc_spconv_sum: forward and input gradient

@pytest.fixture()
def tiled_kernel():
    """``eyoc_spconv_select_kernel(0)``: the workgroup-tiled kernel, which owns the offset split; restored afterwards."""
    L, _ = _lib()
    prev = L.knob("eyoc_spconv_select_kernel", 0)
    yield
    L.knob("eyoc_spconv_select_kernel", prev)


def pack(W):
    _, lib = _lib()
    K, cin, cout = W.shape
    packed = np.full(W.size, np.nan, np.float32)
    assert lib.eyoc_spconv_pack_weights(np.ascontiguousarray(W, np.float32).ctypes.data, None, K, cin, cout, packed.ctypes.data) == 0
    return packed


def pack_transposed(W, mirror):
    _, lib = _lib()
    K, cin, cout = W.shape
    packed = np.full(W.size, np.nan, np.float32)
    assert lib.eyoc_spconv_pack_weights_transposed(np.ascontiguousarray(W, np.float32).ctypes.data, K, cin, cout, mirror, packed.ctypes.data) == 0
    return packed


def spconv_sum(nbr, n_out, x, packed, cin, cout, out=None):
    """One ``eyoc_spconv_sum`` call; the output starts out as NaN.  ``out``: a device view to write into (its ``stride(0)`` is ``ld_out``)."""
    L, lib = _lib()
    xd = x if isinstance(x, torch.Tensor) else dev(np.asarray(x, np.float32))
    nd = None if nbr is None else dev(np.asarray(nbr, np.int32))
    wd = dev(packed)
    own = out is None
    if own:
        out = torch.full((n_out, cout), NAN, dtype=torch.float32, device="cuda")
    K = 1 if nbr is None else nbr.shape[0]
    L.check(lib.eyoc_spconv_sum(L.ctx(), L.ptr(nd), K, n_out, L.ptr(xd), xd.stride(0), cin, L.ptr(wd), cout, L.ptr(out), out.stride(0),
                                L.stream_ptr()), "eyoc_spconv_sum")
    torch.cuda.synchronize()
    return out.cpu().numpy() if own else None


@functools.lru_cache(maxsize=None)
def _sum_case(cin, cout, n_out, empty=()):
    nbr, x, W = R.sum_case(cin, cout, n_out, empty)
    return nbr, x, W, R.conv_forward(nbr, x, W)[0].astype(np.float32)


# (the sizes and why they are these: SUM_SIZES_256 in tests/train_restatement.py - they sit on launch_spconv's thresholds
# cdiv(n_out, 32) * (cout / spconv_ct(cout)) = 512 | 682 | 1024; a change of that rule must be followed by a change of the sizes)
@pytest.mark.parametrize("n_out", R.SUM_SIZES_256)
def test_sum_forward_on_the_split_thresholds(tiled_kernel, n_out):
    nbr, x, W, want = _sum_case(32, 256, n_out)
    got = spconv_sum(nbr, n_out, x, pack(W), 32, 256)
    np.testing.assert_array_equal(got, want, err_msg=f"n_out {n_out}, {R.offset_split(n_out, 256)} shares")


@pytest.mark.parametrize("cin,cout", R.SUM_SHAPES_NARROW)
def test_sum_forward_other_shapes(tiled_kernel, cin, cout):
    for n_out in R.SUM_SIZES_NARROW:
        nbr, x, W, want = _sum_case(cin, cout, n_out)
        np.testing.assert_array_equal(spconv_sum(nbr, n_out, x, pack(W), cin, cout), want, err_msg=f"n_out {n_out}")


def _poison_scratch():
    """A larger split call whose input is all NaN, every (offset, row) a pair: each of its four shares is NaN in every entry, and they
    stay behind in the context's scratch for whatever runs next on the stream."""
    n = 512
    assert R.offset_split(n, 256) == 4
    nbr = ((np.arange(n)[None, :] + np.arange(27)[:, None]) % n).astype(np.int32)
    W = R.integer_data(np.random.default_rng(2), (27, 32, 256))
    out = spconv_sum(nbr, n, np.full((n, 32), np.nan, np.float32), pack(W), 32, 256)
    assert np.isnan(out).all()


@pytest.mark.parametrize("empty", [tuple(range(0, 7)), tuple(range(20, 27))], ids=["first_share_empty", "last_share_empty"])
def test_sum_share_without_pairs_and_scratch_left_by_another_call(tiled_kernel, empty):
    """A four-way split whose first (offsets 0..5) or last (20..26) share has nothing to add, run behind a call that left NaN in
    every entry of the shared scratch: the share must still WRITE its zeros."""
    nbr, x, W, want = _sum_case(32, 256, 100, empty)
    assert (nbr[list(empty)] < 0).all() and R.offset_split(100, 256) == 4
    np.testing.assert_array_equal(spconv_sum(nbr, 100, x, pack(W), 32, 256), want)
    _poison_scratch()
    np.testing.assert_array_equal(spconv_sum(nbr, 100, x, pack(W), 32, 256), want)
    _poison_scratch()
    nbr, x, W, want = _sum_case(32, 256, 33)
    np.testing.assert_array_equal(spconv_sum(nbr, 33, x, pack(W), 32, 256), want)


@pytest.mark.parametrize("n", [1, 33, 257])
def test_sum_input_gradient(tiled_kernel, n):
    """The input gradient as ``autograd.input_gradient`` runs it: a stride-1 table is its own transpose under mirrored offsets
    (``mirror = 1``, same table); the down table's transpose is the up table and the reverse (``mirror = 0``)."""
    rng = np.random.default_rng(100 + n)
    t = R.real_tables(R.small_cloud(rng, n))
    n0, n1 = t["n"]
    assert n0 == n
    cin, cout = 32, 64
    W = R.integer_data(rng, (27, cin, cout))
    # (layer's table, rows of its input, the transposed table the kernel walks, mirror)
    for name, nbr, rows_in, nbr_t, mirror in (("s1", t["s1"], n0, t["s1"], 1), ("down", t["down"], n0, t["up"], 0), ("up", t["up"], n1, t["down"], 0)):
        assert nbr_t.shape[1] == rows_in
        dy = R.integer_data(rng, (nbr.shape[1], cout))
        want = R.conv_grad_input(nbr, rows_in, dy, W)[0]
        assert R.exactly_fp32(want)
        got = spconv_sum(nbr_t, rows_in, dy, pack_transposed(W, mirror), cout, cin)
        np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=name)


def test_sum_input_gradient_in_column_blocks(tiled_kernel):
    """C_in = 192 (``autograd.input_gradient``'s column-block path): the gradient is written into ``[:, 0:128]`` and ``[:, 128:192]``
    of one tensor with ``ld_out = 192``."""
    rng = np.random.default_rng(192)
    nbr = R.real_tables(R.small_cloud(rng, 257))["s1"]
    cin, cout = 192, 64
    W, dy = R.integer_data(rng, (27, cin, cout)), R.integer_data(rng, (257, cout))
    want = R.conv_grad_input(nbr, 257, dy, W)[0]
    assert R.exactly_fp32(want)
    dx = torch.full((257, cin), NAN, dtype=torch.float32, device="cuda")
    for a, w in ((0, 128), (128, 64)):
        spconv_sum(nbr, 257, dy, pack_transposed(np.ascontiguousarray(W[:, a:a + w, :]), 1), cout, w, out=dx[:, a:a + w])
    np.testing.assert_array_equal(dx.cpu().numpy(), want.astype(np.float32))


# ================================================================ (c) batch-norm kernels

EPS = 1e-5
MOMENTUM = float(np.float32(0.05))          # (the ABI takes a float: the restatement gets the same number)


def bn_input(rng, n, c, constant_column):
    """Columns with mean / std cycling through 0, 1, 1e3, 1e5 and a per-column std in [0.1, 10]; column 0 (mean / std = 0, beta = 0)
    straddles zero after the norm; ``constant_column`` (or None) holds one value in every row (var = 0)."""
    ratio = np.array([0.0, 1.0, 1e3, 1e5])[np.arange(c) % 4]
    std = 10.0 ** rng.uniform(-1.0, 1.0, c)
    x = (std * (ratio + rng.normal(size=(n, c)))).astype(np.float32)
    if constant_column is not None:
        x[:, constant_column] = np.float32(3.7 * std[constant_column])
    gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
    beta = rng.normal(size=c).astype(np.float32)
    gamma[0], beta[0] = 1.0, 0.0
    return x, gamma, beta, R.float_data(rng, (n, c))


def bn_forward_gpu(x, gamma, beta, relu, pad, running=None, ld_x=None, ws_bytes=None, expect=0):
    L, lib = _lib()
    n, c = x.shape
    xd = padded(x, pad)
    yd = torch.full((n, c + pad), SENTINEL, dtype=torch.float32, device="cuda")
    yd[:, :c] = NAN
    gd, bd = dev(gamma), dev(beta)
    stats = torch.full((2 * c,), NAN, dtype=torch.float32, device="cuda")
    need = lib.eyoc_bn_workspace_bytes(n, c)
    ws = nan_workspace(max(need, 256))
    args = [L.ctx(), L.ptr(xd), n, c, xd.stride(0) if ld_x is None else ld_x, L.ptr(gd), L.ptr(bd), EPS, 1 if relu else 0, L.ptr(yd), yd.stride(0), L.ptr(stats)]
    tail = [L.ptr(ws), need if ws_bytes is None else ws_bytes, L.stream_ptr()]
    if running is not None:
        rm, rv = dev(running[0]), dev(running[1])
        rc = lib.eyoc_bn_train_forward_running(*args, L.ptr(rm), L.ptr(rv), MOMENTUM, *tail)
    else:
        rc = lib.eyoc_bn_train_forward(*args, *tail)
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.eyoc_last_error())
    if rc:
        assert bool(torch.isnan(stats).all())
        return rc
    full = yd.cpu().numpy()
    assert (full[:, c:] == SENTINEL).all(), "wrote into the pad columns of y"
    return full[:, :c].copy(), stats.cpu().numpy(), (None if running is None else (rm.cpu().numpy(), rv.cpu().numpy())), yd


def bn_backward_gpu(x, yd, dy, gamma, stats, pad):
    """``yd``: the forward's own device output (with its pads) when a ReLU followed, else None."""
    L, lib = _lib()
    n, c = x.shape
    xd, dyd = padded(x, pad), padded(dy, pad)
    if yd is not None:
        yd = yd.clone()
        yd[:, c:] = NAN
    dxd = torch.full((n, c + pad), SENTINEL, dtype=torch.float32, device="cuda")
    dxd[:, :c] = NAN
    gd, sd = dev(gamma), dev(stats)
    dg, db = torch.full((c,), NAN, device="cuda"), torch.full((c,), NAN, device="cuda")
    need = lib.eyoc_bn_workspace_bytes(n, c)
    ws = nan_workspace(need)
    L.check(lib.eyoc_bn_train_backward(L.ctx(), L.ptr(xd), xd.stride(0), L.ptr(yd), 0 if yd is None else yd.stride(0), L.ptr(dyd), dyd.stride(0), n, c,
                                       L.ptr(gd), L.ptr(sd), EPS, L.ptr(dxd), dxd.stride(0), L.ptr(dg), L.ptr(db), L.ptr(ws), need, L.stream_ptr()),
            "eyoc_bn_train_backward")
    torch.cuda.synchronize()
    full = dxd.cpu().numpy()
    assert (full[:, c:] == SENTINEL).all(), "wrote into the pad columns of dx"
    return full[:, :c].copy(), dg.cpu().numpy(), db.cpu().numpy()


def within_one_ulp(got, want64):
    w = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64)


def bn_compare(x, gamma, beta, dy, relu, constant_column, y, stats, dx, dgamma, dbeta, run0=None, run=None, what=""):
    """The results of one forward (``run0`` / ``run``: the running statistics before and after it, or None for the plain entry point) and one
    backward against the restatement; ``what``: a label for messages.  Returns the worst err / bound.  Bars, u = 2^-24, all quantities on the right from the
    float64 restatement (invstd = 1 / sqrt(var + eps), xhat = (x - mean) invstd):

    forward   |y - y64| <= 8u (|xhat gamma| + |beta|) + 2u |mean| invstd |gamma|: the seven fp32 roundings of k_bn_apply (x - mean, var + eps,
              sqrt, 1 / ., * invstd, * gamma, + beta; divide and sqrt are correctly rounded), and the mean stored in fp32 - a property of the
              interface.  mean and var: within 1 ulp of the float64 value rounded to fp32.  ReLU decisions may differ only where
              |y64| <= that bound.
    xhat      as the kernels form it in fp32: var within 1 ulp (2u), + eps (u), sqrt (halves, + u), 1 / . (u): invstd within 4u; x - mean (u)
              and the product (u): e_xhat = 6u |xhat| + 2u |mean| invstd.
    dbeta     fp64 sum of exact fp32 terms, stored in fp32:  E_b = u |dbeta| + n 2^-53 sum|g|         (g = dy where y > 0)
    dgamma    fp64 sum of g * xhat_fp32, stored in fp32:      E_g = sum_r |g| e_xhat + u |dgamma| + n 2^-53 sum|g xhat|
    dx        = fl(gamma invstd) * (g - dbeta inv_n - xhat dgamma inv_n), inv_n = fl(1 / n) (u), B the bracket:
              E_B = E_b / n + 2u |dbeta| / n + (e_xhat |dgamma| + |xhat| E_g) / n + 3u |xhat dgamma| / n + u (|g| + |dbeta| / n) + u |B|
              E_dx = |gamma| invstd E_B + 6u |dx|        (gamma invstd: 4u + u, the last product u)
    The backward restatement is given the GPU's own y for the ReLU mask (the forward's decisions are checked above)."""
    n, c = x.shape
    y64, mean, var = R.bn_forward(x, gamma, beta, EPS, False)
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    invstd = 1.0 / np.sqrt(var + EPS)
    xhat = (x.astype(np.float64) - mean) * invstd
    if constant_column is not None:
        assert var[constant_column] == 0.0
    if n > 1:
        assert (y64[:, 0] > 0).any() and (y64[:, 0] < 0).any()          # column 0 straddles zero: the ReLU mask matters
    assert within_one_ulp(stats[:c], mean).all(), ("mean", n, c)
    assert within_one_ulp(stats[c:], var).all(), ("var", n, c, np.abs(stats[c:] - var).max())
    bound = 8 * U * (np.abs(xhat * g64) + np.abs(b64)) + 2 * U * np.abs(mean) * invstd * np.abs(g64)
    err = np.abs(y - (np.maximum(y64, 0.0) if relu else y64))
    r_y = float((err / bound).max())
    assert (err <= bound).all(), ("y", n, c, relu, r_y)
    if relu:
        flipped = (y > 0) != (y64 > 0)
        assert (np.abs(y64[flipped]) <= bound[flipped]).all() and int(flipped.sum()) <= int((np.abs(y64) <= bound).sum())
    if run is not None:
        # running statistics: (1 - m) (u), the two products (u each), the sum (u), the statistic itself (2u), the unbiasing factor (2u)
        want_rm, want_rv = R.bn_running(run0[0], run0[1], mean, var, n, MOMENTUM)
        for got, want, old, stat in ((run[0], want_rm, run0[0], mean), (run[1], want_rv, run0[1], var * (n / max(n - 1, 1)))):
            assert (np.abs(got - want) <= 8 * U * ((1 - MOMENTUM) * np.abs(old) + MOMENTUM * np.abs(stat))).all(), ("running", n, c)
    dx64, dg64, db64 = R.bn_backward(x, y if relu else None, dy, gamma, mean, var, EPS)
    g = np.where(y > 0, dy, 0.0).astype(np.float64) if relu else dy.astype(np.float64)
    e_xhat = 6 * U * np.abs(xhat) + 2 * U * np.abs(mean) * invstd
    E_b = U * np.abs(db64) + n * 2.0 ** -53 * np.abs(g).sum(0)
    E_g = (np.abs(g) * e_xhat).sum(0) + U * np.abs(dg64) + n * 2.0 ** -53 * np.abs(g * xhat).sum(0)
    B = g - db64 / n - xhat * dg64 / n
    E_B = (E_b / n + 2 * U * np.abs(db64) / n + (e_xhat * np.abs(dg64) + np.abs(xhat) * E_g) / n + 3 * U * np.abs(xhat * dg64) / n
           + U * (np.abs(g) + np.abs(db64) / n) + U * np.abs(B))
    E_dx = np.abs(g64) * invstd * E_B + 6 * U * np.abs(dx64)
    ratios = {}
    for name, got, want, E in (("dbeta", dbeta, db64, E_b), ("dgamma", dgamma, dg64, E_g), ("dx", dx, dx64, E_dx)):
        e = np.abs(got - want)
        assert np.isfinite(got).all() and (e <= E).all(), (name, n, c, relu, float(np.max(e / np.maximum(E, 1e-300))))
        ratios[name] = float(np.max(np.divide(e, E, out=np.zeros_like(e), where=E > 0), initial=0.0))
    print(f"bn n={n} c={c} relu={int(relu)} {what}: max err / bound  y {r_y:.3g}  dbeta {ratios['dbeta']:.3g}  dgamma {ratios['dgamma']:.3g}  dx {ratios['dx']:.3g}")
    return max(r_y, *ratios.values())


def bn_check(n, c, relu, pad, constant_column, seed):
    """One forward (with running statistics) + backward through the raw entry points, each twice (the same bits), under ``bn_compare``."""
    rng = np.random.default_rng([n, c, int(relu), seed])
    x, gamma, beta, dy = bn_input(rng, n, c, constant_column)
    run0 = (rng.normal(size=c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32))
    y, stats, run, yd = bn_forward_gpu(x, gamma, beta, relu, pad, running=run0)
    # the plain entry point and a second call: the same bits
    y2, stats2, _, _ = bn_forward_gpu(x, gamma, beta, relu, pad)
    assert y.tobytes() == y2.tobytes() and stats.tobytes() == stats2.tobytes()
    dx, dgamma, dbeta = bn_backward_gpu(x, yd if relu else None, dy, gamma, stats, pad)
    dx2, dgamma2, dbeta2 = bn_backward_gpu(x, yd if relu else None, dy, gamma, stats, pad)
    assert dx.tobytes() == dx2.tobytes() and dgamma.tobytes() == dgamma2.tobytes() and dbeta.tobytes() == dbeta2.tobytes()
    return bn_compare(x, gamma, beta, dy, relu, constant_column, y, stats, dx, dgamma, dbeta, run0, run, what=f"pad={pad}")


def _constant_columns(c):
    """c >= 8: one tensor has every mean / std ratio AND the constant column (it replaces a ratio-1 column; others remain).  c = 4 has
    four columns for five roles: two tensors, one with the four ratios, one whose ratio-1 column is the constant one."""
    return (c - 3,) if c >= 8 else (None, 1)


@pytest.mark.parametrize("c", [4, 8, 16, 32, 64, 128, 256])
def test_bn_kernels_channel_counts_and_row_counts(c):
    worst = 0.0
    for n in (1, 2, 63, 64, 65, 4097):
        for relu in (False, True):
            for i, const in enumerate(_constant_columns(c)):
                worst = max(worst, bn_check(n, c, relu, 4, const, i))              # ld = c + 4 for x, y, dy and dx
                if n in (2, 65):
                    worst = max(worst, bn_check(n, c, relu, 0, const, 10 + i))     # contiguous rows
    print(f"bn c={c}: worst max err / bound = {worst:.3g}")


@pytest.mark.parametrize("n", [65535, 65536, 65537, 65600])
@pytest.mark.parametrize("c", [4, 64])
def test_bn_kernels_on_the_row_partition_edges(c, n):
    """``bn_blocks`` switches to 1024 workgroups at 65536 rows; past it trailing workgroups start beyond the last row."""
    for relu in (False, True):
        for i, const in enumerate(_constant_columns(c)):
            bn_check(n, c, relu, 4, const, i)


def test_bn_refusals():
    L, lib = _lib()
    rng = np.random.default_rng(3)
    for c, kw in ((12, {}), (512, {}), (32, {"ld_x": 34}), ):
        x = rng.normal(size=(8, c)).astype(np.float32)
        assert bn_forward_gpu(x, np.ones(c, np.float32), np.zeros(c, np.float32), False, 4, expect=L.ERR_INVALID, **kw) == L.ERR_INVALID
    x = rng.normal(size=(100, 32)).astype(np.float32)
    need = lib.eyoc_bn_workspace_bytes(100, 32)
    assert need > 0 and lib.eyoc_bn_workspace_bytes(8, 12) == 0
    assert bn_forward_gpu(x, np.ones(32, np.float32), np.zeros(32, np.float32), False, 0, ws_bytes=need - 1, expect=L.ERR_WORKSPACE) == L.ERR_WORKSPACE


# ================================================================ (d) eyoc_maps_gather_window / _internal

def _gather_cloud(n):
    rng = np.random.default_rng(n)
    if n == 1:
        return np.array([[0, -3, 2, -1]], np.int32)
    half = R.small_cloud(rng, n // 2, lo=-4, hi=4)                       # negative coordinates included
    other = half.copy()
    other[:, 0] = 1                                                      # a second cloud at the SAME xyz: the batch column keeps them apart
    keep = rng.random(len(other)) < 0.8
    extra = R.small_cloud(rng, 40, lo=-4, hi=4)
    extra[:, 0] = 1
    c = np.unique(np.concatenate([half, other[keep], extra]), axis=0)
    rng.shuffle(c)
    return c.astype(np.int32)


@pytest.fixture()
def automatic_row_order():
    """``eyoc_maps_internal_order`` at the library's default (-1: small inputs keep the caller's rows) whatever an earlier test left
    behind - the ctx's switch beats what a build asks for, the caller-ordered second set of maps included.  Restored afterwards."""
    L, lib = _lib()
    prev = lib.eyoc_maps_internal_order(L.ctx(), -1) - 2
    yield
    lib.eyoc_maps_internal_order(L.ctx(), prev)


@pytest.mark.parametrize("cin", [1, 3, 64])
@pytest.mark.parametrize("ks", [1, 3, 5, 7])
def test_gather_window_against_the_restatement(automatic_row_order, ks, cin):
    import eyoc_amd
    L, lib = _lib()
    for n in (1, 300):
        coords = _gather_cloud(n)
        n = len(coords)
        if n > 1:
            xyz0 = {tuple(c[1:]) for c in coords if c[0] == 0}
            assert sum(tuple(c[1:]) in xyz0 for c in coords if c[0] == 1) > 50 and coords[:, 1:].min() < 0
        feats = np.random.default_rng(ks * 100 + cin).normal(size=(n, cin)).astype(np.float32)
        want = R.gather_window(coords, feats, ks).astype(np.float32)
        F, Cd = dev(feats), dev(coords)
        cm = eyoc_amd.SparseTensor(F, coordinates=Cd).coordinate_manager
        assert not lib.eyoc_maps_row_order(cm.maps())
        out = torch.full((n, ks ** 3 * cin), NAN, dtype=torch.float32, device="cuda")
        L.check(lib.eyoc_maps_gather_window(L.ctx(), cm.maps(), ks, L.ptr(F), cin, L.ptr(out), L.stream_ptr()), "eyoc_maps_gather_window")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"caller's rows, n {n}")
        # the same through Z-ordered maps: internal rows in, internal rows out
        prev = lib.eyoc_maps_internal_order(L.ctx(), 1) - 2
        try:
            cmz = eyoc_amd.SparseTensor(F, coordinates=Cd).coordinate_manager
            mz = cmz.maps()
            order = cmz.row_order()
        finally:
            lib.eyoc_maps_internal_order(L.ctx(), prev)
        assert order is not None or n == 1
        order = np.arange(n) if order is None else order.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(n))
        Fz = dev(feats[order])
        out = torch.full((n, ks ** 3 * cin), NAN, dtype=torch.float32, device="cuda")
        L.check(lib.eyoc_maps_gather_window_internal(L.ctx(), mz, ks, L.ptr(Fz), cin, L.ptr(out), L.stream_ptr()), "eyoc_maps_gather_window_internal")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want[order], err_msg=f"internal rows, n {n}")


# ================================================================ (e) one training step on a small batch

SMALL_BATCH_SEED = 0


def test_one_training_step_on_a_small_batch_matches_the_float64_oracle(automatic_row_order):
    """``forward_train`` + backward on two sheets of 200 voxels each (``small_train_batch(0)``: level rows 400 / 164 / 64 / 22), by the
    method of tests/test_gpu_train.py::test_one_sgd_step_matches_the_oracle_under_autograd - the product's ReLU decisions are handed
    to the oracle - with the oracle in FLOAT64.  Bar: features and every parameter gradient within 1e-4 of the tensor's largest entry.
    Condition of the input, measured on the CPU before the seed was fixed: the oracle in float32 and in float64 (same masks, the
    float64 oracle's own) agree within 1.44e-06 on every one of those tensors (worst: block4_tr.norm2.bn.weight; limit 2.5e-5), so the
    bar is not spent on the cloud's own conditioning.  Seeds 0 .. 11 all qualified (1.2e-6 .. 1.8e-6); 0 was taken."""
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    from eyoc_amd.train import forward_train
    from oracle import coords as oc
    from oracle import resunet as orr
    coords, feats, target = R.small_train_batch(SMALL_BATCH_SEED)
    rows = [len(c) for c in oc.build_maps(coords, 5)["cm"]]
    assert len(coords) <= 400 and 16 <= rows[3] <= 64, rows
    sd = syn.make_weights(seed=21)
    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.cuda().train()
    x = eyoc_amd.SparseTensor(dev(feats), coordinates=dev(coords))
    taps = {}
    out = forward_train(model, x, taps)
    (out.F * dev(target)).sum().backward()
    masks = {k: (v.detach() > 0).double().cpu() for k, v in taps.items()}
    assert len(masks) == 15

    sdt = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in sd.items()}
    sdt = {k: (v.double() if v.is_floating_point() else v) for k, v in sdt.items()}
    params = [k for k in sdt if k.endswith(".kernel") or k.endswith("bn.weight") or k.endswith("bn.bias") or k == "final.bias"]
    for k in params:
        sdt[k].requires_grad_(True)
    want = orr.resunet_forward(sdt, coords, feats, train=True, bn_momentum=0.05, dtype=torch.float64, relu_masks=masks)
    (want * torch.from_numpy(target).double()).sum().backward()

    def rel_err(a, b):
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    named = dict(model.named_parameters())
    assert set(named) == set(params)
    errs = {"features": rel_err(out.F.detach().cpu().numpy(), want.detach().numpy())}
    for k in params:
        assert named[k].grad is not None, k
        errs[k] = rel_err(named[k].grad.cpu().numpy().reshape(-1), sdt[k].grad.numpy().reshape(-1))
    worst = max(errs, key=errs.get)
    print(f"small training step, level rows {rows}: features {errs['features']:.2e}, worst {worst} {errs[worst]:.2e}")
    assert errs[worst] < 1e-4, (worst, errs[worst])
