"""The float64 restatements of tests/train_restatement.py against torch autograd in float64 on the CPU, the host packers of
csrc/spconv_grad.hip alone, and the premise of the bit-equal integer cases of tests/test_gpu_train_kernels.py.  No GPU."""
import numpy as np
import pytest
import torch

import train_restatement as R

RTOL = 1e-12


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * max(float(np.abs(want).max(initial=0.0)), 1e-300))


def _tables():
    rng = np.random.default_rng(7)
    t = R.real_tables(R.small_cloud(rng, 257))
    n0, n1 = t["n"]
    planted, n_in = R.gw_planted_table(n_out=2049, n_in=700)
    return [("s1", t["s1"], n0), ("down", t["down"], n0), ("up", t["up"], n1), ("synthetic", planted[:, :300], n_in), ("identity", None, 40)]


@pytest.mark.parametrize("name,nbr,n_in", _tables(), ids=[t[0] for t in _tables()])
def test_convolution_restatement_against_autograd(name, nbr, n_in):
    from oracle import resunet as orr
    rng = np.random.default_rng(11)
    K = 1 if nbr is None else nbr.shape[0]
    n_out = n_in if nbr is None else nbr.shape[1]
    cin, cout = 5, 7
    x, W, dy = R.float_data(rng, (n_in, cin)), R.float_data(rng, (K, cin, cout)), R.float_data(rng, (n_out, cout))
    xt = torch.from_numpy(x).double().requires_grad_(True)
    Wt = torch.from_numpy(W).double().requires_grad_(True)
    table = np.arange(n_in, dtype=np.int32)[None] if nbr is None else nbr
    out = orr.sparse_conv(xt, table, Wt)
    out.backward(torch.from_numpy(dy).double())
    got, S, P = R.conv_forward(nbr, x, W)
    close(got, out.detach().numpy())
    assert (np.abs(got) <= S * (1 + 1e-12)).all() and P.shape == (n_out, 1)
    assert np.array_equal(P[:, 0], (table >= 0).sum(0) * cin)
    dx, S, P = R.conv_grad_input(nbr, n_in, dy, W)
    close(dx, xt.grad.numpy())
    assert (np.abs(dx) <= S * (1 + 1e-12)).all()
    assert np.array_equal(P[:, 0], np.bincount(table[table >= 0], minlength=n_in) * cout)
    dW, S, P = R.conv_grad_weight(nbr, x, dy)
    close(dW, Wt.grad.numpy())
    assert (np.abs(dW) <= S * (1 + 1e-12)).all()
    assert np.array_equal(P[:, 0, 0], (table >= 0).sum(1))


@pytest.mark.parametrize("n,c,relu", [(2, 4, False), (63, 8, True), (257, 32, True), (1000, 16, False)])
def test_batch_norm_restatement_against_torch(n, c, relu):
    rng = np.random.default_rng(n + c)
    x = rng.normal(0.5, 1.5, (n, c)) + rng.normal(size=c) * 10
    gamma, beta, dy = rng.uniform(0.5, 1.5, c), rng.normal(size=c), rng.normal(size=(n, c))
    xt, gt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, gamma, beta))
    ref = torch.nn.functional.batch_norm(xt, None, None, gt, bt, training=True, eps=1e-5)
    if relu:
        ref = torch.relu(ref)
    ref.backward(torch.from_numpy(dy))
    y, mean, var = R.bn_forward(x, gamma, beta, 1e-5, relu)
    close(y, ref.detach().numpy())
    close(mean, x.mean(0))
    close(var, x.var(0))
    dx, dgamma, dbeta = R.bn_backward(x, y if relu else None, dy, gamma, mean, var, 1e-5)
    close(dx, xt.grad.numpy())
    close(dgamma, gt.grad.numpy())
    close(dbeta, bt.grad.numpy())
    # running statistics like nn.BatchNorm1d (momentum 0.05, unbiased variance)
    bn = torch.nn.BatchNorm1d(c, momentum=0.05).double()
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(rng.normal(size=c)))
        bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, c)))
    rm0, rv0 = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    bn.train()(torch.from_numpy(x))
    rm, rv = R.bn_running(rm0, rv0, mean, var, n, 0.05)
    close(rm, bn.running_mean.numpy())
    close(rv, bn.running_var.numpy())


def test_batch_norm_restatement_single_row():
    """n = 1: the variance is zero, y = beta, the unbiased factor is n / max(n - 1, 1) = 1 (torch raises there)."""
    x = np.array([[3.0, -2.0, 0.5, 7.0]])
    gamma, beta = np.array([1.0, 2.0, 3.0, 4.0]), np.array([0.5, -0.5, 0.0, 1.0])
    y, mean, var = R.bn_forward(x, gamma, beta, 1e-5, False)
    assert np.array_equal(y[0], beta) and np.array_equal(mean, x[0]) and not var.any()
    rm, rv = R.bn_running(np.zeros(4), np.ones(4), mean, var, 1, 0.05)
    close(rm, 0.05 * x[0])
    close(rv, np.full(4, 0.95))
    dx, dgamma, dbeta = R.bn_backward(x, None, np.ones((1, 4)), gamma, mean, var, 1e-5)
    assert not dx.any() and not dgamma.any() and np.array_equal(dbeta, np.ones(4))


def test_gather_window_restatement():
    rng = np.random.default_rng(5)
    coords = R.small_cloud(rng, 60, batches=2, lo=-2, hi=2)
    feats = rng.normal(size=(60, 3))
    from oracle import coords as oc
    cm = oc.CoordMap(coords, 1)
    for ks in (1, 3, 5):
        nbr = oc.kernel_map(cm, cm, ks)                       # [ks^3, n]: x fastest
        want = np.where((nbr >= 0).T[:, :, None], feats[np.maximum(nbr, 0).T], 0.0).reshape(60, -1)
        assert np.array_equal(R.gather_window(coords, feats, ks), want)
    assert np.array_equal(R.gather_window(coords, feats, 1), feats)


@pytest.mark.parametrize("K,cin,cout", [(27, 32, 64), (27, 256, 32), (1, 96, 64), (27, 192, 128)])
@pytest.mark.parametrize("mirror", [0, 1])
def test_transposed_packer_is_the_plain_packer_of_the_transposed_kernel(K, cin, cout, mirror):
    """``eyoc_spconv_pack_weights_transposed(w, K, cin, cout, mirror)`` = ``eyoc_spconv_pack_weights`` of ``V[k] = W[K-1-k if mirror
    else k].T`` (a [K, cout, cin] kernel).  The plain packer wants C_out' = cin in {32, 64, 128, 256}: 96 and 192 are refused by both."""
    from eyoc_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(K * 1000 + cin + cout + mirror)
    W = rng.normal(size=(K, cin, cout)).astype(np.float32)
    V = np.ascontiguousarray(np.stack([W[K - 1 - k if mirror else k].T for k in range(K)]))
    got, want = np.full(W.size, np.nan, np.float32), np.full(W.size, np.nan, np.float32)
    rc_t = lib.eyoc_spconv_pack_weights_transposed(W.ctypes.data, K, cin, cout, mirror, got.ctypes.data)
    rc_p = lib.eyoc_spconv_pack_weights(V.ctypes.data, None, K, cout, cin, want.ctypes.data)
    assert rc_t == rc_p
    if cin in (32, 64, 128, 256):
        assert rc_t == 0 and np.array_equal(got, want) and np.array_equal(np.sort(got), np.sort(W.reshape(-1)))
    else:
        assert rc_t == _lib.ERR_INVALID and np.isnan(got).all()


def _integer_results():
    """Every integer case of the GPU tests -> the float64 results that must be exactly representable."""
    for cin, cout in R.GW_PAIRS_NINE + R.GW_PAIRS_WIDE:
        for n_out in R.gw_sizes(cin, cout):
            nbr, x, dy = R.gw_case(cin, cout, n_out, True)
            yield f"grad_weight {cin}x{cout} n={n_out}", R.conv_grad_weight(nbr, x, dy)[0]
    nbr, x, dy = R.gw_case(256, 256, 9217, True, density=3 / 27)
    yield "grad_weight 256x256 n=9217", R.conv_grad_weight(nbr, x, dy)[0]
    for n_out in R.SUM_SIZES_256:
        yield f"sum 32x256 n={n_out}", R.conv_forward(*R.sum_case(32, 256, n_out))[0]
    for cin, cout in R.SUM_SHAPES_NARROW:
        for n_out in R.SUM_SIZES_NARROW:
            yield f"sum {cin}x{cout} n={n_out}", R.conv_forward(*R.sum_case(cin, cout, n_out))[0]
    for empty in (tuple(range(0, 7)), tuple(range(20, 27))):
        yield f"sum empty {empty[0]}..{empty[-1]}", R.conv_forward(*R.sum_case(32, 256, 100, empty))[0]


def test_integer_cases_are_exact_in_fp32():
    """The premise of ``assert_array_equal`` on the GPU: operands -4 .. 4 make every product and partial sum an integer; the results
    (hence, all partial sums being bounded by the sum of absolute values, which is checked instead where it is cheap) stay below 2^24."""
    count = 0
    for name, value in _integer_results():
        assert R.exactly_fp32(value), name
        assert np.array_equal(value, np.round(value)), name
        count += 1
    assert count >= 100
    # the worst conceivable partial sum: 16 (the largest product) times the number of products of an entry
    nbr, x, dy = R.gw_case(256, 256, 9217, True, density=3 / 27)
    assert 16 * int((nbr >= 0).sum(1).max()) < 2 ** 24
    assert 16 * 27 * 256 < 2 ** 24                         # a forward / input-gradient entry: at most K * C products
    assert 16 * 2049 < 2 ** 24                             # a weight-gradient entry of the size sweep: at most n_out pairs


def test_generated_tables_have_the_properties_the_gpu_cases_name():
    nbr, n_in = R.gw_planted_table()                       # asserts its own patterns
    assert nbr.shape == (27, 2049) and n_in == 700
    assert R.grad_weight_rows_per_block(1025, 27, 32, 32) == (2, 576)
    assert R.grad_weight_rows_per_block(2049, 27, 32, 32) == (3, 704)
    assert R.grad_weight_rows_per_block(9217, 27, 256, 256)[0] == 5        # cdiv(9217, 1024) = 10, halved
    assert [R.offset_split(n, 256) for n in R.SUM_SIZES_256] == [4, 4, 4, 4, 4, 3, 3, 2, 2, 1]
    for empty in (tuple(range(0, 7)), tuple(range(20, 27))):
        nbr = R.sum_case(32, 256, 100, empty)[0]
        assert (nbr[list(empty)] < 0).all() and R.offset_split(100, 256) == 4
        # share z of four walks the offsets [27 z / 4, 27 (z + 1) / 4): the first is 0..5, the last 20..26
        assert 27 * 1 // 4 == 6 and 27 * 3 // 4 == 20
    for n in R.SUM_SIZES_256[4:]:
        per_row = (R.sum_case(32, 256, n)[0] >= 0).sum() / n
        assert 2.5 < per_row < 3.5
