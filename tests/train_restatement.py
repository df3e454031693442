"""Plain float64 restatements of the training-side device code (csrc/spconv_grad.hip, the operator behind ``eyoc_spconv_sum``,
csrc/bn.hip) and the random inputs their tests share.  numpy only: no torch autograd, no ``eyoc_amd`` import.  Pinned against torch
autograd in float64 by tests/test_train_restatement_host.py; tests/test_gpu_train_kernels.py compares the kernels with it.

The convolution functions return three things: the value, the sum of the absolute values of the products that went into every
entry (``S``) and the number of those products (``P``, broadcastable to the value).  ``(P + 2) * 2^-24 * S`` bounds the error of an
fp32 sum of ``P`` products taken in any order (one rounding per product, ``P - 1`` additions, one store)."""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32


# ---------------------------------------------------------------- sparse convolution: out[o] = sum_k x[nbr[k][o]] W[k]

def _identity(n):
    return np.arange(n, dtype=np.int32)[None, :]


def conv_forward(nbr, x, W):
    """``out [n_out, cout]``, ``S``, ``P [n_out, 1]``.  ``nbr = None``: the identity map with ``K = 1``."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    if nbr is None:
        nbr = _identity(x.shape[0])
    K, n_out = nbr.shape
    out, S = np.zeros((n_out, W.shape[2])), np.zeros((n_out, W.shape[2]))
    P = np.zeros((n_out, 1), np.int64)
    ax, aW = np.abs(x), np.abs(W)
    for k in range(K):
        o = np.flatnonzero(nbr[k] >= 0)
        if o.size == 0:
            continue
        i = nbr[k][o]
        out[o] += x[i] @ W[k]               # (an output row occurs once per offset: plain fancy-index += is exact)
        S[o] += ax[i] @ aW[k]
        P[o, 0] += x.shape[1]
    return out, S, P


def conv_grad_input(nbr, n_in, dy, W):
    """``dx [n_in, cin]`` = d/dx of ``sum(out * dy)``: ``dx[nbr[k][o]] += dy[o] W[k]^T``; ``S``; ``P [n_in, 1]``."""
    dy, W = np.asarray(dy, np.float64), np.asarray(W, np.float64)
    if nbr is None:
        nbr = _identity(dy.shape[0])
    K = nbr.shape[0]
    dx, S = np.zeros((n_in, W.shape[1])), np.zeros((n_in, W.shape[1]))
    P = np.zeros((n_in, 1), np.int64)
    ady, aW = np.abs(dy), np.abs(W)
    for k in range(K):
        o = np.flatnonzero(nbr[k] >= 0)
        if o.size == 0:
            continue
        i = nbr[k][o]
        np.add.at(dx, i, dy[o] @ W[k].T)    # (a synthetic table may name an input row twice under one offset)
        np.add.at(S, i, ady[o] @ aW[k].T)
        np.add.at(P[:, 0], i, dy.shape[1])
    return dx, S, P


def conv_grad_weight(nbr, x, dy):
    """``dW [K, cin, cout]`` with ``dW[k] = sum over the pairs of offset k of x[i]^T dy[o]``; ``S``; ``P [K, 1, 1]`` (pairs per offset)."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    if nbr is None:
        nbr = _identity(dy.shape[0])
    K = nbr.shape[0]
    dW, S = np.zeros((K, x.shape[1], dy.shape[1])), np.zeros((K, x.shape[1], dy.shape[1]))
    P = np.zeros((K, 1, 1), np.int64)
    for k in range(K):
        o = np.flatnonzero(nbr[k] >= 0)
        if o.size == 0:
            continue
        i = nbr[k][o]
        dW[k] = x[i].T @ dy[o]
        S[k] = np.abs(x[i]).T @ np.abs(dy[o])
        P[k] = o.size
    return dW, S, P


def rounding_bound(S, P):
    """``(P + 2) u S``: a length-``P`` fp32 sum in any order, one rounding each for the product and the final store."""
    return (P + 2) * U32 * S


# ---------------------------------------------------------------- batch norm with batch statistics (header comment of bn.hip)

def bn_forward(x, gamma, beta, eps, relu):
    """``y, mean, biased var``: ``y = (x - mean) / sqrt(var + eps) * gamma + beta`` (+ ReLU); the variance two-pass in float64."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    y = (x - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return (np.maximum(y, 0.0) if relu else y), mean, var


def bn_backward(x, y, dy, gamma, mean, var, eps):
    """``dx, dgamma, dbeta``.  ``y`` (or ``None``): the rectified output of the forward - ``dy`` counts only where ``y > 0``.
    ``dx = gamma / sigma * (dy - mean(dy) - xhat * mean(dy * xhat))``, ``dgamma = sum dy * xhat``, ``dbeta = sum dy``."""
    x, g = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n = x.shape[0]
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.0)
    invstd = 1.0 / np.sqrt(np.asarray(var, np.float64) + eps)
    xhat = (x - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dx = np.asarray(gamma, np.float64) * invstd * (g - dbeta / n - xhat * dgamma / n)
    return dx, dgamma, dbeta


def bn_running(run_mean, run_var, mean, var, n, momentum):
    """``nn.BatchNorm1d``'s update: ``running = (1 - m) running + m batch`` with the variance unbiased by ``n / max(n - 1, 1)`` (the
    kernel's documented ``n = 1`` behaviour: the biased zero is kept; torch raises there)."""
    unbiased = np.asarray(var, np.float64) * (n / max(n - 1, 1))
    return ((1.0 - momentum) * np.asarray(run_mean, np.float64) + momentum * np.asarray(mean, np.float64),
            (1.0 - momentum) * np.asarray(run_var, np.float64) + momentum * unbiased)


# ---------------------------------------------------------------- the first convolution's window gather

def gather_window(coords, feats, ks):
    """``G [n, ks^3 * cin]``: ``G[row][k * cin + ci]`` = feature ``ci`` of the voxel at window offset ``k`` of the row's own batch, or
    0; offsets enumerate x fastest.  ``coords int [n, 4]`` = (b, x, y, z)."""
    coords, feats = np.asarray(coords), np.asarray(feats, np.float64)
    n, cin = feats.shape
    where = {tuple(int(v) for v in c): i for i, c in enumerate(coords)}
    assert len(where) == n, "duplicate coordinates"
    r = ks // 2
    G = np.zeros((n, ks ** 3 * cin))
    for row, (b, x, y, z) in enumerate(coords):
        k = 0
        for dz in range(-r, r + 1):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    i = where.get((int(b), int(x) + dx, int(y) + dy, int(z) + dz))
                    if i is not None:
                        G[row, k * cin:(k + 1) * cin] = feats[i]
                    k += 1
    return G


# ---------------------------------------------------------------- inputs

def integer_data(rng, shape):
    """Integers -4 .. 4, about 30 % zeros, as float32: every product and partial sum of the cases built from them is an integer far
    below 2^24, so fp32 arithmetic on them is exact in any order."""
    v = rng.integers(1, 5, size=shape) * rng.choice((-1, 1), size=shape)
    return np.where(rng.random(shape) < 0.3, 0, v).astype(np.float32)


def float_data(rng, shape):
    """N(0, 1) times a per-column log-uniform scale in [1e-2, 1e2], as float32."""
    scale = 10.0 ** rng.uniform(-2.0, 2.0, size=shape[-1])
    return (rng.normal(size=shape) * scale).astype(np.float32)


def small_cloud(rng, n, batches=1, lo=-6, hi=6):
    """``int32 [n, 4]`` unique (b, x, y, z) in a small box around the origin (negative coordinates included), shuffled."""
    side = hi - lo
    while side ** 3 * batches < 2 * n:
        hi += 1
        side = hi - lo
    flat = rng.permutation(batches * side ** 3)[:n]
    b, rest = flat // side ** 3, flat % side ** 3
    c = np.stack([b, rest % side + lo, (rest // side) % side + lo, rest // (side * side) + lo], 1)
    return c.astype(np.int32)


def real_tables(coords):
    """Rulebooks of a small cloud through ``oracle.coords``: ``{"s1": [27, n0] (n_in = n0), "down": [27, n1] (n_in = n0),
    "up": [27, n0] (n_in = n1), "n": (n0, n1)}`` - the stride-1 table of level 0 and the two tables of the first level boundary."""
    from oracle import coords as oc
    cm0 = oc.CoordMap(np.asarray(coords), 1)
    cm1 = oc.stride_map(cm0, 2)[0]
    return {"s1": oc.kernel_map(cm0, cm0, 3), "down": oc.kernel_map(cm0, cm1, 3), "up": oc.transposed_kernel_map(cm1, cm0, 3),
            "n": (len(cm0), len(cm1))}


def synthetic_table(rng, K, n_out, n_in, density=0.3, empty_offsets=(), empty_row_fraction=0.0, empty_block=None):
    """``int32 [K, n_out]`` with entries in ``[0, n_in)`` or -1: every (offset, row) holds a pair with probability ``density``; the
    offsets in ``empty_offsets`` hold none; a fraction of the rows has no neighbour under any offset; ``empty_block = (k, r0, r1)``
    empties the rows ``[r0, r1)`` of offset ``k``."""
    nbr = rng.integers(0, max(n_in, 1), size=(K, n_out)).astype(np.int32)
    nbr[rng.random((K, n_out)) >= density] = -1
    for k in empty_offsets:
        nbr[k] = -1
    if empty_row_fraction > 0 and n_out > 0:
        nbr[:, rng.random(n_out) < empty_row_fraction] = -1
    if empty_block is not None:
        k, r0, r1 = empty_block
        nbr[k, r0:r1] = -1
    return nbr


def sparse_table(rng, K, n_out, n_in, per_row=3, empty_offsets=()):
    """About ``per_row`` neighbours per output row, spread over the offsets not listed in ``empty_offsets``."""
    live = [k for k in range(K) if k not in set(empty_offsets)]
    nbr = synthetic_table(rng, K, n_out, n_in, density=per_row / len(live))
    for k in empty_offsets:
        nbr[k] = -1
    return nbr


def batch_pair_counts(nbr, rows_per_block):
    """Pair counts of the 64-row batches a wave of ``k_grad_weight`` ballots: per offset, per row block of ``rows_per_block`` rows (a
    multiple of 64), the aligned 64-row pieces of the block."""
    K, n_out = nbr.shape
    counts = []
    for k in range(K):
        for r0 in range(0, n_out, rows_per_block):
            r1 = min(n_out, r0 + rows_per_block)
            for b in range(r0, r1, 64):
                counts.append(int((nbr[k, b:min(b + 64, r1)] >= 0).sum()))
    return np.asarray(counts)


# ---------------------------------------------------------------- the cases both test files walk

GW_PAIRS_NINE = [(a, b) for a in (16, 32, 64) for b in (16, 32, 64)]           # ti / tj of 1, 2 and 4: every k_grad_weight<TI,TJ>
GW_PAIRS_WIDE = [(48, 96), (96, 48), (192, 64), (64, 192), (128, 256)]         # several channel tiles in grid.z
# the four-pair MFMA step (1 3 4 5), a wave's 64-row batch (63 64 65), the four waves of a workgroup (255 256 257), the 1024-row
# block (1023 1024 1025: two blocks of 576 rows; 2049: three of 704)
GW_SIZES_ALL = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
GW_SIZES_SOME = [1, 5, 65, 257, 1025, 2049]


def gw_sizes(cin, cout):
    return GW_SIZES_ALL if (cin, cout) == (32, 32) else GW_SIZES_SOME


def grad_weight_rows_per_block(n_out, K, cin, cout):
    """Row blocks of one ``eyoc_spconv_grad_weight`` launch as ``grad_weight_blocks`` of spconv_grad.hip lays them out: ``(blocks,
    rows per block)``.  Used only to ASSERT properties of generated tables (which batches a wave sees); the kernel is not asked."""
    ti = 4 if cin % 64 == 0 else 2 if cin % 32 == 0 else 1
    tj = 4 if cout % 64 == 0 else 2 if cout % 32 == 0 else 1
    per = K * (cin // (16 * ti)) * (cout // (16 * tj))
    nb = min(-(-n_out // 1024), 64)
    while nb > 1 and nb * per > 4096:
        nb >>= 1
    nb = max(nb, 1)
    return nb, -(-(-(-n_out // nb)) // 64) * 64


def gw_case(cin, cout, n_out, integer, K=27, density=0.3, seed=0):
    """One weight-gradient case over a random table with an arbitrary ``n_in``: ``nbr, x [n_in, cin], dy [n_out, cout]``."""
    rng = np.random.default_rng([cin, cout, n_out, int(integer), K, seed])
    n_in = max(1, (n_out * 2) // 3 + 1)
    nbr = synthetic_table(rng, K, n_out, n_in, density)
    draw = integer_data if integer else float_data
    return nbr, draw(rng, (n_in, cin)), draw(rng, (n_out, cout))


def gw_planted_table(cin=32, cout=32, n_out=2049, n_in=700, K=27, seed=3):
    """The synthetic table of the weight-gradient test with the planted patterns, each ASSERTED: an offset without any pair, rows
    without a neighbour, a whole row block of one offset empty, and 64-row batches whose pair count leaves every remainder mod 4."""
    rng = np.random.default_rng(seed)
    nb, rpb = grad_weight_rows_per_block(n_out, K, cin, cout)
    assert nb >= 2
    nbr = synthetic_table(rng, K, n_out, n_in, 0.3, empty_offsets=(5,), empty_row_fraction=0.1, empty_block=(11, rpb, 2 * rpb))
    assert (nbr[5] < 0).all() and (nbr[11] >= 0).any()
    assert ((nbr >= 0).sum(0) == 0).any() and ((nbr >= 0).sum(0) > 0).any()
    assert (nbr[11, rpb:2 * rpb] < 0).all() and (nbr[11, :rpb] >= 0).any()
    counts = batch_pair_counts(nbr, rpb)
    assert {1, 2, 3} <= set((counts % 4).tolist()), "pair counts with P % 4 in {1, 2, 3} must all occur"
    assert nbr.max() < n_in
    return nbr, n_in


# eyoc_spconv_sum on the workgroup-tiled kernel splits the 27 offsets over z workgroups per row tile where
# wgs = cdiv(n_out, 32) * (cout / spconv_ct(cout)) leaves room: z = 4 while 4 wgs <= 2048, 3 while 3 wgs <= 2048, 2 while
# 2 wgs <= 2048 (launch_spconv in spconv.hip).  With cout = 256 (two column tiles) the rule changes at wgs = 512 / 682 / 1024,
# i.e. between n_out = 8192 | 8193, 10912 | 10913 and 16384 | 16385.  A CHANGE OF THAT RULE MUST BE FOLLOWED BY A CHANGE OF THESE SIZES.
SUM_SIZES_256 = [1, 31, 32, 33, 8192, 8193, 10912, 10913, 16384, 16385]
SUM_SIZES_NARROW = [1, 33, 8193]
SUM_SHAPES_NARROW = [(64, 32), (256, 64)]


def offset_split(n_out, cout):
    """The launcher's rule restated (see the comment above): shares per row tile."""
    wgs = -(-n_out // 32) * (cout // min(cout, 128))
    return 4 if wgs * 4 <= 2048 else 3 if wgs * 3 <= 2048 else 2 if wgs * 2 <= 2048 else 1


def sum_case(cin, cout, n_out, empty_offsets=(), seed=0):
    """Integer forward case at about three neighbours per row: ``nbr [27, n_out], x [n_in, cin], W [27, cin, cout]``."""
    rng = np.random.default_rng([cin, cout, n_out, len(empty_offsets), sum(empty_offsets), seed])
    n_in = max(1, (n_out * 3) // 4 + 1)
    nbr = sparse_table(rng, 27, n_out, n_in, 3, empty_offsets)
    return nbr, integer_data(rng, (n_in, cin)), integer_data(rng, (27, cin, cout))


def exactly_fp32(a):
    """The premise of the bit-equal integer cases: the float64 result survives a float32 round trip and stays below 2^24."""
    a = np.asarray(a, np.float64)
    return bool((a.astype(np.float32).astype(np.float64) == a).all() and (np.abs(a).max(initial=0.0) < 2.0 ** 24))


def plane_cloud(rng):
    """``int32 [<= 200, 3]``: a noisy tilted 20 x 10 voxel sheet around the origin (a surface, as a scan's voxels are: every voxel has
    stride-1 neighbours, and the sheet spans a few cells of every coarser level)."""
    a, b = rng.uniform(-0.6, 0.6, 2)
    i, j = np.meshgrid(np.arange(20), np.arange(10), indexing="ij")
    z = np.round(a * i + b * j + rng.normal(0, 0.4, i.shape)).astype(np.int64)
    return np.unique(np.stack([i.ravel() - 10, j.ravel() - 5, z.ravel()], 1), axis=0).astype(np.int32)


def small_train_batch(seed):
    """Two sheets in one batch: ``coords int32 [n, 4]``, ``feats f32 [n, 1]`` in [0.5, 1.5], ``target f32 [n, 32]`` (the loss is
    ``sum(F * target)``)."""
    rng = np.random.default_rng(seed)
    clouds = [plane_cloud(rng), plane_cloud(rng)]
    coords = np.concatenate([np.concatenate([np.full((len(c), 1), b, np.int32), c], 1) for b, c in enumerate(clouds)], 0)
    feats = rng.uniform(0.5, 1.5, size=(len(coords), 1)).astype(np.float32)
    target = rng.normal(size=(len(coords), 32)).astype(np.float32)
    return coords, feats, target
