"""Restatement of ``MinkowskiInstanceNorm`` as its source defines it (model/common.py:7-8), of its backward, and of the ResUNetIN2
family's forward (model/resunet.py:229-251: batch norm behind the stage convolutions, instance norm inside every residual block,
model/residual_block.py:60-61).  TEST INFRASTRUCTURE: numpy / torch on the CPU, float64 unless told otherwise, nothing from the
product.  **Parity unpinned**: MinkowskiEngine is not installed, so the contract is the one written here.

For ``x [n, c]`` whose row ``r`` belongs to instance ``ids[r]``, ``n_b`` rows in instance ``b``::

    mean[b] = sum_{r in b} x[r] / n_b,  var[b] = sum_{r in b} (x[r] - mean[b])^2 / n_b   (biased, two passes)
    y[r]    = (x[r] - mean[b]) / sqrt(var[b] + eps) * weight + bias  [+ residual[r]]  [ReLU]
    dx[r]   = weight invstd[b] (g[r] - mean_b(g) - xhat[r] mean_b(g xhat)),  g = dy where the rectified output is positive
    dweight = sum over ALL rows of g xhat,  dbias = sum over ALL rows of g,  dresidual = g
"""
import numpy as np
import torch

IN_EPS = 1e-8


def in_forward(x, ids, n_inst, weight, bias, eps=IN_EPS, relu=False, residual=None):
    """-> ``y [n, c], mean [n_inst, c], var [n_inst, c]`` (float64; rows of ``mean`` / ``var`` of an id without rows are NaN)."""
    x = np.asarray(x, np.float64)
    ids = np.asarray(ids, np.int64)
    w, b = np.asarray(weight, np.float64).reshape(1, -1), np.asarray(bias, np.float64).reshape(1, -1)
    mean = np.full((n_inst, x.shape[1]), np.nan)
    var = np.full((n_inst, x.shape[1]), np.nan)
    y = np.empty_like(x)
    for i in range(n_inst):
        rows = np.flatnonzero(ids == i)
        if len(rows) == 0:
            continue
        mean[i] = x[rows].mean(0)
        var[i] = ((x[rows] - mean[i]) ** 2).mean(0)
        y[rows] = (x[rows] - mean[i]) / np.sqrt(var[i] + eps) * w + b
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return (np.maximum(y, 0.0) if relu else y), mean, var


def in_backward(x, y, dy, ids, n_inst, weight, mean, var, eps=IN_EPS):
    """-> ``dx, dresidual (= g), dweight [c], dbias [c]``.  ``y`` (or ``None``): the rectified output of the forward - ``dy`` counts
    only where ``y > 0``."""
    x, g = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    ids = np.asarray(ids, np.int64)
    w = np.asarray(weight, np.float64).reshape(1, -1)
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.0)
    dx = np.empty_like(x)
    dweight, dbias = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for i in range(n_inst):
        rows = np.flatnonzero(ids == i)
        if len(rows) == 0:
            continue
        invstd = 1.0 / np.sqrt(np.asarray(var[i], np.float64) + eps)
        xhat = (x[rows] - mean[i]) * invstd
        gi = g[rows]
        dx[rows] = w * invstd * (gi - gi.mean(0) - xhat * (gi * xhat).mean(0))
        dweight += (gi * xhat).sum(0)
        dbias += gi.sum(0)
    return dx, g, dweight, dbias


def in_state_dict(sd):
    """A ``synthetic.make_weights`` dict -> the IN model's: every ``block*.norm{1,2}.bn.{weight,bias}`` becomes
    ``block*.norm{1,2}.{weight,bias}`` reshaped to ``[1, c]``; the blocks' ``running_*`` / ``num_batches_tracked`` entries go."""
    out = {}
    for k, v in sd.items():
        if k.startswith("block") and ".bn." in k:
            head, leaf = k.split(".bn.")
            if leaf in ("weight", "bias"):
                out[f"{head}.{leaf}"] = np.asarray(v).reshape(1, -1)
            continue
        out[k] = v
    return out


# ---------------------------------------------------------------- the whole network (torch, differentiable)

def instance_norm_t(x, ids, n_inst, sd, name):
    """The instance norm in torch, in the dtype of ``x``, differentiable with respect to ``x`` and the two parameters."""
    from oracle.resunet import _t
    w, b = _t(sd[f"{name}.weight"]).to(x.dtype).reshape(1, -1), _t(sd[f"{name}.bias"]).to(x.dtype).reshape(1, -1)
    ids = torch.as_tensor(np.asarray(ids, np.int64))
    cnt = torch.bincount(ids, minlength=n_inst).clamp(min=1).to(x.dtype)[:, None]
    mean = torch.zeros((n_inst, x.shape[1]), dtype=x.dtype).index_add(0, ids, x) / cnt
    d = x - mean[ids]
    var = torch.zeros((n_inst, x.shape[1]), dtype=x.dtype).index_add(0, ids, d * d) / cnt
    return d / torch.sqrt(var[ids] + IN_EPS) * w + b


def in_resunet_forward(sd, coords, feats, normalize_feature=True, conv1_kernel_size=5, maps=None, return_intermediate=False,
                       dtype=torch.float64, train=False, bn_momentum=0.1, running_out=None, relu_masks=None):
    """Forward of the ResUNetIN2 family (any channel table - shapes come from ``sd``, an ``in_state_dict``): ``oracle.resunet``'s
    ``sparse_conv``, maps and ``batch_norm`` (eval: running statistics; ``train=True``: batch statistics) for everything but the
    block norms, which are ``instance_norm_t`` in either mode.  ``relu_masks``, ``running_out``, ``return_intermediate`` as in
    ``oracle.resunet.resunet_forward``; returns ``out`` or ``(out, stored, maps)``."""
    from oracle import coords as oc
    from oracle import resunet as orr
    orr._TRAIN.update(on=bool(train), momentum=bn_momentum, running=running_out, masks=relu_masks)
    try:
        if maps is None:
            maps = oc.build_maps(coords, conv1_kernel_size)
        s1, down, up = maps["s1"], maps["down"], maps["up"]
        n_inst = int(np.asarray(coords)[:, 0].max()) + 1
        ids = [cm.coords[:, 0] for cm in maps["cm"]]
        kern = lambda name: orr._kernel(sd, name, dtype)
        stored = {}

        def block(x, lvl, name):
            out = orr.sparse_conv(x, s1[lvl], kern(f"{name}.conv1"))
            out = stored[f"{name}.conv1"] = orr._relu(instance_norm_t(out, ids[lvl], n_inst, sd, f"{name}.norm1"), f"{name}.conv1")
            out = orr.sparse_conv(out, s1[lvl], kern(f"{name}.conv2"))
            out = instance_norm_t(out, ids[lvl], n_inst, sd, f"{name}.norm2")
            out = stored[f"{name}.conv2"] = orr._relu(out + x, f"{name}.conv2")
            return out

        def stage(x, nbr, lvl, i):
            out = orr.batch_norm(orr.sparse_conv(x, nbr, kern(f"conv{i}")), sd, f"norm{i}")
            return block(out, lvl, f"block{i}")

        x = orr._t(feats).to(dtype)
        out_s1 = stage(x, maps["k5"], 0, "1")
        out_s2 = stage(out_s1, down[0], 1, "2")
        out_s4 = stage(out_s2, down[1], 2, "3")
        out_s8 = stage(out_s4, down[2], 3, "4")
        out = stage(out_s8, up[2], 2, "4_tr")
        out = stage(torch.cat([out, out_s4], 1), up[1], 1, "3_tr")
        out = stage(torch.cat([out, out_s2], 1), up[0], 0, "2_tr")
        out = torch.cat([out, out_s1], 1)
        ident = np.arange(out.shape[0], dtype=np.int32)[None, :]
        out = stored["conv1_tr"] = orr._relu(orr.sparse_conv(out, ident, kern("conv1_tr")), "conv1_tr")
        out = orr.sparse_conv(out, ident, kern("final")) + orr._t(sd["final.bias"]).to(dtype).reshape(1, -1)
        if normalize_feature:
            out = out / torch.norm(out, p=2, dim=1, keepdim=True)
        return (out, stored, maps) if return_intermediate else out
    finally:
        orr._TRAIN.update(on=False, running=None, masks=None)
