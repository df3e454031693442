"""The oracle forward (oracle/resunet.py) of EVERY channel table against a dense restatement built from ``torch.nn.functional``'s
``conv3d`` / ``conv_transpose3d``: the oracle is what tests/test_gpu_channel_tables.py judges the device by, so it is pinned first.
CPU only.

A sparse convolution is the dense one restricted to the occupied sites: the dense network below multiplies every layer's output by
the occupancy mask of its level (a voxel's coarse parent is ``floor(c / 2)``), so what it carries is the sparse tensor scattered
into a box.  Concatenation order ([decoder | skip], ``ME.cat`` in model/resunet.py:170-184) and the concat widths are read off the
class tables, not off the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import resunet as orr
from channel_tables import EXPECT, TABLES, expected_from_channels, features, weights
from test_oracle_sparse import dense_weight

BOX = 16          # coordinates in [0, 16): levels of 16, 8, 4, 2 sites per axis


def cloud300():
    rng = np.random.default_rng(8)
    c = np.unique(rng.integers(0, BOX, size=(330, 3)), axis=0)
    rng.shuffle(c)
    c = c[:300]
    assert len(c) == 300
    return np.concatenate([np.zeros((300, 1), np.int64), c], 1).astype(np.int32)


def dense_forward(sd, coords, feats, ks, normalize):
    """ResUNet2.forward (model/resunet.py:142-193) on dense [1, C, z, y, x] tensors in float64."""
    t = lambda k: torch.from_numpy(np.asarray(sd[k])).double()
    c = coords[:, 1:].astype(np.int64)
    masks = []
    for l in range(4):
        n = BOX >> l
        m = torch.zeros((1, 1, n, n, n), dtype=torch.float64)
        q = c >> l
        m[0, 0, q[:, 2], q[:, 1], q[:, 0]] = 1.0
        masks.append(m)

    def bn(x, name):
        s = t(f"{name}.bn.weight") / torch.sqrt(t(f"{name}.bn.running_var") + orr.BN_EPS)
        b = t(f"{name}.bn.bias") - t(f"{name}.bn.running_mean") * s
        return x * s.view(1, -1, 1, 1, 1) + b.view(1, -1, 1, 1, 1)

    def conv(x, name, k=3, stride=1):
        return TF.conv3d(x, dense_weight(t(f"{name}.kernel"), k), stride=stride, padding=k // 2)

    def up(x, name):
        W = t(f"{name}.kernel")
        w = W.reshape(3, 3, 3, W.shape[1], W.shape[2]).permute(3, 4, 0, 1, 2).contiguous()      # [cin, cout, kz, ky, kx]
        return TF.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)

    def block(x, name, m):
        y = torch.relu(bn(conv(x, f"{name}.conv1"), f"{name}.norm1")) * m
        y = bn(conv(y, f"{name}.conv2"), f"{name}.norm2") * m
        return torch.relu(y + x)

    x = torch.zeros((1, feats.shape[1], BOX, BOX, BOX), dtype=torch.float64)
    x[0, :, c[:, 2], c[:, 1], c[:, 0]] = torch.from_numpy(feats).double().t()
    m0, m1, m2, m3 = masks
    s1 = block(bn(conv(x, "conv1", ks), "norm1") * m0, "block1", m0)
    s2 = block(bn(conv(s1, "conv2", stride=2), "norm2") * m1, "block2", m1)
    s4 = block(bn(conv(s2, "conv3", stride=2), "norm3") * m2, "block3", m2)
    s8 = block(bn(conv(s4, "conv4", stride=2), "norm4") * m3, "block4", m3)
    widths = {}
    d4 = block(bn(up(s8, "conv4_tr"), "norm4_tr") * m2, "block4_tr", m2)
    cat4 = torch.cat([d4, s4], 1)
    d2 = block(bn(up(cat4, "conv3_tr"), "norm3_tr") * m1, "block3_tr", m1)
    cat2 = torch.cat([d2, s2], 1)
    d1 = block(bn(up(cat2, "conv2_tr"), "norm2_tr") * m0, "block2_tr", m0)
    cat1 = torch.cat([d1, s1], 1)
    widths.update(cat4=(d4.shape[1], s4.shape[1]), cat2=(d2.shape[1], s2.shape[1]), cat1=(d1.shape[1], s1.shape[1]))
    rows = cat1[0, :, c[:, 2], c[:, 1], c[:, 0]].t()
    h = torch.relu(rows @ t("conv1_tr.kernel"))
    out = h @ t("final.kernel") + t("final.bias").reshape(1, -1)
    if normalize:
        out = out / torch.norm(out, p=2, dim=1, keepdim=True)
    return out.numpy(), widths


@pytest.mark.parametrize("name", list(TABLES))
def test_expectation_table_agrees_with_the_class_tables(name):
    """The widths written down in channel_tables.EXPECT are the ones the class tables imply - in oracle.resunet.CHANNEL_TABLES and in
    eyoc_amd.model alike - and the state dict has them, with the decoder's columns in front of the skip's."""
    import eyoc_amd
    cls, C, T, cin, cout, ks, _seed = TABLES[name]
    assert orr.CHANNEL_TABLES[cls] == (C, T)
    M = eyoc_amd.load_model(cls)
    assert tuple(M.CHANNELS) == C and tuple(M.TR_CHANNELS) == T
    _conv1, up_blocks, tail, fused, c_block1, c_block2_tr = EXPECT[name]
    assert (up_blocks, tail, fused, c_block1, c_block2_tr) == expected_from_channels(name)
    sd = weights(name)
    assert sd["conv1.kernel"].shape == (ks ** 3, cin, C[1])
    assert sd["conv4_tr.kernel"].shape == (27, C[4], T[4])
    assert sd["conv3_tr.kernel"].shape == (27, T[4] + C[3], T[3])            # [decoder | skip]
    assert sd["conv2_tr.kernel"].shape == (27, T[3] + C[2], T[2])
    assert sd["conv1_tr.kernel"].shape == (T[2] + C[1], T[1]) == tail[:2]
    assert sd["final.kernel"].shape == (T[1], cout)
    assert sd["block1.conv1.kernel"].shape == (27, c_block1, c_block1)
    assert sd["block2_tr.conv2.kernel"].shape == (27, c_block2_tr, c_block2_tr)


@pytest.mark.parametrize("name", list(TABLES))
def test_oracle_forward_equals_the_dense_network(name):
    cls, C, T, cin, cout, ks, _seed = TABLES[name]
    coords = cloud300()
    feats = features(name, len(coords))
    sd = weights(name)
    for normalize in (False, True):
        got = orr.resunet_forward(sd, coords, feats, normalize_feature=normalize, conv1_kernel_size=ks, dtype=torch.float64).numpy()
        want, widths = dense_forward(sd, coords, feats, ks, normalize)
        assert widths == dict(cat4=(T[4], C[3]), cat2=(T[3], C[2]), cat1=(T[2], C[1]))
        assert got.shape == want.shape == (300, cout) and np.isfinite(want).all()
        # both in float64: what is left is summation order
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    # (`want` is the unit-norm answer from here on)
    # the skip really is the SECOND part of every concat: swapping the halves of conv1_tr's rows changes the answer
    swapped = dict(sd)
    k = sd["conv1_tr.kernel"]
    swapped["conv1_tr.kernel"] = np.concatenate([k[T[2]:], k[:T[2]]], 0)
    other = orr.resunet_forward(swapped, coords, feats, conv1_kernel_size=ks, dtype=torch.float64).numpy()
    assert np.abs(other - want).max() > 1e-3
    # and the fp32 oracle the device is judged by agrees with its fp64 self far inside the 1e-4 bar
    f32 = orr.resunet_forward(sd, coords, feats, conv1_kernel_size=ks).numpy()
    assert np.abs(f32 - want).max() <= 1e-5
