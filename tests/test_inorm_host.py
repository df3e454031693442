"""The ResUNetIN2 family on the host: the instance-norm restatement (tests/inorm_restatement.py) against torch in float64, and the
model zoo's surface - ``load_model`` finds the five IN classes with the reference's bases and channel tables (model/resunet.py:229-251),
their ``state_dict`` carries MinkowskiInstanceNorm's names, and the packed eval plan refuses them.  No GPU."""
import numpy as np
import pytest
import torch

import inorm_restatement as IR

IN_NAMES = ["ResUNetIN2", "ResUNetIN2B", "ResUNetIN2C", "ResUNetIN2D", "ResUNetIN2E"]
# model/resunet.py:229-251: base class, then the base's tables (:12-13, :196-219)
REFERENCE = {
    "ResUNetIN2": ("ResUNet2", [None, 32, 64, 128, 256], [None, 32, 64, 64, 128]),
    "ResUNetIN2B": ("ResUNetBN2B", [None, 32, 64, 128, 256], [None, 64, 64, 64, 64]),
    "ResUNetIN2C": ("ResUNetBN2C", [None, 32, 64, 128, 256], [None, 64, 64, 64, 128]),
    "ResUNetIN2D": ("ResUNetBN2D", [None, 32, 64, 128, 256], [None, 64, 64, 128, 128]),
    "ResUNetIN2E": ("ResUNetBN2E", [None, 128, 128, 128, 256], [None, 64, 128, 128, 128]),
}


def cases():
    """(name, x, ids, n_inst): instances of 1, 2 and many rows, interleaved ids, an id with no rows, a constant column."""
    rng = np.random.default_rng(0)
    c = 8
    out = []
    ids = np.array([0] * 1 + [1] * 2 + [3] * 40)                       # id 2 has no rows
    out.append(("grouped", rng.normal(1.0, 2.0, (len(ids), c)), ids, 4))
    ids = rng.permutation(np.array([0] * 1 + [1] * 2 + [2] * 57 + [4] * 33))
    x = rng.normal(-3.0, 0.5, (len(ids), c))
    x[:, 5] = 2.25                                                      # a constant column: var = 0 in every instance
    out.append(("interleaved", x, ids, 6))
    out.append(("single", rng.normal(size=(17, c)), np.zeros(17, np.int64), 1))
    return out


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_restatement_against_torch(relu, with_res):
    for name, x, ids, n_inst in cases():
        rng = np.random.default_rng(len(ids))
        n, c = x.shape
        w, b = rng.uniform(0.5, 1.5, (1, c)), rng.normal(size=(1, c))
        res = rng.normal(size=(n, c)) if with_res else None
        dy = rng.normal(size=(n, c))
        y, mean, var = IR.in_forward(x, ids, n_inst, w, b, relu=relu, residual=res)
        xt = torch.from_numpy(x).requires_grad_(True)
        wt, bt = torch.from_numpy(w).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
        rt = torch.from_numpy(res).requires_grad_(True) if with_res else None
        yt = torch.empty((n, c), dtype=torch.float64)
        parts = []
        for i in range(n_inst):
            rows = np.flatnonzero(ids == i)
            if len(rows) == 0:
                assert np.isnan(mean[i]).all() and np.isnan(var[i]).all()
                continue
            # [1, c, n_b]: one sample whose "spatial" axis is the instance's rows
            # (torch refuses a single spatial element; the contract there is y = bias, with a gradient of zero into x)
            normed = torch.nn.functional.instance_norm(xt[rows].T[None], eps=1e-8)[0].T if len(rows) > 1 else xt[rows] - xt[rows]
            parts.append((rows, normed * wt + bt))
        yt = torch.zeros((n, c), dtype=torch.float64)
        for rows, p in parts:
            yt = yt.index_add(0, torch.from_numpy(rows), p)
        if with_res:
            yt = yt + rt
        if relu:
            yt = torch.relu(yt)
        yt.backward(torch.from_numpy(dy))
        scale = lambda a: max(float(np.abs(a).max()), 1e-300)
        assert np.abs(y - yt.detach().numpy()).max() <= 1e-12 * scale(y), name
        one = ids == 0
        if one.sum() == 1 and not with_res and not relu:
            np.testing.assert_array_equal(y[one], np.broadcast_to(b, (1, c)))            # one row: y = bias exactly
        dx, dres, dw, db = IR.in_backward(x, y if relu else None, dy, ids, n_inst, w, mean, var)
        for got, want, what in ((dx, xt.grad, "dx"), (dw, wt.grad.reshape(-1), "dweight"), (db, bt.grad.reshape(-1), "dbias")) + \
                (((dres, rt.grad, "dres"),) if with_res else ()):
            want = want.numpy()
            assert np.abs(got - want).max() <= 1e-12 * scale(want), (name, what, float(np.abs(got - want).max()), scale(want))


def test_constant_column_has_zero_variance_and_zero_xhat():
    _, x, ids, n_inst = cases()[1]
    w, b = np.ones((1, x.shape[1])), np.zeros((1, x.shape[1]))
    y, mean, var = IR.in_forward(x, ids, n_inst, w, b)
    present = ~np.isnan(var[:, 5])
    assert (var[present, 5] == 0).all() and (y[:, 5] == 0).all()


@pytest.mark.parametrize("name", IN_NAMES)
def test_load_model_finds_the_in_family(name):
    import eyoc_amd
    Model = eyoc_amd.load_model(name)
    assert Model is not None and Model.__name__ == name
    base, channels, tr_channels = REFERENCE[name]
    assert Model.__mro__[1] is getattr(eyoc_amd.model, base)
    assert Model.NORM_TYPE == "BN" and Model.BLOCK_NORM_TYPE == "IN"
    assert Model.CHANNELS == channels and Model.TR_CHANNELS == tr_channels
    assert getattr(eyoc_amd, name) is Model and Model in eyoc_amd.IN_MODELS
    model = Model(1, 32, conv1_kernel_size=5, normalize_feature=True)                  # construction on the CPU
    assert model.last_spconv_math == "fp32" and model.check_range() is None
    assert not list(model.block1.norm1.buffers())
    w = model.block3_tr.norm2.weight
    assert tuple(w.shape) == (1, tr_channels[3]) and bool((w == 1).all()) and bool((model.block3_tr.norm2.bias == 0).all())


@pytest.mark.parametrize("name", IN_NAMES)
def test_state_dict_is_the_bn_siblings_after_renaming(name):
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    base, channels, tr_channels = REFERENCE[name]
    sibling = eyoc_amd.load_model("ResUNetBN2" + name[len("ResUNetIN2"):])(1, 32, conv1_kernel_size=5)
    model = eyoc_amd.load_model(name)(1, 32, conv1_kernel_size=5)
    want = IR.in_state_dict({k: v.numpy() for k, v in sibling.state_dict().items()})
    got = model.state_dict()
    assert list(got) == list(want)
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(np.shape(v)) for k, v in want.items()}
    assert "block1.norm1.weight" in got and "block1.norm1.bias" in got and "block1.norm1.bn.weight" not in got
    assert "norm1.bn.running_mean" in got and not any(k.startswith("block") and "running" in k for k in got)
    # a make_weights dict loads after the renaming
    sd = IR.in_state_dict(syn.make_weights(seed=3, channels=tuple(channels), tr_channels=tuple(tr_channels)))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})


def test_the_model_lists_and_the_abstract_base():
    import eyoc_amd
    assert len(eyoc_amd.MODELS) == 9 and len(eyoc_amd.IN_MODELS) == 5
    assert [m.__name__ for m in eyoc_amd.IN_MODELS] == IN_NAMES
    assert not set(eyoc_amd.MODELS) & set(eyoc_amd.IN_MODELS)
    with pytest.raises(NotImplementedError):
        eyoc_amd.ResUNet2(1, 32, conv1_kernel_size=5)
    assert eyoc_amd.load_model("ResUNetIN2Z") is None


def test_the_packed_plan_refuses_in_models():
    import eyoc_amd
    model = eyoc_amd.ResUNetIN2C(1, 32, conv1_kernel_size=5, normalize_feature=True)
    for call in (model.pack, model.pack_host, model.repack, model.repack_device, lambda: model.weight_blob,
                 lambda: setattr(model, "spconv_math", "fp32"), lambda: model.range_snapshot(torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(NotImplementedError, match="packed plan: batch-norm models only"):
            call()
    assert model.spconv_math == "auto"                     # the getter still answers


def test_the_library_declares_the_instance_norm_entry_points():
    from eyoc_amd import _lib
    lib = _lib.load()
    R = lib.eyoc_in_chunk_rows()
    assert R >= 1
    assert lib.eyoc_in_workspace_bytes(100, 12, 2) == 0 and lib.eyoc_in_workspace_bytes(100, 32, 1025) == 0
    assert lib.eyoc_in_workspace_bytes(100, 32, 2) > 0 and lib.eyoc_in_plan_bytes(100, 2) >= 4 * (4 + 3 + 100)
