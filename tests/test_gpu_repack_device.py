"""Device-side weight re-pack (``eyoc_model_repack_device`` / ``Model.repack_device`` / ``device_repack`` / ``train.ema_sync``).

``Model.pack_host()`` - the existing host packer - is the reference throughout: the device packer has to reproduce its blob bit for
bit (weights in fp32 fragment order, the split16 halves, shifts, the per-layer scale words, zero padding), for every model family,
for weights that drive every branch of the two layer-scale rules, and it has to leave the handle alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FAMILIES = {
    "BN2C-k5-in1-out32": ("ResUNetBN2C", dict(in_channels=1, out_channels=32, conv1_kernel_size=5)),
    "BN2C-k3-in3-out64": ("ResUNetBN2C", dict(in_channels=3, out_channels=64, conv1_kernel_size=3)),
    "BN2E": ("ResUNetBN2E", dict(channels=(None, 128, 128, 128, 256), tr_channels=(None, 64, 128, 128, 128))),
    "FatBN": ("ResUNetFatBN", dict(channels=(None, 32, 64, 128, 256), tr_channels=(None, 128, 128, 128, 256))),
    "ExpBN2C": ("ResUNetExpBN2C", dict(expanded=True)),
}


@functools.lru_cache(maxsize=None)
def _weights(family, seed):
    from eyoc_amd import synthetic as syn
    return {k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_weights(seed=seed, **FAMILIES[family][1]).items()}


def _model(family="BN2C-k5-in1-out32", seed=1):
    import eyoc_amd
    name, kw = FAMILIES[family]
    m = eyoc_amd.load_model(name)(kw.get("in_channels", 1), kw.get("out_channels", 32), bn_momentum=0.05,
                                  conv1_kernel_size=kw.get("conv1_kernel_size", 5), normalize_feature=True)
    m.load_state_dict(_weights(family, seed))
    return m.cuda().eval()


def _overwrite(model, family="BN2C-k5-in1-out32", seed=99):
    """Every ``state_dict`` entry in place, as the EMA sync writes them."""
    sd = _weights(family, seed)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(sd[k].reshape(v.shape))


def _assert_same_bytes(blob, want, what=""):
    got = blob.cpu().view(torch.int32)
    want = want.view(torch.int32)
    assert got.shape == want.shape
    bad = torch.nonzero(got != want).flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {got.numel()} words differ, first at float {int(bad[0])}: "
                              f"{int(got[bad[0]]) & 0xffffffff:#010x} != {int(want[bad[0]]) & 0xffffffff:#010x}")


def _cloud(rows, seed):
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(-14, 14, size=(6 * rows, 3)), axis=0).astype(np.int32)
    c = c[rng.permutation(len(c))[:rows]]
    assert len(c) == rows
    coords = syn.batch_coords([c])
    return eyoc_amd.SparseTensor(torch.ones((rows, 1), device="cuda"), coordinates=torch.from_numpy(coords).cuda())


# ------------------------------------------------------------------------------------------------ 1. bytes, per model family
@pytest.mark.parametrize("family", list(FAMILIES))
def test_repack_device_writes_the_host_packers_bytes(family):
    model = _model(family)
    blob = model.pack()
    handle, ptr = model._handle.value, blob.data_ptr()
    _overwrite(model, family)
    out = model.repack_device()
    assert out is blob and model._handle.value == handle and model._blob.data_ptr() == ptr
    _assert_same_bytes(blob, model.pack_host(), family)


# ------------------------------------------------------------------------------------------------ 2. edge weights
def _spread(p):
    g = torch.Generator().manual_seed(5)
    mag = torch.exp2(-30.0 * torch.rand(p.shape, generator=g))
    sign = torch.where(torch.rand(p.shape, generator=g) < 0.5, -1.0, 1.0)
    p.copy_((mag * sign).to(p.device))


def _set_flat(p, pairs):
    flat = p.view(-1)
    for i, v in pairs:
        flat[i] = v


EDITS = {
    "conv1-all-zero": lambda m: m.conv1.kernel.zero_(),                                    # first convolution: e stays 1, sh = 8
    "block2.conv1-all-zero": lambda m: m.block2.conv1.kernel.zero_(),                      # split16: zero maximum, sh = 0
    "block3.conv2-inf-and-nan": lambda m: _set_flat(m.block3.conv2.kernel, [(12345, float("inf")), (54321, float("nan"))]),
    "conv1-inf": lambda m: _set_flat(m.conv1.kernel, [(77, float("inf"))]),                # not counted: the finite maximum decides
    "conv3-tiny": lambda m: m.conv3.kernel.mul_(2.0 ** -40),                               # sh clamps at 24
    "conv3-huge": lambda m: m.conv3.kernel.mul_(2.0 ** 20),                                # sh clamps at -6
    "norm2-var-zero": lambda m: m.norm2.bn.running_var.zero_(),                            # scale = gamma / sqrt(eps)
    "norm2-negative-gamma": lambda m: m.norm2.bn.weight.copy_(-m.norm2.bn.weight.abs()),
    "conv2-spread": lambda m: _spread(m.conv2.kernel),                                     # lo halves in the fp16 subnormals
    "final-bias": lambda m: m.final.bias.copy_(torch.linspace(-3.0, 5.0, m.final.bias.numel(), device="cuda").view_as(m.final.bias)),
}


@pytest.fixture(scope="module")
def edge_model():
    model = _model()
    model.pack()
    return model


@pytest.mark.parametrize("edit", list(EDITS))
def test_repack_device_edge_weights(edge_model, edit):
    model = edge_model
    handle = model._handle.value
    _overwrite(model)                    # the other layers stay random; undoes the previous case's edit
    with torch.no_grad():
        EDITS[edit](model)
    model.repack_device()
    assert model._handle.value == handle
    _assert_same_bytes(model._blob, model.pack_host(), edit)


# ------------------------------------------------------------------------------------------------ 3. the forward uses the new weights
@pytest.mark.parametrize("rows,math", [(3000, "fp32"), (9000, "split16")])
def test_forward_after_repack_device_equals_a_fresh_host_pack(rows, math):
    x = _cloud(rows, rows)
    model = _model()
    before = model(x).F.clone()
    assert model.last_spconv_math == math
    handle = model._handle.value
    _overwrite(model)
    model.repack_device()
    got = model(x).F
    assert model._handle.value == handle and model.last_spconv_math == math
    fresh = _model(seed=99)
    want = fresh(x).F
    assert torch.equal(got, want)
    rel = float((before - want).abs().max() / want.abs().max())
    assert rel > 1e-2, rel


# ------------------------------------------------------------------------------------------------ 4. handle state survives
def test_handle_state_survives_a_repack():
    x = _cloud(9000, 9000)
    model = _model()
    model.range_check = False            # (the forward's own check would wait for the stream)
    model(x)                             # builds the maps and the workspace: the timed forward below only enqueues
    model.probe_activations(True)
    model.set_timing(True)
    ev = model.progress_event(-1)
    handle = model._handle.value
    _overwrite(model)
    model.repack_device()
    assert model._handle.value == handle
    torch.cuda.synchronize()
    assert ev.query()
    a = torch.randn(8192, 8192, device="cuda")
    for _ in range(16):                  # keeps the stream busy while the host enqueues the forward behind it
        a = (a @ a) * 1e-2
    out = model(x).F
    fired_late = not ev.query()          # re-recorded by this forward: pending behind the products (an untouched event stays complete)
    torch.cuda.synchronize()
    assert fired_late and ev.query()
    assert model.last_spconv_math == "split16"
    mx = model.check_range()
    assert mx is not None and mx > 0
    ms = model.layer_ms()
    assert len(ms) == 23 and all(t >= 0 for t in ms) and sum(ms) > 0
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ 5. device_repack = True
def test_device_repack_switch():
    x = _cloud(3000, 3000)
    model = _model()
    model.device_repack = True
    blob = model.pack()                  # first pack with the parameters on the GPU: handle over a zeroed blob + device packer
    _assert_same_bytes(blob, model.pack_host(), "first pack")
    h0 = model._handle
    _overwrite(model)
    got = model(x).F
    assert model._handle is h0 and model._blob is blob
    _assert_same_bytes(blob, model.pack_host(), "automatic re-pack")
    assert torch.equal(got, _model(seed=99)(x).F)
    _overwrite(model, seed=1)
    assert model.repack() is blob and model._handle is h0
    _assert_same_bytes(blob, model.pack_host(), "repack()")
    # switched off: the host route replaces handle and blob, as before
    model.device_repack = False
    _overwrite(model)
    model(x)
    assert model._handle is not h0 and model._blob is not blob
    _assert_same_bytes(model._blob, model.pack_host(), "host route")


# ------------------------------------------------------------------------------------------------ 6. adopted blob
def test_repack_device_on_an_adopted_blob():
    src = _model()
    packed = src.pack().clone()
    model = _model()
    blob = model.pack(blob=packed, from_blob=True)
    assert blob is packed and model._packed_version is None
    handle = model._handle.value
    _overwrite(model)
    assert model.repack_device() is packed and model._handle.value == handle
    _assert_same_bytes(packed, model.pack_host(), "adopted blob")
    assert model._packed_version == model._weights_version()


# ------------------------------------------------------------------------------------------------ 7. ema_sync
def test_ema_sync_matches_the_reference_loop():
    from eyoc_amd.train import ema_sync
    labeler, model = _model(seed=1), _model(seed=99)
    with torch.no_grad():                # counters that make the integer entries' arithmetic visible
        for i, (k, v) in enumerate(labeler.state_dict().items()):
            if not v.is_floating_point():
                v.fill_(3 + i)
                model.state_dict()[k].fill_(1000 + 7 * i)
    labeler.pack()
    handle = labeler._handle.value
    decay, debias = 0.99, 1 - 0.99 ** 3
    want = {k: v.clone() for k, v in labeler.state_dict().items()}
    with torch.no_grad():                # lib/trainer.py:1510-1512, tensor by tensor
        for lp, mp in zip(want.values(), model.state_dict().values()):
            lp.copy_((decay * lp + (1 - decay) * mp) / debias)
    ema_sync(labeler, model, decay, debias)
    assert labeler._handle.value == handle
    for k, v in labeler.state_dict().items():
        assert v.dtype == want[k].dtype
        if v.is_floating_point():
            assert torch.equal(v.view(torch.int32), want[k].view(torch.int32)), k
        else:
            assert torch.equal(v, want[k]) and int(v) != 0, k
    _assert_same_bytes(labeler._blob, labeler.pack_host(), "ema")
    ema_sync(labeler, model, decay, debias, full_sync=True)
    assert labeler._handle.value == handle
    for (k, v), mv in zip(labeler.state_dict().items(), model.state_dict().values()):
        assert torch.equal(v, mv), k
    _assert_same_bytes(labeler._blob, model.pack_host(), "full sync")
    with pytest.raises(ValueError):
        ema_sync(labeler, _model("ExpBN2C"), decay, debias)


# ------------------------------------------------------------------------------------------------ 8. errors
@pytest.mark.parametrize("case", ["wrong-cin", "missing-norm"])
def test_repack_device_errors_leave_the_blob_alone(case):
    from eyoc_amd import _lib
    lib = _lib.load()
    model = _model()
    blob = model.pack()
    before = blob.clone()
    _overwrite(model)
    layers, n, keep = model._layer_params(device=True)
    hit = 0
    for i in range(n):
        if case == "wrong-cin" and layers[i].name == b"block2.conv1":
            layers[i].cin += 32
            hit += 1
        if case == "missing-norm" and layers[i].name == b"norm3":
            layers[i].name = b"norm3_gone"
            hit += 1
    assert hit == 1
    ws = _lib.workspace(lib.eyoc_model_repack_workspace_bytes(model._handle), blob.device)
    rc = lib.eyoc_model_repack_device(_lib.ctx(blob.device.index), model._handle, layers, n, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    msg = lib.eyoc_last_error().decode()
    assert rc == _lib.ERR_INVALID
    assert ("'block2.conv1'" if case == "wrong-cin" else "'norm3'") in msg, msg
    torch.cuda.synchronize()
    assert torch.equal(blob.view(torch.int32), before.view(torch.int32))
    # too small a workspace is refused as well, before anything runs
    rc = lib.eyoc_model_repack_device(_lib.ctx(blob.device.index), model._handle, layers, n, _lib.ptr(ws), 256, _lib.stream_ptr())
    assert rc == _lib.ERR_WORKSPACE
    del keep
