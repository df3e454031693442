"""The packed plan of the ResUNetIN2 family on the host: the opt-in switch (``model.packed_in``), and the blob ``eyoc_model_pack_host_in``
writes - where an instance norm's weight and bias sit, that the block convolutions are packed with nothing folded in, that the stage
convolutions are the BN sibling's, and that a batch-norm model's blob is what the old entry point gives.  No GPU.

The blob's layout is restated here from the plan's rule (csrc/model.hip build_plan): per layer, in plan order, its fp32 weights
(``pad64(K cin cout)`` floats; a norm layer: ``pad64(c)``) and its shifts (``pad64(cout)``); then per convolution its split16 weights
(not the first convolution) and 64 scale words."""
import ctypes as C

import numpy as np
import pytest
import torch

import inorm_restatement as IR

STAGES = ("1", "2", "3", "4", "4_tr", "3_tr", "2_tr")


def pad64(v):
    return (v + 63) // 64 * 64


def plan_layout(model, inorm):
    """-> {layer name: dict(w, wn, b, bn[, w16, s])} float offsets / counts, and the blob's size"""
    Cn, T = model.CHANNELS, model.TR_CHANNELS
    width = {"1": Cn[1], "2": Cn[2], "3": Cn[3], "4": Cn[4], "4_tr": T[4], "3_tr": T[3], "2_tr": T[2]}
    cin = {"1": model.in_channels, "2": Cn[1], "3": Cn[2], "4": Cn[3], "4_tr": Cn[4], "3_tr": Cn[3] + T[4], "2_tr": Cn[2] + T[3]}
    layers = []                                                     # (name, K, cin, cout, kind)
    for s in STAGES:
        c = width[s]
        layers.append(("conv" + s, model.conv1_kernel_size ** 3 if s == "1" else 27, cin[s], c, "conv1" if s == "1" else "conv"))
        for i in ("1", "2"):
            layers.append((f"block{s}.conv{i}", 27, c, c, "conv"))
            if inorm:
                layers.append((f"block{s}.norm{i}", 0, c, c, "norm"))
    layers.append(("conv1_tr", 1, Cn[1] + T[2], T[1], "conv"))
    layers.append(("final", 1, T[1], model.out_channels, "conv"))
    off, out = 0, {}
    for name, K, ci, co, kind in layers:
        wn = pad64(co) if kind == "norm" else pad64(K * ci * co)
        out[name] = dict(w=off, wn=wn, b=off + wn, bn=pad64(co), elems=K * ci * co, K=K, cin=ci, cout=co, kind=kind)
        off += wn + pad64(co)
    for name, K, ci, co, kind in layers:
        if kind == "norm":
            continue
        if kind != "conv1":
            out[name]["w16"] = off
            off += pad64(K * ci * co)
        out[name]["s"] = off
        off += 64
    return out, off


def make(name, seed=3, packed_in=True):
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    Model = eyoc_amd.load_model(name)
    sd = syn.make_weights(seed=seed, channels=tuple(Model.CHANNELS), tr_channels=tuple(Model.TR_CHANNELS))
    if name.startswith("ResUNetIN2"):
        sd = IR.in_state_dict(sd)
    model = Model(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    if name.startswith("ResUNetIN2"):
        model.packed_in = packed_in
        with torch.no_grad():                                        # make_weights' norms inside the blocks: give every one its own values
            g = torch.Generator().manual_seed(seed)
            for n, p in model.named_parameters():
                if n.startswith("block") and ".norm" in n:
                    p.copy_(torch.rand(p.shape, generator=g) + 0.5)
    return model.eval()


def test_refusals_stand_and_the_switch_opts_in():
    import eyoc_amd
    from eyoc_amd import _lib
    lib = _lib.load()
    model = make("ResUNetIN2C", packed_in=False)
    assert model.packed_in is False
    for call in (model.pack, model.pack_host, model.repack, model.repack_device, lambda: model.weight_blob,
                 lambda: setattr(model, "spconv_math", "fp32"), lambda: model.range_snapshot(torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(NotImplementedError, match="packed plan: batch-norm models only"):
            call()
    d = model._desc()
    bn_floats = int(lib.eyoc_model_blob_floats(C.byref(d)))
    assert model.blob_floats() == bn_floats                          # the default model answers as before
    model.packed_in = True
    blob = model.pack_host()
    layout, floats = plan_layout(model, True)
    assert blob.dtype == torch.float32 and blob.numel() == model.blob_floats() == floats
    assert int(lib.eyoc_model_blob_floats_in(C.byref(d), 1)) == floats
    # the old entry point on the same descriptor: unchanged, and the new one with block_norm 0 is the old one
    sibling = make("ResUNetBN2C")
    layout_bn, floats_bn = plan_layout(sibling, False)
    assert int(lib.eyoc_model_blob_floats(C.byref(d))) == bn_floats == floats_bn == int(lib.eyoc_model_blob_floats_in(C.byref(d), 0))
    assert floats == floats_bn + 14 * 2 * 64 + sum(2 * 2 * (pad64(layout[f"block{s}.norm1"]["cout"]) - 64) for s in STAGES)
    assert lib.eyoc_model_blob_floats_in(C.byref(d), 2) == 0
    model.spconv_math = "fp32"                                       # the setter is open too (no handle yet: it is remembered)
    assert model.spconv_math == "fp32"
    # a BN sibling: pack_host() against the old entry point called by hand, and against the new one with block_norm 0
    got = sibling.pack_host()
    sd_ = sibling._desc()
    layers, nl, keep = sibling._layer_params()
    old = torch.full((floats_bn,), 7.0)
    new0 = torch.full((floats_bn,), 9.0)
    assert lib.eyoc_model_pack_host(C.byref(sd_), layers, nl, C.c_void_p(old.data_ptr()), old.numel()) == 0
    assert lib.eyoc_model_pack_host_in(C.byref(sd_), layers, nl, C.c_void_p(new0.data_ptr()), new0.numel(), 0) == 0
    assert got.numpy().tobytes() == old.numpy().tobytes() == new0.numpy().tobytes()


def test_blob_contents():
    from eyoc_amd import _lib
    lib = _lib.load()
    model = make("ResUNetIN2C")
    sibling = make("ResUNetBN2C")
    layout, floats = plan_layout(model, True)
    layout_bn, _ = plan_layout(sibling, False)
    blob = model.pack_host().numpy().copy()
    # an instance norm: weight at w_off, bias at b_off, zero padding
    for name in ("block1.norm1", "block4.norm2", "block2_tr.norm2"):
        L = layout[name]
        mod = model.get_submodule(name)
        c = L["cout"]
        np.testing.assert_array_equal(blob[L["w"]:L["w"] + c], mod.weight.detach().numpy().reshape(-1))
        np.testing.assert_array_equal(blob[L["b"]:L["b"] + c], mod.bias.detach().numpy().reshape(-1))
        assert not blob[L["w"] + c:L["w"] + L["wn"]].any() and not blob[L["b"] + c:L["b"] + L["bn"]].any()
    # one weight changed: exactly that float of that layer's slot
    with torch.no_grad():
        model.block3.norm2.weight[0, 5] += 0.25
    after = model.pack_host().numpy()
    diff = np.flatnonzero(blob.view(np.uint32) != after.view(np.uint32))
    assert diff.tolist() == [layout["block3.norm2"]["w"] + 5]
    # a block convolution: packed with nothing folded in, in both packings, shift 0
    for name in ("block1.conv1", "block3.conv2", "block4_tr.conv1"):
        L = layout[name]
        W = np.ascontiguousarray(model.get_submodule(name).kernel.detach().numpy(), np.float32)
        want = np.zeros(L["elems"], np.float32)
        assert lib.eyoc_spconv_pack_weights(W.ctypes.data, None, L["K"], L["cin"], L["cout"], want.ctypes.data) == 0
        np.testing.assert_array_equal(after[L["w"]:L["w"] + L["elems"]].view(np.uint32), want.view(np.uint32), err_msg=name)
        want16, osc = np.zeros(L["elems"], np.float32), np.zeros(1, np.float32)
        assert lib.eyoc_spconv_pack_weights_split16(W.ctypes.data, None, L["K"], L["cin"], L["cout"], want16.ctypes.data, osc.ctypes.data) == 0
        np.testing.assert_array_equal(after[L["w16"]:L["w16"] + L["elems"]].view(np.uint32), want16.view(np.uint32), err_msg=name)
        assert after[L["s"]] == osc[0] and not after[L["s"] + 1:L["s"] + 64].any()
        assert not after[L["b"]:L["b"] + L["bn"]].any()
    # the stage convolutions (and the tail): the BN sibling's slots for the same stage parameters
    bn_blob = sibling.pack_host().numpy()
    for name in ["conv" + s for s in STAGES] + ["conv1_tr", "final"]:
        L, B = layout[name], layout_bn[name]
        for key, cnt in (("w", L["wn"]), ("b", L["bn"]), ("w16", L["wn"]), ("s", 64)):
            if key in L:
                np.testing.assert_array_equal(after[L[key]:L[key] + cnt].view(np.uint32), bn_blob[B[key]:B[key] + cnt].view(np.uint32),
                                              err_msg=f"{name} {key}")


def test_a_missing_or_missized_instance_norm_is_refused_by_name():
    from eyoc_amd import _lib
    lib = _lib.load()
    model = make("ResUNetIN2C")
    d = model._desc()
    blob = torch.zeros(model.blob_floats())

    def pack(edit):
        layers, nl, keep = model._layer_params()
        for i in range(nl):
            if layers[i].name == b"block2.norm1":
                edit(layers[i])
        return lib.eyoc_model_pack_host_in(C.byref(d), layers, nl, C.c_void_p(blob.data_ptr()), blob.numel(), 1)

    assert pack(lambda lp: None) == 0
    for edit in (lambda lp: setattr(lp, "bn_weight", None), lambda lp: setattr(lp, "bn_bias", None), lambda lp: setattr(lp, "cout", 32),
                 lambda lp: setattr(lp, "name", b"block2.norm9")):
        assert pack(edit) == _lib.ERR_INVALID
        assert "block2.norm1" in lib.eyoc_last_error().decode()
    # a batch norm's statistics where an instance norm is expected: the caller packed the wrong model
    some = np.ones(64, np.float32)
    assert pack(lambda lp: setattr(lp, "bn_mean", some.ctypes.data_as(C.POINTER(C.c_float)))) == _lib.ERR_INVALID
    assert "block2.norm1" in lib.eyoc_last_error().decode()
    # and the BN plan refuses the IN model's layer list (no statistics), as before
    layers, nl, keep = model._layer_params()
    assert lib.eyoc_model_pack_host(C.byref(d), layers, nl, C.c_void_p(blob.data_ptr()), blob.numel()) == _lib.ERR_INVALID


def test_broadcast_model_takes_an_opted_in_model_on_the_host():
    """dist.broadcast_model lives on the packed blob: the sending rank's blob is pack_host()'s, a model that did not opt in still refuses"""
    from eyoc_amd import dist
    model = make("ResUNetIN2C")
    blob = dist.broadcast_model(model, "cpu")
    assert blob.numpy().tobytes() == model.pack_host().numpy().tobytes()
    with pytest.raises(NotImplementedError, match="packed plan: batch-norm models only"):
        dist.broadcast_model(make("ResUNetIN2C", packed_in=False), "cpu")
