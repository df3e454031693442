"""Inputs, models and the configuration matrix that tests/test_gpu_conv1_family.py runs the first convolution's five kernels on.
``run_case`` is also what recorded tests/golden/conv1_bytes.json from a build of the parent commit (see the test's docstring): the
library under test is the only thing that differed.

The clouds are those of tests/test_gpu_conv1_persistent.py (its builders, imported): the smallest shapes at which the kernels take
different paths - a ragged single tile, a tile boundary, seven idle waves, a tile across batch indices, a two-pass stage."""
import functools
import hashlib

import numpy as np
import torch

import channel_tables
import test_gpu_conv1_persistent as P
from test_gpu_channel_tables import knobs            # eyoc_<name> switches of the ctx for a block, restored whatever happens

CLOUDS = ("partial-tile", "one-tile-plus-one", "class-0-only", "two-batches", "second-pass")
KNOBS = (3, 1, 0, 2)                                 # eyoc_spconv_select_conv1_kernel: persistent block vectors, block vectors, MFMA, octree walk


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def coords(cloud):
    c = P._case(cloud)[0]
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def feats(cloud, seed, cin):
    """``_feats`` of the persistent test; for more than one input channel a seeded [n, cin] array built the same way"""
    n = len(coords(cloud))
    if cin == 1:
        f = P._feats(n, seed)
    else:
        rng = np.random.default_rng(seed)
        f = rng.uniform(0.25, 2.0, size=(n, cin)).astype(np.float32)
        f[rng.random(n) < 0.05] = 0.0
    f.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------ models
# name -> (class, state dict, in channels, out channels, first convolution's window)
def _spec(name):
    from eyoc_amd import synthetic as syn
    if name in channel_tables.TABLES:                    # "BN2C-k3-in3-out64" (3 -> 32, 3^3: the walker with C_in = 3), "BN2E" (1 -> 128, 5^3)
        cls, _C, _T, cin, cout, ks, _seed = channel_tables.TABLES[name]
        return cls, channel_tables.weights(name), cin, cout, ks, channel_tables.layout_kw(name)
    ks = int(name[len("BN2C-k"):])                       # "BN2C-k5", "BN2C-k3": the persistent test's weights; "BN2C-k7": the probing kernel
    sd = syn.make_weights(seed=7 if ks == 7 else 11, in_channels=1, conv1_kernel_size=ks)
    return "ResUNetBN2C", sd, 1, 32, ks, None


@functools.lru_cache(maxsize=None)
def model(name):
    import eyoc_amd
    cls, sd, cin, cout, ks, _kw = _spec(name)
    m = eyoc_amd.load_model(cls)(cin, cout, bn_momentum=0.05, conv1_kernel_size=ks, normalize_feature=True)
    missing = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    assert not missing.missing_keys and not missing.unexpected_keys
    m = m.cuda().eval()
    m.range_check = False                                # the split16 cases read the guard's words themselves
    return m


# ------------------------------------------------------------------------------------------------ configurations
def cases():
    """-> ``[(key, model, cloud, math, maps_internal_order, conv1 kernel knob, conv1 workgroups)]``"""
    out = []

    def add(name, cloud, math, order, knob=3, wg=0):
        out.append((f"{name}/{math}/order={order}/conv1={knob}/wg={wg}/{cloud}", name, cloud, math, order, knob, wg))

    for ks in (5, 3):
        # split16 on Z-ordered maps: the knob picks conv1_bfp_kernel, conv1_bf_kernel, conv1_mfma_kernel or conv1_tree_kernel<32>
        for knob in KNOBS:
            for cloud in CLOUDS:
                add(f"BN2C-k{ks}", cloud, "split16", 1, knob)
        for cloud in ("second-pass", "two-batches"):     # one persistent workgroup walks every tile: both LDS buffers reused
            add(f"BN2C-k{ks}", cloud, "split16", 1, 3, 1)
        # fp32: conv1_tree_kernel<32> writing fp32 rows; on Z-ordered maps the input goes through launch_permute_rows first
        for order in (0, 1):
            for cloud in ("partial-tile", "two-batches"):
                add(f"BN2C-k{ks}", cloud, "fp32", order)
    for math, order in (("fp32", 0), ("fp32", 1), ("split16", 1)):
        add("BN2C-k3-in3-out64", "two-batches", math, order)          # conv1_tree_kernel<32> with C_in = 3
        for cloud in ("partial-tile", "two-batches"):
            add("BN2C-k7", cloud, math, order)                        # conv1_kernel<32>: a 7^3 window has no walker
    for order in (0, 1):
        add("BN2E", "partial-tile", "fp32", order)                    # conv1_kernel<128>: 125 x 132 floats exceed the walker's 64 KB
    assert len({c[0] for c in out}) == len(out)
    return out


def run_case(name, cloud, math, order, knob, wg):
    """One forward -> ``dict(sha256=<of out.F's bytes>, words=<the four range-guard words, split16 only>)``"""
    import eyoc_amd
    m = model(name)
    cin, ks = _spec(name)[2], _spec(name)[4]
    c, f = coords(cloud), feats(cloud, ks, cin)
    m.spconv_math = math
    try:
        with torch.no_grad():
            if math == "split16":
                assert order == 1
                out, words, _ = P._run(m, np.array(c), np.array(f), knob, wg)   # Z-ordered maps, the knobs set and restored, the words read
                words = [int(w) for w in words.astype(np.uint32)]
            else:
                with knobs(maps_internal_order=order, spconv_select_conv1_kernel=knob, spconv_conv1_workgroups=wg):
                    x = eyoc_amd.SparseTensor(torch.from_numpy(np.array(f)).cuda(), coordinates=torch.from_numpy(np.array(c)).cuda())
                    out = m(x).F
                    assert m._handle is not None and m.last_spconv_math == "fp32"
                    assert (x.coordinate_manager.row_order() is not None) == (order == 1)
                    out, words = out.contiguous().cpu().numpy(), None
        assert out.shape == (len(c), _spec(name)[3]) and np.isfinite(out).all()
        return dict(sha256=hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest(), words=words)
    finally:
        m.spconv_math = "auto"
