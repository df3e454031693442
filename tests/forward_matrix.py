"""Inputs, models and the configuration matrix that tests/test_gpu_forward_steps.py runs the packed forward on, and the three-cloud batch
it shares with tests/test_gpu_sampled_tail.py.  ``run_case`` is also what recorded tests/golden/forward_steps.json and
tests/golden/forward_bytes.json from a build of the parent commit (see the test's docstring): it takes the function that answers the
schedule as an argument, everything else is the same code."""
import functools
import hashlib

import numpy as np
import torch

from test_gpu_channel_tables import knobs            # eyoc_<name> switches of the ctx for a block, restored whatever happens


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def large_batch():
    """-> ``(coords, feats, rows per cloud)``: three clouds in one batch, just above the 8192 rows from which the forward runs split16
    arithmetic on Z-ordered rows.  Batch index 0 is a dense 20 x 20 x 20 block: its 256-row tiles reference more than 639 distinct
    neighbour rows, so their records stage in TWO passes; the two lidar-like clouds behind it give one-pass tiles and a ragged last tile."""
    from eyoc_amd import synthetic as syn
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(20), indexing="ij"), -1).reshape(-1, 3) + 5
    p = syn.make_pair(2, beams=32, azimuths=1000, band=None)
    coords = syn.batch_coords([g, p["coords0"], p["coords1"]])
    n = len(coords)
    feats = np.random.default_rng(5).uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    assert n >= 8192 and n % 256 != 0
    return coords, feats, (len(g), len(p["coords0"]), len(p["coords1"]))


@functools.lru_cache(maxsize=None)
def small_cloud():
    """-> ``(coords, feats)``: one lidar-like cloud of 4599 rows - the caller's row order, fp32 by default, no tile records"""
    from eyoc_amd import synthetic as syn
    coords = syn.batch_coords([syn.make_pair(3, beams=16, azimuths=500, band=None)["coords0"]])
    assert 2048 < len(coords) < 6000
    return coords, np.random.default_rng(6).uniform(0.5, 2.0, size=(len(coords), 1)).astype(np.float32)


def fixture(which):
    return large_batch()[:2] if which == "large" else small_cloud()


def listed_rows(which):
    """17 rows in no order (one 16-row chunk and one row more)"""
    n = len(fixture(which)[0])
    return np.random.default_rng(17).permutation(n)[:17].astype(np.int64)


# ------------------------------------------------------------------------------------------------ models
MODELS = ("BN2C", "IN2C", "ExpBN2C", "BN2")
# BN2C     5^3 first convolution, normalised output, the 96 -> 64 -> 32 tail
# IN2C     ResUNetIN2C on the packed plan: instance-norm steps, the instance plans built on demand
# ExpBN2C  ResUNetExpBN2C: the stand-alone affine norms
# BN2      the row of tests/channel_tables.py whose tail is 96 -> 32 -> 32: the tail matcher must refuse it


@functools.lru_cache(maxsize=None)
def model(name):
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    if name == "BN2":
        import channel_tables
        cls, sd = channel_tables.TABLES[name][0], channel_tables.weights(name)
    elif name == "IN2C":
        import inorm_restatement as IR
        cls, sd = "ResUNetIN2C", IR.in_state_dict(syn.make_weights(seed=21))
    elif name == "ExpBN2C":
        cls, sd = "ResUNetExpBN2C", syn.make_weights(seed=33, expanded=True)
    else:
        cls, sd = "ResUNetBN2C", syn.make_weights()
    m = eyoc_amd.load_model(cls)(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    missing = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    assert not missing.missing_keys and not missing.unexpected_keys
    m = m.cuda().eval()
    if name == "IN2C":
        m.packed_in = True
    return m


# ------------------------------------------------------------------------------------------------ configurations
# the batch paths forced onto any input (tests/test_gpu_channel_tables.py FORCED): Z-ordered rows, every record family, 64-channel
# workgroups on the stride-1 layers - the only setting in which the tail rides in block2_tr.conv2's epilogue on inputs this small
FORCED = dict(spconv_upc_min_rows=0, maps_internal_order=1, spconv_st_split_below=0)


def cases():
    """-> ``[(case name, switches, spconv_math, rows listed?)]``: the default, then one switch at a time over all its values"""
    out = [("default", {}, "auto", False), ("math=fp32", {}, "fp32", False), ("math=split16", {}, "split16", False)]
    out += [(f"fuse_tail={v}", dict(model_fuse_tail=v), "auto", False) for v in (0, 1, 2)]
    out += [(f"sampled_tail={v}" + (",rows" if r else ""), dict(model_sampled_tail=v), "auto", r) for v in (0, 1) for r in (False, True)]
    out += [(f"up_kernel={v}", dict(spconv_select_up_kernel=v), "auto", False) for v in (0, 1, 2)]
    out += [(f"lazy_tables={v}", dict(maps_lazy_tables=v), "auto", False) for v in (0, 1)]
    out += [(f"split16_kernel={v}", dict(spconv_select_split16_kernel=v), "auto", False) for v in (0, 1, 2)]
    out += [(f"down_kernel={v}", dict(spconv_select_down_kernel=v), "auto", False) for v in (0, 1)]
    # beyond the switches one at a time: the record families that start at 2^17 rows in production, and the forced batch paths
    out += [("upc_min_rows=0", dict(spconv_upc_min_rows=0), "auto", False)]
    out += [("forced" + (",rows" if r else ""), FORCED, "split16", r) for r in (False, True)]
    return out


def run_case(which, name, switches, math, rows, steps_of):
    """One configuration: the maps built and the forward run under ``switches`` -> ``dict(steps=, work=, math=, sha256=)``.
    ``steps_of(model, x, rows, out)`` answers the schedule as ``Model.forward_steps`` does."""
    import eyoc_amd
    coords, feats = fixture(which)
    m = model(name)
    r = torch.from_numpy(listed_rows(which)).cuda() if rows else None
    m.spconv_math = math
    try:
        with knobs(**switches), torch.no_grad():         # (no gradient can be asked for: the IN model takes its packed plan)
            x = eyoc_amd.SparseTensor(torch.from_numpy(feats).cuda(), coordinates=torch.from_numpy(coords).cuda())
            out = m(x, rows=r) if rows else m(x).F
            assert m._handle is not None and not out.requires_grad, "the forward must have run the packed plan"
            steps = steps_of(m, x, r, out)
            work = m.layer_work(x)
            return dict(steps=[list(s) for s in steps], work=[[w["name"], w["pairs"], w["flop"], w["gather_bytes"], w["compulsory_bytes"]] for w in work],
                        math=m.last_spconv_math, sha256=hashlib.sha256(out.contiguous().cpu().numpy().tobytes()).hexdigest())
    finally:
        m.spconv_math = "auto"
