"""tests/downsample_restatement.py against a plain dictionary-of-lists loop, its invariants, the wrapper's refusals without a GPU, and
the new symbols in the header and in ``_lib.PROTOTYPES``."""
import math
import os
import re

import numpy as np
import pytest

import downsample_restatement as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dict_of_lists(pts, voxel, attrs=None):
    """Open3D's algorithm as one would write it down: a dictionary from cell to the list of its points, in input order."""
    p = [[float(np.float32(v)) for v in row[:3]] for row in pts]
    a = None if attrs is None else [[float(np.float32(v)) for v in row] for row in attrs]
    lo = [min(q[k] for q in p) - 0.5 * voxel for k in range(3)]
    cells, order = {}, []
    for i, q in enumerate(p):
        c = tuple(math.floor((q[k] - lo[k]) / voxel) for k in range(3))
        if c not in cells:
            cells[c] = []
            order.append(c)
        cells[c].append(i)
    xyz, att, first, count, inverse = [], [], [], [], [0] * len(p)
    for r, c in enumerate(order):
        rows = cells[c]
        for cols, out in ((p, xyz),) + (((a, att),) if a is not None else ()):
            s = [0.0] * len(cols[0])
            for i in rows:
                for k in range(len(s)):
                    s[k] += cols[i][k]
            out.append([np.float32(v / float(len(rows))) for v in s])
        first.append(rows[0])
        count.append(len(rows))
        for i in rows:
            inverse[i] = r
    return (np.array(xyz, np.float32), None if a is None else np.array(att, np.float32), np.array(first, np.int32),
            np.array(count, np.int32), np.array(inverse, np.int32))


def _cloud(seed, n, scale=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * scale + offset).astype(np.float32)


@pytest.mark.parametrize("seed, n, voxel, offset", [(0, 300, 0.5, 0.0), (1, 257, 0.25, -40.0), (2, 400, 1.5, 1.0e4), (3, 1, 0.3, 0.0)])
def test_restatement_equals_the_dictionary_loop(seed, n, voxel, offset):
    p = _cloud(seed, n, 1.0, offset)
    a = np.random.default_rng(seed + 100).normal(size=(n, 3)).astype(np.float32)
    got = DR.restate_cloud(p, voxel, a)
    xyz, att, first, count, inverse = dict_of_lists(p, voxel, a)
    assert got["status"] == 0
    assert got["xyz"].tobytes() == xyz.tobytes() and got["attrs"].tobytes() == att.tobytes()
    assert np.array_equal(got["first"], first) and np.array_equal(got["count"], count) and np.array_equal(got["inverse"], inverse)
    assert n < 10 or count.max() > 1, "the case must hold a voxel with several points"


def test_invariants():
    p = _cloud(5, 500, 2.0)
    r = DR.restate_cloud(p, 0.7)
    m = len(r["count"])
    assert r["count"].sum() == len(p) and r["xyz"].shape == (m, 3) and r["attrs"] is None
    assert np.all(np.diff(r["first"]) > 0) and r["first"][0] == 0
    assert np.array_equal(r["inverse"][r["first"]], np.arange(m))
    for row in range(m):                                   # first = the lowest point of the row, count = its points
        members = np.flatnonzero(r["inverse"] == row)
        assert members[0] == r["first"][row] and len(members) == r["count"][row]
    assert np.array_equal(np.bincount(r["inverse"], minlength=m), r["count"])


@pytest.mark.parametrize("bad", ["nan", "inf", "extent"])
def test_a_refused_cloud_has_no_rows_and_leaves_the_others_alone(bad):
    good0, good1, mid = _cloud(6, 50), _cloud(7, 60, 3.0), _cloud(8, 40)
    if bad == "extent":
        mid[3, 1] = mid[:, 1].min() + 0.3 * ((1 << 17) + 2)
    else:
        mid[3, 1] = np.nan if bad == "nan" else -np.inf
    pts, seg = np.concatenate([good0, mid, good1]), [0, 50, 90, 150]
    r = DR.restate_batch(pts, seg, 0.3)
    assert list(r["status"]) == [0, DR.RANGE, 0]
    assert r["seg_out"][1] == r["seg_out"][2] and np.all(r["inverse"][50:90] == -1)
    alone0, alone1 = DR.restate_cloud(good0, 0.3), DR.restate_cloud(good1, 0.3)
    assert r["xyz"].tobytes() == np.concatenate([alone0["xyz"], alone1["xyz"]]).tobytes()
    assert np.array_equal(r["inverse"][90:], alone1["inverse"]) and np.array_equal(r["first"][r["seg_out"][2]:], alone1["first"])


def test_the_extent_limit_is_2_to_the_17_cells():
    edge = np.zeros((2, 3), np.float32)
    edge[1, 0] = ((1 << 17) - 1) * 0.25                    # largest cell 2^17 - 1: held
    assert DR.restate_cloud(edge, 0.25)["status"] == 0
    edge[1, 0] = (1 << 17) * 0.25 - 0.125                  # largest cell exactly 2^17: refused
    assert DR.restate_cloud(edge, 0.25)["status"] == DR.RANGE


def test_empty_clouds():
    r = DR.restate_batch(_cloud(9, 30), [0, 0, 30, 30], 0.5)
    assert list(r["status"]) == [0, 0, 0] and r["seg_out"][0] == r["seg_out"][1] == 0 and r["seg_out"][2] == r["seg_out"][3]


def test_reverse_order_is_another_sum():
    import downsample_cases as DC
    p, a = DC.order_sensitive(65)
    fwd, rev = DR.restate_cloud(p, DC.HUGE_VOXEL, a), DR.restate_cloud(p, DC.HUGE_VOXEL, a, reverse=True)
    assert len(fwd["count"]) == 1 and fwd["count"][0] == 65
    assert fwd["xyz"].tobytes() != rev["xyz"].tobytes() or fwd["attrs"].tobytes() != rev["attrs"].tobytes()


# ---- the wrapper refuses bad input before anything touches a GPU
@pytest.mark.parametrize("kw, word", [
    (dict(seg=[0, 9]), "segments"), (dict(seg=[1, 10]), "segments"), (dict(seg=[0, 6, 4, 10]), "segments"), (dict(seg=[10]), "segments"),
    (dict(voxel=0.0), "voxel_size"), (dict(voxel=-1.0), "voxel_size"), (dict(voxel=float("nan")), "voxel_size"),
    (dict(voxel=float("inf")), "voxel_size"), (dict(attrs=np.zeros((9, 2), np.float32)), "attribute rows"),
    (dict(attrs=np.zeros((10, 9), np.float32)), "attribute columns"), (dict(seg=[0] * 1025 + [10]), "clouds"),
])
def test_wrapper_refuses_before_touching_a_gpu(kw, word, monkeypatch):
    import torch
    from eyoc_amd import downsample
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(downsample, "_cuda_f32", lambda *a, **k: pytest.fail("the input was uploaded before it was validated"))
    with pytest.raises(ValueError, match=word):
        downsample.voxel_down_sample_batched(np.zeros((10, 3), np.float32), kw.get("seg", [0, 10]), kw.get("voxel", 0.3), kw.get("attrs"))


def test_single_cloud_wrapper_refuses_a_bad_voxel_size_without_a_gpu():
    from eyoc_amd import downsample
    with pytest.raises(ValueError, match="voxel_size"):
        downsample.voxel_down_sample(np.zeros((4, 3), np.float32), 0.0)


def test_shim_and_switches_exist():
    import inspect
    import eyoc_amd
    from eyoc_amd import fpfh, matches, o3d
    assert callable(o3d.PointCloud.voxel_down_sample) and callable(o3d.geometry.PointCloud.voxel_down_sample)
    for fn in (matches.compute_overlap_ratio, matches.overlap_ratio_batched, fpfh.register_fpfh_batched):
        assert inspect.signature(fn).parameters["downsample"].default is False
    assert eyoc_amd.voxel_down_sample_batched is eyoc_amd.downsample.voxel_down_sample_batched and callable(eyoc_amd.voxel_down_sample)


def test_symbols_are_declared_and_prototyped():
    from eyoc_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eyoc_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("eyoc_voxel_downsample_workspace_bytes", "eyoc_voxel_downsample_batched"):
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/eyoc_hip.h"
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert len(_lib.PROTOTYPES["eyoc_voxel_downsample_batched"][1]) == 19
    assert re.search(r"#define EYOC_VERSION 111\b", src)
    assert lib.eyoc_voxel_downsample_workspace_bytes(0, 1, 0) == 0
    a, b = lib.eyoc_voxel_downsample_workspace_bytes(1000, 3, 0), lib.eyoc_voxel_downsample_workspace_bytes(2000, 3, 8)
    assert 0 < a < b and a % 256 == 0


def test_the_workspace_case_is_in_the_contract_table():
    """tests/test_gpu_downsample.py adds its case to the table of tests/test_gpu_workspace_contract.py when it is imported (nothing at
    its module level touches a GPU): that names the new sizing function and the wrapper's allocation site for the completeness test."""
    import test_gpu_downsample  # noqa: F401
    import test_gpu_workspace_contract as G
    assert set(G.CASES["voxel_downsample"].covers) == {"eyoc_voxel_downsample_workspace_bytes", "downsample.py:voxel_down_sample_batched"}
