"""CPU checks of the radius-match feature (no GPU): the restatement the GPU tests compare against (tests/matches_restatement.py) -
its two candidate sources agree bit for bit on the GPU tests' inputs, the contract's corner rules hold, planted defects are caught -
and the boundary: the header declares the new entry points, and without a GPU the Python functions fail loudly."""
import os
import re

import numpy as np
import pytest

import matches_cases as cases
import matches_restatement as M
from icp_restatement import _d2, pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


ALL_CASES = [("ragged", cases.ragged), ("dense", cases.dense), ("faces0.5", lambda: cases.faces(0.5)), ("faces0.45", lambda: cases.faces(0.45)),
             ("chunked", lambda: cases.chunked(n_pairs=8))]


@pytest.mark.parametrize("name,make", ALL_CASES, ids=[n for n, _ in ALL_CASES])
def test_brute_and_tree_agree_bit_for_bit(name, make):
    pairs, r = make()
    seen = 0
    for src, tgt, T in pairs:
        for K in (None, 1, 3):
            b, t = M.brute(src, tgt, T, r, K), M.tree(src, tgt, T, r, K)
            assert _same(b, t), (name, K)
            seen += len(b[0])
    assert seen > 0


def test_ragged_statuses_and_sizes():
    pairs, r = cases.ragged()
    st = [M.status(s, t, T, r) for s, t, T in pairs]
    assert st == [0, 0, 0, 0, 0, 0, M.BAD_INIT, M.RANGE, 0]
    m = [len(M.brute(s, t, T, r)[0]) for s, t, T in pairs]
    assert m[0] > 300 and m[1] > 0 and m[2] > 0 and m[8] > 0
    assert m[3:8] == [0, 0, 0, 0, 0]      # empty source, empty target, far apart, NaN pose, inf target
    assert [len(s) for s, _, _ in pairs[:3]] == [300, 1, 513] and [len(t) for _, t, _ in pairs[:3]] == [280, 700, 40]


def test_dense_case_has_ties_and_gate_equal_candidates():
    (src, tgt, T), = cases.dense()[0]
    r = 0.5
    d = _d2(pose(src, T)[0][None], tgt.astype(np.float64))
    assert int((d == r * r).sum()) == 6                      # at the gate exactly: no match
    pairs, d2 = M.brute(src, tgt, T, r)
    row0 = pairs[:, 0] == 0
    assert int(row0.sum()) == 150 and int((d < r * r).sum()) == 150
    assert len(np.unique(d2[row0])) < 75                     # exact ties (every value at least twice)
    j = pairs[row0, 1]
    tie = np.flatnonzero(np.diff(d2[row0]) == 0)
    assert len(tie) >= 75 and (j[tie] < j[tie + 1]).all()    # a tie goes to the lower target row
    assert (np.diff(d2[row0]) >= 0).all()


def test_strict_gate_K_and_empty_segments():
    src = np.zeros((1, 3), np.float32)
    tgt = np.array([[0.5, 0, 0], [0.25, 0, 0], [0, -0.25, 0], [0, 0, 0.125], [0, 0.5, 0]], np.float32)
    pairs, d2 = M.brute(src, tgt, None, 0.5)
    assert pairs.tolist() == [[0, 3], [0, 1], [0, 2]] and d2.tolist() == [0.015625, 0.0625, 0.0625]
    assert M.brute(src, tgt, None, 0.5, 2)[0].tolist() == [[0, 3], [0, 1]]
    assert M.brute(src, tgt, None, 0.5, 1)[0].tolist() == [[0, 3]]
    assert M.brute(src, tgt, None, 0.5, 9)[0].tolist() == pairs.tolist()
    assert M.counts(src, tgt, None, 0.5, 2).tolist() == [2]
    for s, t in ((src[:0], tgt), (src, tgt[:0]), (src[:0], tgt[:0])):
        assert len(M.brute(s, t, None, 0.5)[0]) == 0 and M.status(s, t, None, 0.5) == 0 and len(M.tree(s, t, None, 0.5)[0]) == 0
    assert M.brute(src, tgt, None, 0.5)[0].dtype == np.int64


def test_faces_hit_the_key_range_exactly_at_the_limit():
    for r in (0.5, 0.45):
        pairs, _ = cases.faces(r)
        st = [M.status(s, t, T, r) for s, t, T in pairs]
        assert st == [0, 0, 0, M.RANGE, 0, M.RANGE, M.RANGE], (r, st)
        assert len(M.brute(*pairs[2], r)[0]) >= 3 and len(M.brute(*pairs[4], r)[0]) >= 3     # matches in the outermost cells
    hi_in, hi_out, lo_in, lo_out = cases.range_limits(0.5)
    assert (hi_out, lo_in) == (np.float32(65536.0625), np.float32(-65536.0625))
    # one ulp decides at the gate (r = 0.5: the multiples of r are exact)
    src, tgt, T = cases.faces(0.5)[0][0]
    d = _d2(pose(src, T)[:, None, :], tgt.astype(np.float64)[None])
    assert (d == 0.25).any() and ((d < 0.25) & (d > 0.2499999)).any() and ((d > 0.25) & (d < 0.2500001)).any()
    assert (src < 0).any() and (src > 0).any()


def test_collate_is_the_reference_loop():
    rng = np.random.default_rng(5)
    n0, n1 = [7, 0, 12, 5], [9, 4, 0, 6]
    match = [rng.integers(0, 5, (m, 2)) for m in (6, 0, 0, 3)]
    # lib/data_loaders.py:48-72, literally: the head moves for every pair; a pair without matches contributes nothing
    curr = np.zeros((1, 2), np.int64)
    ref = []
    for b in range(len(n0)):
        if len(match[b]) != 0:
            ref.append(np.array(match[b]) + curr)
        curr[0, 0] += n0[b]
        curr[0, 1] += n1[b]
    got, seg = M.collate(match, n0, n1)
    assert np.array_equal(got, np.concatenate(ref)) and seg.tolist() == [0, 6, 6, 6, 9]
    assert got.dtype == np.int64


# --- planted defects: each is a wrong reading of the contract, and the comparison with ``brute`` has to notice ----------------------
def _defect(src, tgt, T, r, K, kind):
    p, q = pose(src, np.eye(4) if T is None else T), np.asarray(tgt, np.float32).astype(np.float64)
    out_p, out_d = [], []
    for i in range(len(p)):
        d = _d2(p[i][None], q)
        j = np.flatnonzero(d <= r * r if kind == "le_gate" else d < r * r)
        if kind == "k_before_sort" and K:
            j = j[:K]
        o = np.argsort(j, kind="stable") if kind == "order_by_j" else np.lexsort((j, d[j]))
        if K:
            o = o[:K]
        out_p.append(np.stack([np.full(len(o), i), j[o]], 1))
        out_d.append(d[j[o]])
    return np.concatenate(out_p).astype(np.int64), np.concatenate(out_d)


@pytest.mark.parametrize("kind,K", [("order_by_j", None), ("le_gate", None), ("k_before_sort", 3), ("none", None), ("none", 3)])
def test_planted_defects_are_caught(kind, K):
    (src, tgt, T), = cases.dense()[0]
    ref = M.brute(src, tgt, T, 0.5, K)
    got = _defect(src, tgt, T, 0.5, K, kind)
    assert _same(ref, got) == (kind == "none")


def test_overlap_ratio_restatement():
    rng = np.random.default_rng(9)
    s, t, T = cases.lattice_pair(rng, 200, 120)
    c01, c10 = M.counts(s, t, T, 0.3, 1), M.counts(t, s, np.linalg.inv(T), 0.3, 1)
    assert set(np.unique(c01)) <= {0, 1} and 0 < c01.sum() < len(s)
    assert M.overlap_ratio(s, t, T, 0.3) == max(c01.sum() / 200, c10.sum() / 120)


# --- the boundary ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "eyoc_hip.h")).read()
    assert "#define EYOC_VERSION 111" in src
    block = src[src.index("eyoc_posed_nn_grid("):]
    for name, ret in (("eyoc_radius_matches_workspace_bytes", "size_t"), ("eyoc_radius_matches_count", "int"), ("eyoc_radius_matches_fill", "int")):
        assert re.search(rf"^{ret} {name}\(", block, flags=re.M), name
    from eyoc_amd import _lib
    lib = _lib.load()
    for name in ("eyoc_radius_matches_workspace_bytes", "eyoc_radius_matches_count", "eyoc_radius_matches_fill"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    small, big = lib.eyoc_radius_matches_workspace_bytes(1, 100, 100), lib.eyoc_radius_matches_workspace_bytes(65, 100, 100)
    assert 0 < small < big and small % 256 == 0                     # a table per chunk
    assert lib.eyoc_radius_matches_workspace_bytes(0, 1, 1) == 0


def test_host_side_argument_checks_need_no_device():
    import ctypes as C
    from eyoc_amd import _lib
    lib = _lib.load()
    seg = (C.c_int32 * 2)(0, 0)
    assert lib.eyoc_radius_matches_count(None, None, None, seg, seg, 1, None, 0.5, 0, None, None, None, 0, None) == _lib.ERR_INVALID
    assert b"NULL argument" in lib.eyoc_last_error()
    # everything the host can check is checked before the device is touched: stand-in pointers are never followed
    buf = C.create_string_buffer(1024)
    p = C.c_void_p((C.addressof(buf) + 255) // 256 * 256)
    for radius, K, total, out, msg in ((0.0, 0, 0, None, b"radius"), (float("nan"), 0, 0, None, b"radius"), (0.5, -1, 0, None, b"max_per_source"),
                                       (0.5, 0, -1, None, b"negative"), (0.5, 0, 5, None, b"NULL output")):
        assert lib.eyoc_radius_matches_fill(p, None, None, seg, seg, 1, None, radius, K, p, p, total, out, out, p, 0, None) == _lib.ERR_INVALID
        assert msg in lib.eyoc_last_error(), lib.eyoc_last_error()
    bad = (C.c_int32 * 2)(0, -1)
    assert lib.eyoc_radius_matches_count(p, None, None, bad, seg, 1, None, 0.5, 0, p, p, p, 0, None) == _lib.ERR_INVALID
    assert lib.eyoc_radius_matches_count(p, None, None, seg, seg, 1, None, 0.5, 0, p, p, p, 0, None) == _lib.ERR_WORKSPACE


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import eyoc_amd
    a = np.zeros((4, 3), np.float32)
    with pytest.raises(eyoc_amd.EyocError):
        eyoc_amd.get_matching_indices(a, a, np.eye(4), 0.3)
    with pytest.raises(eyoc_amd.EyocError):
        eyoc_amd.matching_indices_batched([a], [a], None, search_voxel_size=0.3)
    with pytest.raises(eyoc_amd.EyocError):
        eyoc_amd.compute_overlap_ratio(a, a, np.eye(4), 0.3)
    with pytest.raises(eyoc_amd.EyocError):
        eyoc_amd.overlap_ratio_batched([a], [a], None, 0.3)
