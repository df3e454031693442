"""Batched label generation, the part that needs no GPU: the C ABI (symbols, the slice descriptor's size), the exports, the workspace
size as a host function, and the argument checks, which all answer EYOC_ERR_INVALID before anything touches a device (the context and
the device pointers handed over here are dummies that are never followed)."""
import ctypes as C
import os
import re

import pytest

from eyoc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("eyoc_lowe_topk_segmented", "eyoc_pair_filter_batched", "eyoc_posed_nn_grid_workspace_bytes", "eyoc_posed_nn_grid")
DUMMY = C.c_void_p(0x1000)                      # non-NULL, never dereferenced: every check below fails before a device call


def seg(*v):
    return (C.c_int32 * len(v))(*v)


def test_header_declares_and_lib_binds_the_entry_points():
    src = open(os.path.join(ROOT, "include", "eyoc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.PROTOTYPES
        assert hasattr(lib, name)
    assert re.search(r"\}\s*eyoc_sim_slice\s*;", code)
    assert C.sizeof(_lib.SimSlice) == 24 and _lib.SimSlice.grid1.offset == 16
    assert lib.eyoc_version() == 111


def test_python_api_is_exported():
    import eyoc_amd
    for name in ("lowe_topk_segmented", "pair_filter_batched", "posed_nn_grid", "match_and_filter_corr_batched",
                 "correspondences_under_pose_batched", "corr_through_registration", "label_step"):
        assert callable(getattr(eyoc_amd, name)), name
    # the per-pair functions are still there
    for name in ("lowe_topk", "match_and_filter_corr", "correspondences_under_pose"):
        assert callable(getattr(eyoc_amd, name)), name


def test_workspace_bytes_does_not_decrease_in_any_argument():
    f = _lib.load().eyoc_posed_nn_grid_workspace_bytes
    base = f(1, 1000, 1000)
    assert base > 0 and base % 256 == 0
    assert f(0, 10, 10) == 0 and f(1, -1, 10) == 0 and f(1, 10, -1) == 0
    assert f(1, 0, 0) > 0
    for grid in ([(p, 5000, 6000) for p in (1, 2, 63, 64, 65, 1024)],
                 [(4, q, 6000) for q in (0, 1, 255, 256, 257, 5000, 80000, 1 << 20)],
                 [(4, 5000, t) for t in (0, 1, 31, 32, 33, 6000, 100000, 1 << 20)]):
        sizes = [f(*a) for a in grid]
        assert sizes == sorted(sizes), (grid, sizes)
    assert f(4, 1 << 20, 6000) > f(4, 5000, 6000) and f(4, 5000, 1 << 20) > f(4, 5000, 6000)


def test_topk_rejects_bad_arguments_before_any_device_call():
    lib = _lib.load()
    call = lambda ctx, d1, s, nseg, k, mode, out: lib.eyoc_lowe_topk_segmented(ctx, d1, DUMMY, s, nseg, k, mode, out, None, None)
    good = seg(0, 10, 30)
    assert call(None, DUMMY, good, 2, 5, 0, DUMMY) == _lib.ERR_INVALID
    assert call(DUMMY, None, good, 2, 5, 0, DUMMY) == _lib.ERR_INVALID
    assert call(DUMMY, DUMMY, None, 2, 5, 0, DUMMY) == _lib.ERR_INVALID
    assert call(DUMMY, DUMMY, good, 2, 5, 0, None) == _lib.ERR_INVALID
    assert call(DUMMY, DUMMY, good, 2, 11, 0, DUMMY) == _lib.ERR_INVALID                    # k above the first segment
    assert b"above the 10 rows of segment 0" in lib.eyoc_last_error()
    assert call(DUMMY, DUMMY, seg(0, 30, 10), 2, 5, 0, DUMMY) == _lib.ERR_INVALID           # unsorted
    assert b"must not decrease" in lib.eyoc_last_error()
    assert call(DUMMY, DUMMY, seg(1, 10, 30), 2, 5, 0, DUMMY) == _lib.ERR_INVALID           # does not start at 0
    assert call(DUMMY, DUMMY, good, 2, -1, 0, DUMMY) == _lib.ERR_INVALID
    assert call(DUMMY, DUMMY, good, 0, 5, 0, DUMMY) == _lib.ERR_INVALID
    assert call(DUMMY, DUMMY, good, 2, 5, 2, DUMMY) == _lib.ERR_INVALID                     # mode
    assert lib.eyoc_lowe_topk_segmented(DUMMY, DUMMY, None, good, 2, 5, 0, DUMMY, None, None) == _lib.ERR_INVALID   # mode 0 needs d2


def test_filter_rejects_bad_arguments_before_any_device_call():
    lib = _lib.load()
    s2, m2 = seg(0, 100, 200), seg(0, 10, 20)

    def call(mode=0, ctx=DUMMY, sp0=s2, sp1=s2, sm=m2, nseg=2, T=None, tables=None, slices=None, g0=5.0, out=DUMMY, cnt=DUMMY, P0=DUMMY):
        return lib.eyoc_pair_filter_batched(ctx, mode, P0, DUMMY, DUMMY, DUMMY, sp0, sp1, sm, nseg, T, 2.0, tables, slices, g0, 0.4, out, cnt, None)
    assert call(ctx=None) == _lib.ERR_INVALID
    assert call(cnt=None) == _lib.ERR_INVALID
    assert call(out=None) == _lib.ERR_INVALID
    assert call(P0=None) == _lib.ERR_INVALID
    assert call(sm=None) == _lib.ERR_INVALID
    assert call(mode=3) == _lib.ERR_INVALID
    assert call(mode=1) == _lib.ERR_INVALID                                                  # no poses
    assert call(mode=2) == _lib.ERR_INVALID                                                  # no tables
    sl = (_lib.SimSlice * 2)(_lib.SimSlice(0, 4, 4, 1.0, 0), _lib.SimSlice(0, 0, 4, 1.0, 0))
    assert call(mode=2, tables=DUMMY, slices=sl) == _lib.ERR_INVALID                          # xlim 0
    assert b"table slice of pair 1" in lib.eyoc_last_error()
    assert call(nseg=0) == _lib.ERR_INVALID and call(nseg=1025) == _lib.ERR_INVALID
    assert call(sm=seg(0, 20, 10)) == _lib.ERR_INVALID                                        # unsorted
    assert call(sp0=seg(0, 200, 100)) == _lib.ERR_INVALID
    assert call(sp1=seg(5, 100, 200)) == _lib.ERR_INVALID


def test_grid_rejects_bad_arguments_before_any_device_call():
    lib = _lib.load()
    s2, t2 = seg(0, 100, 200), seg(0, 50, 300)
    big = 1 << 30

    def call(ctx=DUMMY, ss=s2, st=t2, n=2, T=DUMMY, r=2.0, sel=None, ssel=None, idx=DUMMY, status=DUMMY, ws=DUMMY, ws_bytes=big, src=DUMMY):
        return lib.eyoc_posed_nn_grid(ctx, src, DUMMY, ss, st, n, T, r, sel, ssel, idx, None, status, ws, ws_bytes, None)
    for kw in (dict(ctx=None), dict(ss=None), dict(st=None), dict(T=None), dict(status=None), dict(ws=None), dict(idx=None), dict(src=None)):
        assert call(**kw) == _lib.ERR_INVALID, kw
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert call(r=r) == _lib.ERR_INVALID, r
    assert b"max_dist must be positive" in lib.eyoc_last_error()
    assert call(n=0) == _lib.ERR_INVALID and call(n=1025) == _lib.ERR_INVALID
    assert call(ss=seg(0, 200, 100)) == _lib.ERR_INVALID                                      # unsorted
    assert call(st=seg(0, 300, 50)) == _lib.ERR_INVALID
    assert call(ss=seg(1, 100, 200)) == _lib.ERR_INVALID
    assert call(sel=DUMMY) == _lib.ERR_INVALID                                                # a selection without its segments
    assert call(ssel=seg(0, 5, 9)) == _lib.ERR_INVALID
    assert call(sel=DUMMY, ssel=seg(0, 9, 5)) == _lib.ERR_INVALID
    assert call(ws=C.c_void_p(0x1010)) == _lib.ERR_INVALID                                    # alignment
    assert call(ws_bytes=256) == _lib.ERR_WORKSPACE
    assert call(ws_bytes=lib.eyoc_posed_nn_grid_workspace_bytes(2, 200, 300) - 1) == _lib.ERR_WORKSPACE


def test_python_refusals_need_no_gpu():
    import eyoc_amd
    with pytest.raises(AssertionError):
        eyoc_amd.match_and_filter_corr_batched([], [], [], [], feature_filter="Ratio")
    with pytest.raises(AssertionError):
        eyoc_amd.match_and_filter_corr_batched([], [], [], [], spatial_filter="Cube")
    with pytest.raises(ValueError):
        eyoc_amd.match_and_filter_corr_batched([], [], [], [], spatial_filter="Similarity")
    with pytest.raises(ValueError):
        eyoc_amd.corr_through_registration([], [], [], None, on_degenerate="ignore")
