"""GPU: every stage of ``eyoc_sc2pcr`` (csrc/sc2pcr.hip) against the fp64 restatement of tests/sc2pcr_stages.py.

One library call per input through ctypes, the workspace copied back once (``eyoc_sc2pcr_workspace_layout`` says where each stage
left its result), then one checker per stage, each fed with the device's own output of the stage before it.  The two tolerances that
depend on the input's spectral gap (eigenvector ``v``, local-stage ``seed_h``) are 4 x the error of the fp32 torch oracle against the
same fp64 restatement on the same stage input, computed here at run time and printed next to the device's figure."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _inputs as gi
import sc2pcr_stages as st

pytestmark = pytest.mark.gpu

_cache = {}


def _golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g4_sc2pcr.npz"))


def _params(p, n):
    from eyoc_amd import _lib as L
    n_seed = int(n * p["ratio"])      # as eyoc_amd.Matcher._params: a ratio that floors to Python's int(n * ratio) in fp32 too
    return L.Sc2pcrParams(float(p["inlier_threshold"]), float(p["d_thre"]), (n_seed + 0.5) / n, float(p["nms_radius"]),
                          int(p["num_iterations"]), 16384, int(p["k1"]), int(p["k2"]))


def _layout(p, n):
    from eyoc_amd import _lib as L
    lay = L.Sc2pcrLayout()
    assert L.load().eyoc_sc2pcr_workspace_layout(n, C.byref(_params(p, n)), C.byref(lay)) == 0
    assert lay.total == L.load().eyoc_sc2pcr_workspace_bytes(n, C.byref(_params(p, n)))
    return lay


def device_dump(src, tgt, p):
    """One ``eyoc_sc2pcr`` call; the whole workspace comes back in one copy."""
    from eyoc_amd import _lib as L
    lib, n = L.load(), len(src)
    lay, cp = _layout(p, n), _params(p, n)
    s, t = torch.from_numpy(np.ascontiguousarray(src)).cuda(), torch.from_numpy(np.ascontiguousarray(tgt)).cuda()
    T = torch.empty(16, dtype=torch.float32, device="cuda")
    fit = torch.zeros(max(lay.n_seed, 1), dtype=torch.float32, device="cuda")
    ws = torch.zeros(int(lay.total), dtype=torch.uint8, device="cuda")
    L.check(lib.eyoc_sc2pcr(L.ctx(0), L.ptr(s), L.ptr(t), n, C.byref(cp), L.ptr(T), L.ptr(fit), L.ptr(ws), ws.numel(), L.stream_ptr()),
            "eyoc_sc2pcr")
    torch.cuda.synchronize()
    return st.dump_from_workspace(ws.cpu().numpy(), lay, src, tgt, p, fit.cpu().numpy(), T.cpu().numpy())


def restated(name):
    """Input, fp64 first-order restatement and the fp32 oracle's own eigenvector error against it - once per input and module."""
    if name not in _cache:
        src, tgt, p = st.case_input(name, gi, _golden())
        fo = st.FirstOrder(src, tgt, p)
        _cache[name] = (src, tgt, p, fo, st.oracle_v_error(fo, src, tgt, p))
    return _cache[name]


def _report(name, res, ev):
    print(f"sc2pcr stages {name}: fp32 oracle against fp64, v: {ev:.2e} -> tolerance {st.tolerance(ev):.2e}")
    for stage in st.STAGES:
        print(f"    {stage:13s} {res[stage]}")


@pytest.mark.parametrize("name", st.GPU_CASES)
def test_every_stage_matches_the_fp64_restatement(name):
    src, tgt, p, fo, ev = restated(name)
    D = device_dump(src, tgt, p)
    res = st.run_all(D, fo, st.tolerance(ev))
    _report(name, res, ev)
    assert st.failed(res) == [], {k: res[k] for k in st.failed(res)}


def test_batched_slices_equal_the_single_pair_dumps_byte_for_byte():
    """One ``eyoc_sc2pcr_batched`` call of 9 ragged pairs with two different ``num_iterations``: pair b lives at
    ``ws + b * align_up(max_b total)`` with its own layout; every buffer of its slice equals the dump of the single-pair call byte for
    byte (``y`` and the bytes beyond each buffer's length excluded), and passes the checkers."""
    from eyoc_amd import _lib as L
    names = ("golden3", "n65", "n777", "golden0", "n20", "tdm", "golden2", "scaled", "exact")
    cases = [restated(nm) for nm in names]
    assert len({c[2]["num_iterations"] for c in cases}) == 2
    ns = [len(c[0]) for c in cases]
    B = len(cases)
    lays = [_layout(c[2], n) for c, n in zip(cases, ns)]
    params = (L.Sc2pcrParams * B)(*[_params(c[2], n) for c, n in zip(cases, ns)])
    seg = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    src = torch.from_numpy(np.concatenate([c[0] for c in cases])).cuda()
    tgt = torch.from_numpy(np.concatenate([c[1] for c in cases])).cuda()
    stride = max(l.n_seed for l in lays)
    slice_bytes = (max(int(l.total) for l in lays) + 255) // 256 * 256
    lib = L.load()
    i_max = int(np.argmax(ns))
    assert lib.eyoc_sc2pcr_batched_workspace_bytes_n(ns[i_max], B, C.byref(params[i_max])) == slice_bytes * B
    T = torch.empty((B, 16), dtype=torch.float32, device="cuda")
    fit = torch.zeros((B, stride), dtype=torch.float32, device="cuda")
    ws = torch.zeros(slice_bytes * B, dtype=torch.uint8, device="cuda")
    segc = (C.c_int32 * (B + 1))(*seg.tolist())
    L.check(lib.eyoc_sc2pcr_batched(L.ctx(0), L.ptr(src), L.ptr(tgt), segc, B, params, L.ptr(T), L.ptr(fit), stride, L.ptr(ws),
                                    ws.numel(), L.stream_ptr()), "eyoc_sc2pcr_batched")
    torch.cuda.synchronize()
    wsh, Th, fh = ws.cpu().numpy(), T.cpu().numpy(), fit.cpu().numpy()
    for b, (nm, (s, t, p, fo, ev)) in enumerate(zip(names, cases)):
        Db = st.dump_from_workspace(wsh[b * slice_bytes:(b + 1) * slice_bytes], lays[b], s, t, p, fh[b], Th[b])
        D1 = device_dump(s, t, p)
        assert st.dumps_equal(Db, D1) == [], f"pair {b} ({nm})"
        res = st.run_all(Db, fo, st.tolerance(ev))
        assert st.failed(res) == [], (nm, {k: res[k] for k in st.failed(res)})
