"""The device-side draws (csrc/draws.hip, eyoc_amd/draws.py) against their numpy restatement (tests/draws_restatement.py), bit for
bit: ``np.array_equal`` on the int64 outputs at the smallest shapes at which the kernels can go wrong - one lane, one wave, a ragged
last block, full permutations, a sort that spans several blocks and takes rocPRIM's large-size path -, the argument rules, the
workspace bounds and repeatability."""
import ctypes as C

import numpy as np
import pytest
import torch

import draws_restatement as dr

pytestmark = pytest.mark.gpu

SUBSETS = [(1, 1), (5, 5), (64, 16), (257, 256), (1025, 3), (5000, 5000), (100003, 2048)]
PAIRS = [(1, 1, 1), (257, 1, 7), (4099, 120000, 119999), (1024, 2 ** 31 - 1, 2)]
MIXED = [(64, 16), (9, 0), (5, 5), (0, 0), (257, 256), (1025, 3), (5000, 5000), (1, 1)]       # eight slots, a k = 0 and an n = 0 one
CANARY = 0x5A


def host(views):
    return [v.cpu().numpy() for v in views]


def restated_mixed():
    if not hasattr(restated_mixed, "value"):
        restated_mixed.value = dr.subsets(21, 6, MIXED)
    return restated_mixed.value


# ----------------------------------------------------------------------------------------------------------------- 1. subsets
@pytest.mark.parametrize("n,k", SUBSETS)
def test_subset_equals_the_restatement(n, k):
    from eyoc_amd import DeviceDraws
    d = DeviceDraws(11)
    d.call = 3
    (got,) = d.subsets([(n, k)])
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (k,) and d.call == 4
    got = got.cpu().numpy()
    assert np.array_equal(got, dr.subset(11, 3, 0, n, k))
    assert len(np.unique(got)) == k and (got >= 0).all() and (got < n).all()


def test_eight_slots_in_one_call_and_one_call_each():
    from eyoc_amd import DeviceDraws
    d = DeviceDraws(21)
    d.call = 6
    together = host(d.subsets(MIXED))
    want = restated_mixed()
    for s, (n, k) in enumerate(MIXED):
        assert together[s].shape == (k,) and np.array_equal(together[s], want[s]), (s, n, k)
    # the same slots one call each (the others keep their places, empty): identical results
    for s, (n, k) in enumerate(MIXED):
        d.call = 6
        alone = host(d.subsets([(0, 0)] * s + [(n, k)]))
        assert np.array_equal(alone[s], together[s]), (s, n, k)
        assert all(len(a) == 0 for a in alone[:s])
    # two slots of one shape differ
    d.call = 6
    a, b = host(d.subsets([(5000, 5000), (5000, 5000)]))
    assert not np.array_equal(a, b) and np.array_equal(np.sort(a), np.arange(5000)) and np.array_equal(np.sort(b), np.arange(5000))


@pytest.mark.parametrize("seed,call", [(0, 0), ((1 << 64) - 1, 0), (0x123456789ABCDEF, 1), (11, (5 << 32) | 9), (11, (1 << 60) - 1)])
def test_seeds_and_call_numbers(seed, call):
    """Both words of the seed and of the call number reach the generator (a call number with the high 32-bit word set included)."""
    from eyoc_amd import DeviceDraws
    d = DeviceDraws(seed)
    d.call = call
    got = host(d.subsets([(257, 256), (1025, 3)]))
    want = dr.subsets(seed, call, [(257, 256), (1025, 3)])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    d.call = call
    assert np.array_equal(d.pairs(257, 1000, 999, slot=2).cpu().numpy(), dr.pairs(seed, call, 2, 257, 1000, 999))


# ----------------------------------------------------------------------------------------------------------------- 2. pairs
@pytest.mark.parametrize("N,n0,n1", PAIRS)
def test_pairs_equal_the_restatement(N, n0, n1):
    from eyoc_amd import DeviceDraws
    d = DeviceDraws(13)
    d.call = 2
    got = d.pairs(N, n0, n1)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (N, 2) and got.is_contiguous() and d.call == 3
    got = got.cpu().numpy()
    assert np.array_equal(got, dr.pairs(13, 2, 0, N, n0, n1))
    assert (got >= 0).all() and (got[:, 0] < n0).all() and (got[:, 1] < n1).all()


# ----------------------------------------------------------------------------------------------------------------- 3. errors
def _raw(n, k, out, ws, ws_bytes=None, n_slots=None, call=0, seed=5):
    from eyoc_amd import _lib
    ns, ks = (C.c_int * max(len(n), 1))(*n), (C.c_int * max(len(k), 1))(*k)
    return _lib.load().eyoc_draw_subsets(_lib.ctx(0), seed, call, len(n) if n_slots is None else n_slots, ns, ks, _lib.ptr(out), _lib.ptr(ws),
                                         ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_ptr())


def test_invalid_arguments_leave_output_and_workspace_alone():
    from eyoc_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    ws = _lib.workspace(lib.eyoc_draw_workspace_bytes(4096), dev)
    out = torch.empty(4096, dtype=torch.int64, device=dev)
    out.view(torch.uint8).fill_(CANARY)
    ws.fill_(CANARY)
    calls = [lambda: _raw([3], [4], out, ws), lambda: _raw([1] * 9, [1] * 9, out, ws), lambda: _raw([-1], [0], out, ws),
             lambda: _raw([3], [-1], out, ws), lambda: _raw([64, 3], [16, 4], out, ws), lambda: _raw([64], [16], out, ws, call=1 << 60),
             lambda: lib.eyoc_draw_pairs(_lib.ctx(0), 5, 0, 0, -1, 2, 2, _lib.ptr(out), _lib.stream_ptr()),
             lambda: lib.eyoc_draw_pairs(_lib.ctx(0), 5, 0, 0, 4, -2, 2, _lib.ptr(out), _lib.stream_ptr()),
             lambda: lib.eyoc_draw_pairs(_lib.ctx(0), 5, 0, 8, 4, 2, 2, _lib.ptr(out), _lib.stream_ptr()),
             lambda: lib.eyoc_draw_pairs(_lib.ctx(0), 5, 0, 0, 4, 0, 2, _lib.ptr(out), _lib.stream_ptr())]
    for i, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID, i
        torch.cuda.synchronize()
        assert bool((out.view(torch.uint8) == CANARY).all()) and bool((ws == CANARY).all()), i
    # empty slots are legal and write nothing
    assert _raw([0, 7], [0, 0], out, ws) == 0 and _raw([], [], out, ws) == 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == CANARY).all()) and bool((ws == CANARY).all())


def test_workspace_bounds():
    """One byte short is refused and writes nothing; the exact size is enough and leaves the bytes behind it alone."""
    from eyoc_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    slots = [(100003, 2048), (257, 256)]
    total_n, total_k = sum(n for n, _ in slots), sum(k for _, k in slots)
    need = lib.eyoc_draw_workspace_bytes(total_n)
    assert need % 256 == 0
    tail = 1 << 16
    buf = _lib.workspace(need + tail, dev)
    buf.fill_(CANARY)
    out = torch.empty(total_k + 512, dtype=torch.int64, device=dev)
    out.view(torch.uint8).fill_(CANARY)
    n, k = [s[0] for s in slots], [s[1] for s in slots]
    assert _raw(n, k, out, buf, ws_bytes=need - 1, seed=17, call=1) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()) and bool((out.view(torch.uint8) == CANARY).all())
    assert _raw(n, k, out, buf, ws_bytes=need, seed=17, call=1) == 0
    torch.cuda.synchronize()
    assert bool((buf[need:] == CANARY).all()), "written behind the workspace"
    assert bool((out[total_k:].view(torch.uint8) == CANARY).all()), "written behind the output"
    want = np.concatenate(dr.subsets(17, 1, slots))
    assert np.array_equal(out[:total_k].cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------------- 4. repeatability
def test_same_call_same_bytes_also_on_a_side_stream():
    from eyoc_amd import DeviceDraws
    d = DeviceDraws(33)

    def both():
        d.call = 9
        s = d.subsets(MIXED[:4] + [(100003, 2048)])
        p = d.pairs(4099, 120000, 119999)
        return [x.cpu().numpy().tobytes() for x in (*s, p)]
    first = both()
    assert both() == first
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = both()
    side.synchronize()
    assert on_side == first
