"""The restatement of the device-side draws (tests/draws_restatement.py) on the host: the published Philox4x32-10 vectors, the
distribution of both draws on fixed seeds, their structure, and the host logic of ``DeviceDraws``.  The GPU test
(tests/test_gpu_draws.py) makes the device equal to this restatement bit for bit, so the device inherits what is shown here.

The bar of the three chi-square statistics is ``chi2.ppf(0.999, 63)`` = 103.44.  Realised by the committed layout: first position
43.74, inclusion counts 59.51, pair cells 58.60 (EXPERIMENTS.md, "Device-side draws")."""
import numpy as np
import pytest

import draws_restatement as dr

# counter, key -> output: the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def chi2_bar():
    from scipy.stats import chi2
    return float(chi2.ppf(0.999, 63))


# ----------------------------------------------------------------------------------------------------------------- 1. the generator
@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = dr.philox4x32_10(counter, key)
    assert tuple(int(w[0]) for w in got) == want


def test_philox_is_vectorised_elementwise():
    """An array of counters gives what the counters give one by one; the words of the layout land where the header says."""
    idx = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5], np.uint64)
    seed, call, slot = 0xFEDCBA9876543210, (1 << 59) | 12345, 5
    got = dr.draw_words(seed, call, slot, idx)
    for e, i in enumerate(idx.tolist()):
        one = dr.philox4x32_10((i & 0xFFFFFFFF, i >> 32, call & 0xFFFFFFFF, (call >> 32) | (slot << 28)), (seed & 0xFFFFFFFF, seed >> 32))
        assert [int(w[e]) for w in got] == [int(w[0]) for w in one]
    assert (call >> 32) < 1 << 28               # the call's high word and the slot do not overlap


def test_mulhi_matches_python_integers():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 2 ** 64, 4096, dtype=np.uint64)
    x[:4] = [0, 1, 2 ** 64 - 1, 2 ** 63]
    for n in (1, 2, 7, 8, 120000, 2 ** 31 - 1):
        want = [(int(v) * n) >> 64 for v in x.tolist()]
        assert dr.mulhi64(x, n).tolist() == want
        assert max(want) < n


# ----------------------------------------------------------------------------------------------------------------- 2. distribution
def test_subset_distribution_on_fixed_seeds():
    """n = 64, k = 16, seeds 0 .. 19 999 (call 0, slot 0): the first position is uniform over the 64 values, and every value is
    included equally often."""
    T, n, k = 20000, 64, 16
    keys = dr.subset_keys(np.arange(T, dtype=np.uint64)[:, None], 0, 0, n)
    order = np.argsort(keys, axis=1, kind="stable")[:, :k]
    np.testing.assert_array_equal(order[7], dr.subset(7, 0, 0, n, k))                 # the batched form is the draw
    first = np.bincount(order[:, 0], minlength=n)
    chi_first = float(((first - T / n) ** 2 / (T / n)).sum())
    cnt = np.bincount(order.ravel(), minlength=n)
    chi_incl = float(((cnt - T * k / n) ** 2 / (T * (k / n) * (1 - k / n))).sum())
    print(f"subset draw, n 64 k 16, 20000 seeds: chi-square first position {chi_first:.2f} inclusion {chi_incl:.2f} bar {chi2_bar():.2f}")
    assert chi_first < chi2_bar()
    assert chi_incl < chi2_bar()


def test_pair_distribution_on_a_fixed_seed():
    N = 65536
    p = dr.pairs(0, 0, 0, N, 8, 8)
    cells = np.bincount(p[:, 0] * 8 + p[:, 1], minlength=64)
    chi = float(((cells - N / 64) ** 2 / (N / 64)).sum())
    print(f"pair draw, 8 x 8 cells, 65536 rows: chi-square {chi:.2f} bar {chi2_bar():.2f}")
    assert chi < chi2_bar()


# ----------------------------------------------------------------------------------------------------------------- 3. structure
SHAPES = [(1, 1), (5, 5), (64, 16), (257, 256), (1025, 3), (5000, 5000), (100003, 2048), (9, 0)]


def test_subsets_are_distinct_values_in_range_and_full_draws_are_permutations():
    for s, (n, k) in enumerate(SHAPES):
        got = dr.subset(3, 1, s, n, k)
        assert got.dtype == np.int64 and got.shape == (k,)
        assert len(np.unique(got)) == k and (got >= 0).all() and (got < n).all()
        if k == n:
            np.testing.assert_array_equal(np.sort(got), np.arange(n))
    assert dr.subset(3, 1, 0, 0, 0).shape == (0,)


def test_slots_and_calls_and_seeds_differ():
    a = dr.subsets(5, 0, [(5000, 5000), (5000, 5000)])
    assert not np.array_equal(a[0], a[1])
    assert not np.array_equal(a[0], dr.subset(5, 1, 0, 5000, 5000))
    assert not np.array_equal(a[0], dr.subset(5, 1 << 32, 0, 5000, 5000))           # the call's high word is read
    assert not np.array_equal(a[0], dr.subset(6, 0, 0, 5000, 5000))
    assert not np.array_equal(a[0], dr.subset(5 + (1 << 32), 0, 0, 5000, 5000))     # the seed's high word is read
    assert not np.array_equal(dr.pairs(5, 0, 0, 64, 1000, 1000), dr.pairs(5, 0, 1, 64, 1000, 1000))
    assert not np.array_equal(dr.pairs(5, 0, 0, 64, 1000, 1000), dr.pairs(5, 1, 0, 64, 1000, 1000))


def test_a_slot_alone_equals_the_slot_among_seven_others():
    together = dr.subsets(9, 4, SHAPES)
    for s, (n, k) in enumerate(SHAPES):
        alone = dr.subsets(9, 4, [(0, 0)] * s + [(n, k)])
        np.testing.assert_array_equal(alone[s], together[s])
        # a prefix of a longer draw of the same slot: k only cuts the order
        np.testing.assert_array_equal(dr.subset(9, 4, s, n, n)[:k], together[s])


def test_pairs_are_in_range():
    for N, n0, n1 in ((1, 1, 1), (257, 1, 7), (4099, 120000, 119999), (1024, 2 ** 31 - 1, 2)):
        p = dr.pairs(2, 3, 0, N, n0, n1)
        assert p.shape == (N, 2) and p.dtype == np.int64 and (p >= 0).all() and (p[:, 0] < n0).all() and (p[:, 1] < n1).all()
    assert len(np.unique(dr.pairs(2, 3, 0, 1024, 2 ** 31 - 1, 2)[:, 0])) == 1024       # 64-bit words: no two rows alike
    assert dr.pairs(2, 3, 0, 0, 5, 5).shape == (0, 2)


# ----------------------------------------------------------------------------------------------------------------- 4. DeviceDraws
def test_device_draws_call_numbering_and_argument_errors(monkeypatch):
    """Host logic only: nothing here reaches a device (an all-empty call launches nothing; the device lookup is stood in for)."""
    import torch

    import eyoc_amd
    from eyoc_amd import DeviceDraws, _lib
    from eyoc_amd import draws as D
    _lib.load()
    assert eyoc_amd.DeviceDraws is D.DeviceDraws and D.MAX_SLOTS == dr.MAX_SLOTS
    monkeypatch.setattr(D.DeviceDraws, "_device", lambda self, device=None: torch.device("cpu"))
    d = DeviceDraws(7)
    assert d.seed == 7 and d.call == 0
    out = d.subsets([(0, 0), (10, 0)])
    assert d.call == 1 and [tuple(o.shape) for o in out] == [(0,), (0,)] and all(o.dtype == torch.int64 for o in out)
    assert tuple(d.pairs(0, 5, 5).shape) == (0, 2) and d.call == 2
    assert d.subsets([]) == [] and d.call == 3
    # argument errors: EYOC_ERR_INVALID, raised before the device is looked at, and no call number is consumed
    for bad in (lambda: d.subsets([(3, 4)]), lambda: d.subsets([(-1, 0)]), lambda: d.subsets([(3, -1)]), lambda: d.subsets([(1, 1)] * 9),
                lambda: d.subsets([(2 ** 30, 1)] * 2), lambda: d.pairs(-1, 2, 2), lambda: d.pairs(1, -2, 2), lambda: d.pairs(4, 0, 2),
                lambda: d.pairs(4, 2, 0), lambda: d.pairs(1, 2, 2, slot=8), lambda: d.pairs(1, 2 ** 31, 2)):
        with pytest.raises(eyoc_amd.EyocError) as e:
            bad()
        assert e.value.code == _lib.ERR_INVALID and d.call == 3
    # .call is readable and settable: replay and resume
    d.call = 0
    assert d.call == 0
    d.call = (1 << 60) - 1
    d.subsets([(0, 0)])
    assert d.call == 1 << 60
    with pytest.raises(eyoc_amd.EyocError):            # the counter's 60 bits are used up
        d.subsets([(0, 0)])
    for v in (-1, 1 << 60):
        with pytest.raises(eyoc_amd.EyocError):
            d.call = v
    for s in (-1, 1 << 64):
        with pytest.raises(eyoc_amd.EyocError):
            DeviceDraws(s)
    assert DeviceDraws((1 << 64) - 1).seed == (1 << 64) - 1


def test_library_refuses_bad_arguments_before_any_launch():
    """The C entry points' own argument rules, on the host: every one of these returns before it touches a device."""
    import ctypes as C

    from eyoc_amd import _lib
    lib = _lib.load()
    assert lib.eyoc_draw_workspace_bytes(0) == 0 and lib.eyoc_draw_workspace_bytes(-5) == 0
    small, big = lib.eyoc_draw_workspace_bytes(1), lib.eyoc_draw_workspace_bytes(100003)
    assert small >= 24 and small % 256 == 0 and big >= 24 * 100003 and big % 256 == 0
    fake = C.c_void_p(4096)                             # a stand-in ctx / buffer: never dereferenced on these paths

    def sub(n, k, call=0, n_slots=None, ws_bytes=1 << 30):
        ns, ks = (C.c_int * len(n))(*n), (C.c_int * len(k))(*k)
        return lib.eyoc_draw_subsets(fake, 1, call, len(n) if n_slots is None else n_slots, ns, ks, fake, fake, ws_bytes, None)
    assert sub([3], [4]) == _lib.ERR_INVALID
    assert sub([-1], [0]) == _lib.ERR_INVALID
    assert sub([3], [-1]) == _lib.ERR_INVALID
    assert sub([1] * 9, [1] * 9) == _lib.ERR_INVALID
    assert sub([1], [1], n_slots=-1) == _lib.ERR_INVALID
    assert sub([1], [1], call=1 << 60) == _lib.ERR_INVALID
    assert sub([2 ** 30] * 2, [1, 1]) == _lib.ERR_INVALID
    assert sub([100003], [7], ws_bytes=big - 1) == _lib.ERR_WORKSPACE
    assert b"workspace" in lib.eyoc_last_error()
    assert sub([0, 5], [0, 0]) == 0 and sub([], []) == 0                       # all slots empty: nothing to launch
    assert lib.eyoc_draw_subsets(None, 1, 0, 0, None, None, None, None, 0, None) == _lib.ERR_INVALID
    for args in ((0, -1, 2, 2), (0, 1, -2, 2), (0, 1, 2, -2), (8, 1, 2, 2), (-1, 1, 2, 2), (0, 4, 0, 2), (0, 4, 2, 0)):
        assert lib.eyoc_draw_pairs(fake, 1, 0, *args, fake, None) == _lib.ERR_INVALID, args
    assert lib.eyoc_draw_pairs(fake, 1, 1 << 60, 0, 1, 2, 2, fake, None) == _lib.ERR_INVALID
    assert lib.eyoc_draw_pairs(fake, 1, 0, 0, 0, 0, 0, None, None) == 0        # no rows: nothing to launch
