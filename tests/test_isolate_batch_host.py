"""Host side of per-pair failure isolation (no GPU): defaults, status bits, NULL-ctx refusals of the new entry points, the cloud -> pair
mapping, the segment layout with empty segments, the numpy model of the drop, and the bound on rebuilds with a stubbed build."""
import ctypes as C

import numpy as np
import pytest

from eyoc_amd import _lib
from eyoc_amd import harness as h


def test_isolation_is_off_by_default_and_bits_do_not_collide():
    cfg = h.RegistrationConfig()
    assert cfg.isolate_failures is False and cfg.fp32_retry_per_step is False
    bits = [h.DROPPED_DUPLICATE, h.DROPPED_RANGE, h.DROPPED_EMPTY, h.DROPPED_NONFINITE]
    assert bits == [1, 2, 4, 8] and h.DROPPED == 15 and h.RETRIED_FP32 == 16 and not h.DROPPED & h.RETRIED_FP32
    assert h.MAX_REBUILDS == 2
    step = h.PendingStep(None, None, None, None)
    assert step.dropped is None and step.status is None


def test_new_entry_points_refuse_a_null_ctx():
    lib = _lib.load()
    mask = np.zeros(32, np.uint32)
    n = C.c_int(7)
    assert lib.eyoc_batch_drop(None, None, None, 0, 0, mask.ctypes.data, None, None, None, C.byref(n), None, None, 0, None) == _lib.ERR_INVALID
    assert b"eyoc_batch_drop" in lib.eyoc_last_error()
    assert lib.eyoc_remap_rows(None, None, 0, None, 0, None, None) == _lib.ERR_INVALID
    off = np.zeros(2, np.int64)
    vox = np.zeros(2, np.int64)
    faults = np.zeros(2, np.int32)
    i64 = C.POINTER(C.c_int64)
    rc = lib.eyoc_voxelize_batched_isolating(None, None, 3, off.ctypes.data_as(i64), 1, 0, 0.3, 0, None, None, None, vox.ctypes.data_as(i64),
                                             None, 0, None, faults.ctypes.data)
    assert rc == _lib.ERR_INVALID and b"eyoc_voxelize_batched_isolating: NULL argument" in lib.eyoc_last_error()
    # sizes: the isolating voxeliser needs two counters per cloud (+ padding, 256-byte granules) more; the drop 4 bytes per row + its tables
    assert lib.eyoc_voxelize_batched_isolating_workspace_bytes(1000, 64) == lib.eyoc_voxelize_batched_workspace_bytes(1000, 64) + 768
    assert lib.eyoc_batch_drop_workspace_bytes(-1) == 0
    assert lib.eyoc_batch_drop_workspace_bytes(1 << 20) >= 4 << 20


def test_clouds_map_to_pairs_through_the_offsets():
    offsets = np.array([0, 10, 20, 20, 35, 50, 61])              # 6 clouds = 3 pairs, one of them empty
    assert h.pairs_of_clouds([0, 1, 2, 5], offsets, 3).tolist() == [0, 0, 1, 2]
    assert h.pairs_of_clouds([], offsets, 3).tolist() == []
    with pytest.raises(ValueError):
        h.pairs_of_clouds([6], offsets, 3)                        # not a cloud of this batch
    with pytest.raises(ValueError):
        h.pairs_of_clouds([0], offsets, 4)                        # 6 clouds are not 4 pairs
    bits = h.fault_bits([3], [0, 3, 4], offsets, 3)
    assert bits.tolist() == [h.DROPPED_RANGE, h.DROPPED_DUPLICATE | h.DROPPED_RANGE, h.DROPPED_RANGE]


def test_segments_keep_a_slot_for_a_dropped_pair():
    seg = h.live_segments([0, h.DROPPED_RANGE, 0, 0, h.DROPPED_EMPTY], 5)
    assert seg.tolist() == [0, 5, 5, 10, 15, 15] and seg.dtype == np.int64
    assert h.live_segments(np.zeros(4, np.int64), 7).tolist() == (np.arange(5) * 7).tolist()
    assert h.live_segments([1, 2], 9).tolist() == [0, 0, 0]


def test_numpy_model_of_the_drop_agrees_with_delete():
    from eyoc_amd.isolate import batch_mask, drop_model
    coords = np.array([[0, 1, 1, 1], [3, 2, 2, 2], [0, 3, 3, 3], [5, 4, 4, 4], [3, 5, 5, 5], [1024, 6, 6, 6], [700, 7, 7, 7]], np.int32)
    feats = np.arange(14, dtype=np.float32).reshape(7, 2)
    mask = batch_mask([3, 700, 44])
    assert mask[0] == 1 << 3 and mask[1] == 1 << 12 and mask[21] == 1 << 28 and np.count_nonzero(mask) == 3
    c, f, row_map, kept = drop_model(coords, feats, mask)
    gone = [1, 4, 6]
    np.testing.assert_array_equal(c, np.delete(coords, gone, 0))
    np.testing.assert_array_equal(f, np.delete(feats, gone, 0))
    assert row_map.tolist() == [0, -1, 1, 2, -1, 3, -1]
    assert kept[0] == 2 and kept[5] == 1 and kept.sum() == 3      # the row of batch index 1024 stays and is counted nowhere
    with pytest.raises(ValueError):
        batch_mask([1024])


class _FakeBatch:
    """What ``build_with_isolation`` needs of a batch."""

    def __init__(self, P, dropped=None, log=None):
        self.P, self.offsets = P, np.arange(2 * P + 1) * 10
        self.dropped = np.zeros(P, np.int64) if dropped is None else dropped
        self.log = [] if log is None else log

    def without_pairs(self, bits):
        self.log.append(np.asarray(bits).tolist())
        return _FakeBatch(self.P, self.dropped | bits, self.log)


def test_rebuilds_are_bounded_and_the_original_error_is_raised():
    src = _FakeBatch(4)
    calls = []

    def always_fails(b):
        calls.append(b)
        code = _lib.ERR_RANGE if len(calls) == 1 else _lib.ERR_DUPLICATE
        raise _lib.EyocError(f"failure {len(calls)}", code)
    faults = iter([([], [2]), ([5], []), ([1], [])])
    with pytest.raises(_lib.EyocError) as ei:
        h.build_with_isolation(src, always_fails, lambda: next(faults))
    assert str(ei.value) == "failure 1" and ei.value.code == _lib.ERR_RANGE       # the third failure ends it: the original error
    assert len(calls) == 3 and calls[0] is src and not src.dropped.any()
    assert src.log == [[0, h.DROPPED_RANGE, 0, 0], [0, 0, h.DROPPED_DUPLICATE, 0]]
    assert calls[2].dropped.tolist() == [0, h.DROPPED_RANGE, h.DROPPED_DUPLICATE, 0]

    # two rebuilds are allowed
    n = []

    def third_time_lucky(b):
        n.append(b)
        if len(n) < 3:
            raise _lib.EyocError("x", _lib.ERR_DUPLICATE)
        return "maps"
    faults = iter([([0], []), ([7], [])])
    out, reduced = h.build_with_isolation(_FakeBatch(4), third_time_lucky, lambda: next(faults))
    assert out == "maps" and reduced.dropped.tolist() == [h.DROPPED_DUPLICATE, 0, 0, h.DROPPED_DUPLICATE]

    # no mask bit (a row whose own batch index is out of range), or only pairs that are gone already: raised as it is, no rebuild
    for fault, dropped in ((([], []), None), (([2], []), np.array([0, h.DROPPED_EMPTY, 0, 0]))):
        tries = []

        def fails(b):
            tries.append(b)
            raise _lib.EyocError("as it is", _lib.ERR_RANGE)
        with pytest.raises(_lib.EyocError, match="as it is"):
            h.build_with_isolation(_FakeBatch(4, dropped), fails, lambda: fault)
        assert len(tries) == 1

    # any other error passes through untouched
    def broken(b):
        raise _lib.EyocError("hip", _lib.ERR_HIP)
    with pytest.raises(_lib.EyocError, match="hip"):
        h.build_with_isolation(_FakeBatch(2), broken, lambda: pytest.fail("not asked"))
