"""Host-side checks of the batched validation step (no GPU): the fp64 restatement of the metrics kernel against the reference's own
outputs (``g12_valid.npz``), the meters, and the record layout."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import _inputs_valid as gv
from valid_restatement import check_against_g12, g12_cases, hit_distances, valid_record

from eyoc_amd import _lib
from eyoc_amd import validate as V


@pytest.fixture(scope="module")
def g12():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g12_valid.npz"))


def test_fixture_is_small_and_keeps_its_margin(g12):
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "g12_valid.npz")) < 100 * 1024
    cases = json.loads(str(g12["cases"]))
    assert sorted(c[1] for c in cases) == [3, 64, 777, 1025, 1500, 5000]
    assert all(0.35 <= c[2] <= 1.0 for c in cases)
    assert float(g12["margin"].min()) >= gv.MARGIN
    assert float(g12["loss_gap"].max()) < 1e-6
    for c, v, p0, p1, x0, T_est, T_gt in g12_cases(g12):
        assert len(x0) == 4 * len(p0) + 100
        assert np.abs(hit_distances(p0, p1, None, T_gt) - gv.HIT_THRESH).min() == pytest.approx(g12["margin"][c, v], rel=1e-9)


def test_restatement_matches_the_reference(g12):
    for c, v, p0, p1, x0, T_est, T_gt in g12_cases(g12):
        rec = valid_record(p0, p1, None, x0, T_est, T_gt, gv.HIT_THRESH)
        assert rec["status"] == 0 and rec["n_corr"] == len(p0) and rec["n_points"] == len(x0)
        check_against_g12(g12, c, v, rec, len(p0))
        if v == 1 and len(p0) >= 64:        # (three points follow their own noise)
            assert abs(rec["rre"] - np.deg2rad(2.0)) < 1e-3


def test_restatement_degenerate_pairs():
    p0, p1, x0, T_gt = gv.valid_case(44, 64, 0.9, (0.0, 0.0, 0.1, 1.0, 0.0, 0.0), False)
    r = valid_record(p0[:0], p1[:0], None, x0, T_gt, T_gt)
    assert r["status"] == V.EMPTY and np.isnan(r["hit_ratio"]) and np.isnan(r["loss"]) and r["rte"] == 0.0
    idx = np.arange(64); idx[5] = 64
    r = valid_record(p0, p1, idx, x0, T_gt, T_gt)
    assert r["status"] == V.BAD_INDEX and np.isnan(r["hit_ratio"]) and r["hits"] == 0 and r["loss"] == 0.0
    Tn = T_gt.copy(); Tn[1, 3] = np.inf
    r = valid_record(p0, p1, None, x0, Tn, T_gt)
    assert r["status"] == V.POSE_NONFINITE and np.isnan(r["loss"]) and np.isnan(r["rte"]) and np.isnan(r["rre"]) and r["hits"] > 0
    r = valid_record(p0, p1, None, x0[:0], T_gt, T_gt)
    assert r["status"] == 0 and np.isnan(r["loss"]) and r["hits"] > 0 and r["n_points"] == 0


def _records(rows):
    rec = np.zeros(len(rows), V.RECORD_DTYPE)
    for i, row in enumerate(rows):
        for k, val in row.items():
            rec[k][i] = val
    return rec


def test_meters_skip_nan_rre_in_its_mean_only():
    m = V.ValidMeters()
    m.update(_records([dict(loss=0.2, hit_ratio=0.5, rte=1.0, rre=0.1, n_corr=10),
                       dict(loss=0.4, hit_ratio=0.1, rte=3.0, rre=np.nan, n_corr=10)]))
    s = m.summary()
    assert list(s) == ["loss", "rre", "rte", "feat_match_ratio", "hit_ratio"]          # the reference's five, lib/trainer.py:397-403
    assert s["rre"] == pytest.approx(0.1) and s["loss"] == pytest.approx(0.3) and s["rte"] == pytest.approx(2.0)
    assert s["hit_ratio"] == pytest.approx(0.3) and s["feat_match_ratio"] == 1.0
    assert m.skipped == 0 and m.count == 2


def test_meters_skip_empty_pairs_everywhere_and_count_them():
    m = V.ValidMeters()
    m.update(_records([dict(loss=0.2, hit_ratio=0.5, rte=1.0, rre=0.1, n_corr=10),
                       dict(loss=np.nan, hit_ratio=np.nan, rte=np.nan, rre=np.nan, status=V.EMPTY | V.POSE_NONFINITE)]))
    m.update(_records([dict(loss=0.6, hit_ratio=0.0, rte=2.0, rre=0.3, n_corr=10)])[0])     # a single record
    s = m.summary()
    assert m.skipped == 1 and m.count == 2
    assert s == pytest.approx({"loss": 0.4, "rre": 0.2, "rte": 1.5, "feat_match_ratio": 0.5, "hit_ratio": 0.25})
    assert V.ValidMeters().summary() == {"loss": 0.0, "rre": 0.0, "rte": 0.0, "feat_match_ratio": 0.0, "hit_ratio": 0.0}


def test_feat_match_ratio_threshold_is_strict():
    m = V.ValidMeters()
    m.update(_records([dict(hit_ratio=0.05, n_corr=20), dict(hit_ratio=np.nextafter(0.05, 1.0), n_corr=20), dict(hit_ratio=0.0499, n_corr=20)]))
    assert m.summary()["feat_match_ratio"] == pytest.approx(1.0 / 3.0)


def test_decode_round_trips_a_hand_built_record():
    raw = struct.pack("<5d3iId", 0.25, 0.5, 1.5, 0.125, 0.75, 7, 14, 5100, 4, -2.0)
    assert len(raw) == 64
    r = V.decode_valid_records(raw + raw)
    assert r.shape == (2,)
    for rec in r:
        assert (rec["loss"], rec["hit_ratio"], rec["rte"], rec["rre"], rec["cos_rre"]) == (0.25, 0.5, 1.5, 0.125, 0.75)
        assert (rec["hits"], rec["n_corr"], rec["n_points"], rec["status"], rec["reserved"]) == (7, 14, 5100, 4, -2.0)
    assert r.tobytes() == raw + raw
    c = _lib.ValidRecord.from_buffer_copy(raw)
    assert (c.loss, c.cos_rre, c.hits, c.n_points, c.status, c.reserved) == (0.25, 0.75, 7, 5100, 4, -2.0)
    np.testing.assert_array_equal(V.decode_valid_records(np.frombuffer(raw, np.uint8).reshape(1, 64)), r[:1])
    with pytest.raises(ValueError):
        V.decode_valid_records(raw[:63])


def test_bound_struct_is_64_bytes():
    assert C.sizeof(_lib.ValidRecord) == 64 == V.RECORD_BYTES == V.RECORD_DTYPE.itemsize
    assert (V.EMPTY, V.BAD_INDEX, V.POSE_NONFINITE) == (1, 2, 4)
