"""CPU checks of the mutual nearest-neighbour feature (no GPU): the restatement the GPU tests compare against
(tests/mutual_restatement.py) obeys the contract's corner rules and is not vacuous on the GPU tests' inputs, its checker catches one
planted defect at a time, and the boundary: the built library exports the new entry points and is still version 111."""
import numpy as np
import pytest

import mutual_restatement as M


def _run(A, B, seg_a, seg_b, dist_type, min_keep=0, defect=None):
    idx_ab, idx_ba, flags = M.search(A, B, seg_a, seg_b, dist_type, defect)
    return (idx_ab, idx_ba, flags) + M.compact(idx_ab, flags, seg_a, min_keep, defect)


def test_library_exports_the_new_entry_points():
    from eyoc_amd import _lib
    lib = _lib.load()
    for name in ("eyoc_knn1_mutual", "eyoc_mutual_compact", "eyoc_knn_mutual_select"):
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES
    assert lib.eyoc_version() == 111
    assert lib.eyoc_knn_mutual_select(None, -2) == -1          # no ctx, no GPU: the query fails without touching anything


@pytest.mark.parametrize("dist_type", (0, 1, 2))
def test_column_minima_are_the_reverse_query(dist_type):
    """The restatement reads both directions off one matrix; the matrix of (B, A) is its transpose bit for bit."""
    for na, nb in ((65, 33), (31, 300)):
        A, B = M.pair_inputs(na, nb, 32)
        D, Dt = M.distance_matrix(A, B, dist_type), M.distance_matrix(B, A, dist_type)
        assert D.T.tobytes() == np.ascontiguousarray(Dt).tobytes() or np.array_equal(D.T, Dt, equal_nan=True)
        idx_ab, idx_ba, _ = M.segment(A, B, dist_type)
        assert np.array_equal(idx_ab, np.argmin(D, axis=1)) and np.array_equal(idx_ba, np.argmin(Dt, axis=1))


def test_no_case_is_vacuous():
    """Every GPU case with na, nb >= 32 has between 10 % and 90 % mutual rows."""
    seen = 0
    for na, nb in M.SHAPES:
        for c in (M.WIDTHS if (na, nb) in M.WIDE_SHAPES else (32,)):
            if min(na, nb) < 32:
                continue
            A, B = M.pair_inputs(na, nb, c)
            for dist_type in (0, 1, 2):
                share = M.mutual_share(M.segment(A, B, dist_type)[2])
                assert 0.10 <= share <= 0.90, (na, nb, c, dist_type, share)
                seen += 1
    assert seen >= 30


def test_ties_go_to_the_lowest_index_both_ways():
    A, B = M.pair_inputs(70, 40, 32)
    A[67] = A[3]
    B[37] = B[5]
    A[3] = A[67] = B[5]                                        # the duplicates are each other's nearest, at distance exactly 0
    idx_ab, idx_ba, flags = M.segment(A, B, 0)
    assert idx_ab[3] == 5 and idx_ab[67] == 5 and idx_ba[5] == 3 and idx_ba[37] == 3
    assert flags[3] == 3 and flags[67] == 2


def test_rows_without_a_neighbour_are_never_mutual():
    A, B = M.pair_inputs(20, 12, 32)
    A[4, 7] = np.nan
    B[0, 3] = np.nan
    idx_ab, idx_ba, flags = M.segment(A, B, 0)
    assert idx_ab[4] == 0 and flags[4] == 0 and idx_ba[0] == 0
    assert not (flags[idx_ab == 0] & 1).any()                  # nothing is mutual with the NaN target 0
    # an empty side: every index 0, no flags
    idx_ab, idx_ba, flags = M.segment(A, B[:0], 0)
    assert not idx_ab.any() and len(idx_ba) == 0 and not flags.any()
    # GemmL2 with rows of norm > 1: the first NaN wins, both ways
    A2, B2 = 3.0 * A, 3.0 * B
    A2[4], B2[0] = 3.0 * M.unit_rows(9, 1, 32)[0], 3.0 * M.unit_rows(10, 1, 32)[0]
    D = M.distance_matrix(A2, B2, 2)
    assert np.isnan(D).any()
    idx_ab, idx_ba, _ = M.segment(A2, B2, 2)
    for i in range(len(A2)):
        if np.isnan(D[i]).any():
            assert idx_ab[i] == np.flatnonzero(np.isnan(D[i]))[0]
    for j in range(len(B2)):
        if np.isnan(D[:, j]).any():
            assert idx_ba[j] == np.flatnonzero(np.isnan(D[:, j]))[0]


@pytest.mark.parametrize("k", (2, 3))
def test_fallback_case_has_an_exact_count(k):
    A, B = M.fallback_case(k)
    idx_ab, _, flags = M.segment(A, B, 0)
    assert int((flags & 1).sum()) == k + 1 and (flags >> 1).all()
    rows, corr, seg_out = M.compact(idx_ab, flags, [0, len(A)], min_keep=4)
    if k + 1 < 4:                                              # 3 mutual rows: all rows stay
        assert np.array_equal(rows, np.arange(len(A))) and seg_out[1] == len(A)
    else:                                                      # 4 mutual rows: exactly those
        assert np.array_equal(rows, np.flatnonzero(flags & 1)) and seg_out[1] == 4
    assert np.array_equal(corr, idx_ab[rows])
    assert M.compact(idx_ab, flags, [0, len(A)], min_keep=0)[2][1] == k + 1


def _defect_inputs(defect):
    if defect == "reverse_ties_high":                          # needs an exact tie in a column
        A, B = M.pair_inputs(70, 40, 32)
        A[3] = A[67] = B[5]
        return A, B, [0, 70], [0, 40], 0
    if defect == "fallback_le":                                # needs count == min_keep
        A, B = M.fallback_case(3)
        return A, B, [0, len(A)], [0, len(B)], 4
    if defect == "no_neighbour_mutual":                        # row 0 and target 0 without a neighbour: both indices read 0
        A, B = M.pair_inputs(20, 12, 32)
        A[0, 0] = B[0, 0] = np.nan
        return A, B, [0, 20], [0, 12], 0
    A, B = M.pair_inputs(65, 33, 32)
    return A, B, [0, 65], [0, 33], 0


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_checker_catches_a_planted_defect(defect):
    A, B, seg_a, seg_b, min_keep = _defect_inputs(defect)
    M.check(_run(A, B, seg_a, seg_b, 0, min_keep), A, B, seg_a, seg_b, 0, min_keep)          # the clean run passes
    with pytest.raises(AssertionError):
        M.check(_run(A, B, seg_a, seg_b, 0, min_keep, defect), A, B, seg_a, seg_b, 0, min_keep)


def test_config_refuses_the_filter_in_front_of_sc2pcr():
    from eyoc_amd.harness import RegistrationConfig
    assert RegistrationConfig().mutual_filter is False
    assert RegistrationConfig(mutual_filter=True).mutual_filter is True
    with pytest.raises(ValueError):
        RegistrationConfig(use_RANSAC=False, mutual_filter=True)
