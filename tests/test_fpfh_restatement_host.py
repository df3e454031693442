"""The FPFH restatement (tests/fpfh_restatement.py) checked on the host: analytic cases, the cap on undecided rows for the very inputs
the GPU test uses, and planted defects that the GPU test's comparison must notice.  No device compute."""
import numpy as np
import pytest

import fpfh_restatement as R

SEEDS = (3, 4)          # tests/test_gpu_fpfh.py uses the same


def test_planar_lattice_is_200_in_the_three_middle_bins():
    """All normals (0, 0, 1) on z = 0: every pair feature is exactly (0, 0, 0), so S has 100 in bins 5, 16, 27, and W / G there is 1."""
    pts, nrm = R.planar_lattice(6, extra_lone=2)
    ref = R.fpfh_rows(pts, nrm, 1.5, 40)
    want = np.zeros(33)
    want[[5, 16, 27]] = 200.0
    assert (ref.k[:36] >= 3).all() and not ref.undecided_F.any()
    for i in range(36):
        np.testing.assert_array_equal(ref.F[i], want)
        assert ref.cnt[i, 5] == ref.cnt[i, 16] == ref.cnt[i, 27] == ref.k[i] and ref.cnt[i].sum() == 3 * ref.k[i]
    # lone points: zero rows
    assert (ref.k[36:] == 0).all() and (ref.F[36:] == 0).all() and (ref.Fn[36:] == 0).all()
    R.check_against(ref, ref.cnt, ref.k, ref.F.astype(np.float32), ref.Fn.astype(np.float32))


def test_two_coincident_points_count_each_other_and_add_nothing_to_w():
    pts = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], np.float32)
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], np.float32)
    ref = R.fpfh_rows(pts, nrm, 0.5, 10)
    assert ref.k.tolist() == [1, 1] and ref.lists[0].tolist() == [1] and ref.lists[1].tolist() == [0]
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0                                   # S alone: W is empty (d2 = 0), G = 0
    np.testing.assert_array_equal(ref.F, np.stack([want, want]))
    assert np.isfinite(ref.Fn).all()


def test_list_is_cut_by_distance_then_row_and_excludes_the_row():
    pts, nrm = R.cubic_lattice(0, m=4)
    ref = R.fpfh_rows(pts, nrm, 0.6, 8)        # 0.25 lattice: 6 at 0.25, 12 at 0.354, 8 at 0.433 ... - the cut at 7 falls into a tie
    x = pts.astype(np.float64)
    for i in (0, 21, 42, 63):
        d2 = ((x - x[i]) ** 2).sum(1)
        order = sorted((d2[j], j) for j in range(len(x)) if d2[j] < 0.36)[:8]
        assert [j for _, j in order if j != i] == ref.lists[i].tolist()
        assert i not in ref.lists[i] and ref.k[i] == len(ref.lists[i]) <= 7


@pytest.mark.parametrize("seed", SEEDS)
def test_undecided_rows_stay_below_one_percent_on_the_gpu_tests_inputs(seed):
    pts, nrm = R.wavy_cloud(seed)
    ref = R.fpfh_rows(pts, nrm, **R.WAVY)
    assert ref.k.min() >= 1 and ref.k.max() < R.WAVY["max_nn"] - 1 and ref.k.sum() > 5000
    assert ref.undecided_F.mean() <= 0.01
    R.check_against(ref, ref.cnt, ref.k, ref.F.astype(np.float32), ref.Fn.astype(np.float32))
    pts, nrm = R.cubic_lattice(seed)
    assert R.fpfh_rows(pts, nrm, 0.6, 16).undecided_F.mean() <= 0.01


def defect_cloud():
    """The wavy cloud plus what two of the defects need: a duplicated point (d2 = 0 inside a list) and, far away, a pair of points whose
    normals make the same angle with the line between them (an exact tie of the swap test with different normals)."""
    pts, nrm = R.wavy_cloud(SEEDS[0], n=300, side=3.6)
    pts = np.concatenate([pts, pts[:1], np.array([[100.0, 0.0, 0.0], [100.25, 0.0, 0.0]], np.float32)])
    nrm = np.concatenate([nrm, nrm[1:2], np.array([[0.6, 0.8, 0.0], [0.6, 0.0, 0.8]], np.float32)])
    return pts, nrm


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_fails_the_comparison(defect):
    pts, nrm = defect_cloud()
    ref = R.fpfh_rows(pts, nrm, **R.WAVY)
    R.check_against(ref, ref.cnt, ref.k, ref.F.astype(np.float32), ref.Fn.astype(np.float32))
    wrong = R.fpfh_rows(pts, nrm, defect=defect, **R.WAVY)
    with np.errstate(over="ignore", invalid="ignore"):
        feat, featn = wrong.F.astype(np.float32), wrong.Fn.astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_against(ref, wrong.cnt, wrong.k, feat, featn)


def test_the_tie_of_the_swap_test_is_decided_without_a_swap():
    pts, nrm = defect_cloud()
    ref = R.fpfh_rows(pts[-2:], nrm[-2:], 0.45, 10)
    f, near = R.pair_features(pts[-2].astype(np.float64), nrm[-2].astype(np.float64), pts[-1:].astype(np.float64), nrm[-1:].astype(np.float64))
    assert not near.any() and f[0, 2] == np.float64(np.float32(0.6)) and not ref.undecided_hist.any()


def test_scene_generator_is_deterministic_and_moved_rigidly():
    src, tgt, T = R.corner_scene()
    src2, tgt2, _ = R.corner_scene()
    assert np.array_equal(src, src2) and np.array_equal(tgt, tgt2) and 250 < len(tgt) < len(src) < 400
    ok, rte, rre = R.registered(T, T)
    assert ok and rte == 0.0 and rre < 1e-5
    assert not R.registered(np.eye(4), T)[0]


def test_shim_transform_rotates_the_normals_with_the_points():
    import eyoc_amd.o3d as o3d
    pts, nrm = R.wavy_cloud(SEEDS[0], n=20)
    pcd = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(pts))
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [1.0, 2.0, 3.0]
    pcd.transform(T)                                          # no normals: nothing but the points moves
    assert len(pcd.normals) == 0 and not pcd.has_normals()
    pcd.normals = o3d.utility.Vector3dVector(nrm)
    before = pcd.points.copy()
    pcd.transform(T)
    np.testing.assert_array_equal(pcd.points, before @ T[:3, :3].T + T[:3, 3])
    np.testing.assert_array_equal(pcd.normals, nrm.astype(np.float64) @ T[:3, :3].T)     # rotated, not translated
    assert pcd.has_normals()
