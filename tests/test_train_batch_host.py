"""Host side of the training-batch path (eyoc_amd/trainbatch.py): ``draw_augmentation`` against the reference's own
``sample_random_trans`` / ``apply_transform`` (G13, tests/golden/make_golden_trainbatch.py), and the fp64 restatement the GPU tests
compare the kernels with (tests/trainbatch_restatement.py) against the reference's posed points and against answers known by hand."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import trainbatch_cases as cases
import trainbatch_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g13():
    g = np.load(os.path.join(HERE, "golden", "g13_augment.npz"))
    table = [tuple(c) for c in json.loads(str(g["cases"]))]
    assert table == [tuple(c) for c in R.g13_cases()]
    return g, table


def test_draws_match_the_reference(g13):
    """Same draws consumed, R within 1e-14 (``expm``'s own rounding; 2.7e-15 measured), and R (-mean64) within n 2^-24 max|x| of the
    reference's translation - the worst case of its fp32 accumulation of the mean."""
    from eyoc_amd.trainbatch import draw_augmentation
    g, table = g13
    for c, (seed, n, rr) in enumerate(table):
        randg = np.random.RandomState(seed)
        rot, scale = draw_augmentation(randg, 1, rotation_range=rr)
        assert randg.rand() == g["next_u"][c], f"case {c}: the generator is not where the reference leaves it"
        assert rot.shape == (2, 3, 3) and rot.dtype == np.float64 and scale.tolist() == [1.0]
        for i in (0, 1):
            T = g["T"][c, i]
            assert np.abs(rot[i] - T[:3, :3]).max() <= 1e-14, (c, i)
            assert np.abs(rot[i] - R.rodrigues(*_axis_angle(seed, rr, i))).max() == 0.0
            xyz = R.g13_cloud(seed, n, i)
            t = R.cloud_pose(rot[i], xyz.astype(np.float64).mean(0))[:3, 3]
            bound = n * 2.0 ** -24 * float(np.abs(xyz).max())
            assert np.abs(t - T[:3, 3]).max() <= bound, (c, i, np.abs(t - T[:3, 3]).max(), bound)


def _axis_angle(seed, rr, i):
    randg = np.random.RandomState(seed)
    for _ in range(i + 1):
        axis, u = randg.rand(3) - 0.5, randg.rand(1)
    return axis, rr * np.pi / 180.0 * (u[0] - 0.5)


def test_draw_order_with_scaling():
    """Per pair: two rotations from ``randg``, then ``random() < 0.95`` and, if true, a second ``random()`` from ``pyrandom``."""
    import random
    from eyoc_amd.trainbatch import draw_augmentation
    rot, scale = draw_augmentation(np.random.RandomState(3), 40, random_scale=True, pyrandom=random.Random(9))
    ref, want = random.Random(9), []
    for _ in range(40):
        want.append(0.8 + (1.2 - 0.8) * ref.random() if ref.random() < 0.95 else 1.0)
    assert scale.tolist() == want and 1.0 in want
    assert np.array_equal(rot, draw_augmentation(np.random.RandomState(3), 40)[0])
    same, ones = draw_augmentation(None, 2, random_rotation=False)
    assert np.array_equal(same, np.tile(np.eye(3), (4, 1, 1))) and ones.tolist() == [1.0, 1.0]
    assert np.abs(np.einsum("bij,bkj->bik", rot, rot) - np.eye(3)).max() < 1e-15 * 8


def test_restated_posed_points_match_apply_transform(g13):
    """1e-12 relative: BLAS may associate the three products differently, so this is not a bit test.  Relative to the terms that are
    summed - the largest coordinate plus the largest translation -, not to the result: a centred cloud of one point is posed onto the
    origin, where only the terms' rounding is left."""
    g, table = g13
    for c, (seed, n, rr) in enumerate(table):
        for i in (0, 1):
            want, T = g[f"posed{c}_{i}"], g["T"][c, i]
            xyz = R.g13_cloud(seed, n, i)
            got = R.pose_points(xyz, T)
            assert got.shape == want.shape == (n, 3)
            assert np.abs(got - want).max() <= 1e-12 * (float(np.abs(xyz).max()) + np.abs(T[:3, 3]).max()), (c, i)


def test_restated_pose_composition():
    rng = np.random.default_rng(2)
    for scale in (None, 1.17):
        T0, T1, M2 = (cases.rigid(rng, 300.0) for _ in range(3))
        want = T1 @ M2 @ np.linalg.inv(T0)
        if scale is not None:
            want[:3, 3] = scale * want[:3, 3]
        np.testing.assert_allclose(R.compose(T0, T1, M2, scale), want, rtol=1e-12, atol=1e-10)


def test_restated_quantiser_on_hand_made_faces():
    clouds, coords, sel, xyz, offsets = cases.hand_faces()
    eye = [np.eye(4)] * 2
    got = R.quantize_posed(clouds, eye, None, cases.HAND_VOXEL)
    assert np.array_equal(got[0], coords) and got[0].dtype == np.int32
    assert np.array_equal(got[1], sel)
    assert got[2].tobytes() == xyz.tobytes()
    assert np.array_equal(got[3], offsets) and not got[4].any()
    # the same voxel in two clouds: both kept, the batch indices differ
    assert coords[-1].tolist() == [1, 20, 20, 20] and [0, 20, 20, 20] in coords[:-1].tolist()
    based = R.quantize_posed(clouds, eye, [1.0, 1.0], cases.HAND_VOXEL, batch_base=7)
    assert np.array_equal(based[0][:, 1:], coords[:, 1:]) and np.array_equal(based[0][:, 0], coords[:, 0] + 7)


def test_restated_quantiser_faults():
    clouds = cases.general_clouds()
    poses = [cases.rigid(np.random.default_rng(b), 5.0) for b in range(len(clouds))]
    clean = R.quantize_posed(clouds, poses, None, 0.3, isolate=True)
    assert not clean[4].any() and np.diff(clean[3]).tolist()[:2] == [0, 1] and clean[3][-1] < sum(cases.GENERAL_SIZES) * 0.8
    bad = [c.copy() for c in clouds]
    bad[2][17, 1] = np.nan
    bad[4][200] = (1e6, 0.0, 0.0)
    iso = R.quantize_posed(bad, poses, None, 0.3, isolate=True)
    assert iso[4].tolist() == [[0, 0], [0, 0], [0, 1], [0, 0], [1, 0], [0, 0]]
    assert np.diff(iso[3])[[2, 4]].tolist() == [0, 0]
    with pytest.raises(R.RangeFault) as e:
        R.quantize_posed(bad, poses, None, 0.3)
    assert e.value.cloud == 2


def test_workspace_sizes_and_null_arguments():
    """The host side of the three entry points, as far as it goes without a device."""
    from eyoc_amd import _lib
    lib = _lib.load()
    assert lib.eyoc_voxelize_batched_posed_workspace_bytes(1000, 4) >= lib.eyoc_voxelize_batched_isolating_workspace_bytes(1000, 4) + 12 * 1000
    assert lib.eyoc_cloud_centroids_workspace_bytes(3 * 4096 + 1, 5) >= (3 + 5) * 24       # a partial sum per started tile of every cloud
    assert lib.eyoc_cloud_centroids_workspace_bytes(-1, 1) == 0 and lib.eyoc_voxelize_batched_posed_workspace_bytes(10, 0) == 0
    off = np.zeros(2, np.int64)
    i64 = C.POINTER(C.c_int64)
    assert lib.eyoc_cloud_centroids(None, None, 3, off.ctypes.data_as(i64), 1, 0, None, None, 0, None) == _lib.ERR_INVALID
    assert b"eyoc_cloud_centroids: NULL argument" in lib.eyoc_last_error()
    assert lib.eyoc_augment_poses(None, None, None, None, None, 1, None, None, None) == _lib.ERR_INVALID
    assert lib.eyoc_voxelize_batched_posed(None, None, 3, off.ctypes.data_as(i64), 1, 0, None, None, 0.3, 0, None, None, None,
                                           off.ctypes.data_as(i64), None, 0, None, None) == _lib.ERR_INVALID
    assert b"eyoc_voxelize_batched_posed" in lib.eyoc_last_error()
