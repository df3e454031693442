"""An ``open3d``-shaped namespace for the Open3D calls on the registration path: feature-matching RANSAC and point-to-point ICP.

``scripts/test_kitti.py:159-177`` builds point clouds and features with ``util/pointcloud.py:9-21``
(``o3d.geometry.PointCloud()``, ``o3d.utility.Vector3dVector``, ``o3d.pipelines.registration.Feature()`` with
``resize(dim, n)`` and a ``data`` array of shape ``[dim, n]`` in float64) and calls
``o3d.pipelines.registration.registration_ransac_based_on_feature_matching(pcd0, pcd1, feat0, feat1, False, d,
TransformationEstimationPointToPoint(False), 4, [CorrespondenceCheckerBasedOnEdgeLength(0.9),
CorrespondenceCheckerBasedOnDistance(d)], RANSACConvergenceCriteria(4000000, 10000))``.  With

    import eyoc_amd.o3d as o3d

those lines run unchanged; the work happens in ``libeyoc_hip.so`` (``eyoc_amd.registration``).  Only what that call site
touches exists here - this is not an Open3D re-implementation: other estimation methods and ``ransac_n != 4`` raise
``NotImplementedError``, unknown checkers raise ``TypeError``.  ``mutual_filter=True`` (the reference passes False) keeps the reciprocal
feature matches only, all of them when fewer than ``ransac_n`` are reciprocal, like Open3D.

``o3d.pipelines.registration.registration_icp(pcd0, pcd1, 0.2, np.eye(4), TransformationEstimationPointToPoint(),
ICPConvergenceCriteria(max_iteration=200))`` and ``pcd0.transform(reg.transformation)`` (``lib/data_loaders.py:497-507``) and the legacy
``o3d.registration.registration_icp`` of ``scripts/SC2_PCR/benchmark_utils.py:52-54`` run unchanged as well (``eyoc_amd.icp``);
``TransformationEstimationPointToPoint(with_scaling=True)`` and point-to-plane raise ``NotImplementedError``.  Point-to-plane ICP itself
exists (``eyoc_amd.icp.registration_icp_point_to_plane``, with ``estimate_normals`` for the target's normals); this shim keeps refusing
``TransformationEstimationPointToPlane``: its ``PointCloud`` carries normals for the FPFH route below only.

The hand-crafted descriptor of ``scripts/SC2_PCR/dataset.py:66-74`` runs as written too: ``pcd.estimate_normals(
o3d.geometry.KDTreeSearchParamHybrid(radius, max_nn))`` and ``o3d.pipelines.registration.compute_fpfh_feature(pcd,
o3d.geometry.KDTreeSearchParamHybrid(radius, max_nn))`` (``eyoc_amd.fpfh``; the result is a ``Feature`` with ``[33, n]`` float64 ``data``).
The normals point to the origin (Open3D leaves the sign to the eigen-solver), and FPFH depends on that sign.  Only the hybrid search
parameter exists.

``pcd.voxel_down_sample(voxel_size)``, the first call of every Open3D global-registration program and of ``util/pointcloud.py:38,43-44``,
returns a new ``PointCloud`` of voxel centroids (``eyoc_amd.downsample``); ``voxel_down_sample_and_trace`` does not exist.
"""
from __future__ import annotations

import types

import numpy as np

from . import registration as _reg


def _vector3d(a):
    """``o3d.utility.Vector3dVector``: an ``[n, 3]`` float64 array."""
    a = np.ascontiguousarray(np.asarray(a), dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"Vector3dVector needs an [n, 3] array, got {a.shape}")
    return a


class PointCloud:
    """``o3d.geometry.PointCloud``: ``points`` / ``colors`` holders (util/pointcloud.py:9-14)."""

    def __init__(self, points=None):
        self.points = np.zeros((0, 3)) if points is None else _vector3d(points)
        self.colors = np.zeros((0, 3))
        self.normals = np.zeros((0, 3))

    def has_normals(self):
        return len(self.normals) == len(self.points) and len(self.points) > 0

    def estimate_normals(self, search_param=None):
        """``normals`` <- ``eyoc_amd.icp.estimate_normals`` (float64 ``[n, 3]``, towards the origin); the hybrid search parameter only."""
        from . import icp as _icp
        if not isinstance(search_param, KDTreeSearchParamHybrid):
            raise NotImplementedError("estimate_normals needs a KDTreeSearchParamHybrid(radius, max_nn)")
        n = _icp.estimate_normals(np.asarray(self.points, np.float32), search_param.radius, search_param.max_nn)
        self.normals = n.cpu().numpy().astype(np.float64)
        return self

    def voxel_down_sample(self, voxel_size):
        """``o3d.geometry.PointCloud.voxel_down_sample`` (util/pointcloud.py:38,43-44) -> a new ``PointCloud``: one point per occupied
        voxel, the mean of the voxel's points (``eyoc_amd.downsample``: grid anchored half a voxel below the minimum corner, fp64 sums
        in point order, float32 in and out), rows ordered by the voxel's lowest point index.  The shim's rule for normals: they go
        through the same call as attributes, and every mean is then scaled to unit length; a zero mean stays zero.  Colours are not
        carried.  Open3D is not part of any build here, so this follows its documented behaviour, not a comparison."""
        from . import _lib, downsample as _ds
        if not len(self.points):
            raise RuntimeError("voxel_down_sample: the cloud has no points")
        p = np.asarray(self.points, np.float32)
        out = PointCloud()
        if self.has_normals():
            xyz, _, status, nrm = _ds.voxel_down_sample_batched(p, [0, len(p)], voxel_size, attrs=np.asarray(self.normals, np.float32))
        else:
            xyz, _, status = _ds.voxel_down_sample_batched(p, [0, len(p)], voxel_size)
            nrm = None
        if int(status[0]) != 0:
            raise _lib.EyocError("voxel_down_sample: a point is not finite or the cloud spans more than 2^17 cells on an axis",
                                 _lib.ERR_RANGE)
        out.points = xyz.cpu().numpy().astype(np.float64)
        if nrm is not None:
            m = nrm.cpu().numpy().astype(np.float64)
            length = np.sqrt((m * m).sum(1, keepdims=True))
            out.normals = np.divide(m, length, out=np.zeros_like(m), where=length > 0)
        return out

    def __len__(self):
        return len(self.points)

    def transform(self, T):
        """In place, like Open3D: ``points <- R points + t``, ``normals <- R normals`` (where the cloud carries normals)."""
        T = np.asarray(T, np.float64)
        self.points = self.points @ T[:3, :3].T + T[:3, 3]
        if len(self.normals):
            self.normals = np.asarray(self.normals, np.float64) @ T[:3, :3].T
        return self


class KDTreeSearchParamHybrid:
    """``o3d.geometry.KDTreeSearchParamHybrid``: the neighbours inside ``radius``, at most the ``max_nn`` nearest."""

    def __init__(self, radius, max_nn):
        self.radius = float(radius)
        self.max_nn = int(max_nn)


class Feature:
    """``o3d.pipelines.registration.Feature``: ``data`` is ``[dim, n]`` float64 (util/pointcloud.py:17-21)."""

    def __init__(self):
        self.data = np.zeros((0, 0))

    def resize(self, dim, n):
        self.data = np.zeros((int(dim), int(n)))

    def dimension(self):
        return self.data.shape[0]

    def num(self):
        return self.data.shape[1]


class TransformationEstimationPointToPoint:
    def __init__(self, with_scaling=False):
        self.with_scaling = bool(with_scaling)


class TransformationEstimationPointToPlane:
    """Exists so that a call site that builds one gets the shim's ``NotImplementedError`` from ``registration_icp``, not an AttributeError."""

    def __init__(self, kernel=None):
        self.kernel = kernel


class ICPConvergenceCriteria:
    def __init__(self, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
        self.relative_fitness = float(relative_fitness)
        self.relative_rmse = float(relative_rmse)
        self.max_iteration = int(max_iteration)


class CorrespondenceCheckerBasedOnEdgeLength:
    def __init__(self, similarity_threshold=0.9):
        self.similarity_threshold = float(similarity_threshold)


class CorrespondenceCheckerBasedOnDistance:
    def __init__(self, distance_threshold):
        self.distance_threshold = float(distance_threshold)


class RANSACConvergenceCriteria:
    """``confidence`` is clamped to [0, 1] like Open3D >= 0.12 does; at 1 (the reference passes 10000) there is no early
    exit and every one of ``max_iteration`` hypotheses is evaluated; below 1 a pair stops at the first checkpoint at which its best
    fitness meets the criterion (``eyoc_amd.registration.ransac_batched_from_correspondences``; 0 is refused by the call)."""

    def __init__(self, max_iteration=100000, confidence=0.999):
        self.max_iteration = int(max_iteration)
        self.confidence = float(min(max(confidence, 0.0), 1.0))


RegistrationResult = _reg.RegistrationResult


def compute_fpfh_feature(input, search_param):
    """``o3d.pipelines.registration.compute_fpfh_feature``: the cloud must carry normals (``estimate_normals``) -> ``Feature`` with
    ``data`` ``[33, n]`` float64, the fp32 rows of ``eyoc_amd.fpfh.compute_fpfh_feature`` widened."""
    from . import fpfh as _fpfh
    if not isinstance(input, PointCloud):
        raise TypeError("input must be eyoc_amd.o3d.geometry.PointCloud")
    if not isinstance(search_param, KDTreeSearchParamHybrid):
        raise NotImplementedError("compute_fpfh_feature needs a KDTreeSearchParamHybrid(radius, max_nn)")
    if not input.has_normals():
        raise RuntimeError("compute_fpfh_feature: the cloud has no normals (call estimate_normals first)")
    rows = _fpfh.compute_fpfh_feature(np.asarray(input.points, np.float32), search_param.radius, search_param.max_nn,
                                      normals=np.asarray(input.normals, np.float32))
    f = Feature()
    f.data = np.ascontiguousarray(rows.cpu().numpy().astype(np.float64).T)
    return f


def _knn_rows(feature):
    """``[dim, n]`` float64 -> ``[n, dim]`` float32 rows; FPFH's 33 columns are padded with zeros to 64, a width the neighbour search takes
    (zero columns change no distance)."""
    rows = np.ascontiguousarray(feature.data.T, np.float32)
    if rows.shape[1] == 33:
        rows = np.concatenate([rows, np.zeros((rows.shape[0], 31), np.float32)], 1)
    return rows


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                                  max_correspondence_distance, estimation_method=None, ransac_n=3, checkers=(),
                                                  criteria=None, seed=0):
    """Positional layout of Open3D >= 0.12 (the 5th argument is ``mutual_filter``: RANSAC over the reciprocal matches, ``fitness`` over
    the correspondences used - ``eyoc_amd.registration``).  ``seed`` is an extension: Open3D draws
    from ``std::random_device``; here hypothesis ``h`` samples with the counter hash of ``oracle/ransac.py``."""
    if not isinstance(source, PointCloud) or not isinstance(target, PointCloud):
        raise TypeError("source / target must be eyoc_amd.o3d.geometry.PointCloud")
    if not isinstance(source_feature, Feature) or not isinstance(target_feature, Feature):
        raise TypeError("source_feature / target_feature must be eyoc_amd.o3d.pipelines.registration.Feature")
    if estimation_method is None:
        estimation_method = TransformationEstimationPointToPoint(False)
    if not isinstance(estimation_method, TransformationEstimationPointToPoint) or estimation_method.with_scaling:
        raise NotImplementedError("only TransformationEstimationPointToPoint(False) is implemented (scripts/test_kitti.py:173)")
    criteria = RANSACConvergenceCriteria() if criteria is None else criteria
    if not criteria.confidence > 0.0:
        raise ValueError(f"RANSACConvergenceCriteria.confidence = {criteria.confidence!r}: must be above 0")
    edge, dist = None, None
    for c in checkers or ():
        if isinstance(c, CorrespondenceCheckerBasedOnEdgeLength):
            edge = c.similarity_threshold
        elif isinstance(c, CorrespondenceCheckerBasedOnDistance):
            dist = c.distance_threshold
        else:
            raise TypeError(f"unsupported correspondence checker {type(c).__name__}")
    if edge is None or dist is None:
        raise NotImplementedError("the kernels apply both the edge-length and the distance checker (scripts/test_kitti.py:174-175)")
    if abs(dist - float(max_correspondence_distance)) > 1e-12 * max(1.0, abs(dist)):
        raise NotImplementedError("the distance checker's threshold must equal max_correspondence_distance (as in the reference)")
    if source_feature.num() != len(source) or target_feature.num() != len(target):
        raise ValueError("features and points disagree in length")
    return _reg.registration_ransac_based_on_feature_matching(
        np.asarray(source.points, np.float32), np.asarray(target.points, np.float32),
        _knn_rows(source_feature), _knn_rows(target_feature),
        mutual_filter, float(max_correspondence_distance), None, ransac_n, None, (criteria.max_iteration, criteria.confidence),
        seed=seed, edge_similarity=edge, confidence=min(float(criteria.confidence), 1.0))     # Open3D clamps the confidence to 1


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """Point-to-point ICP with Open3D's positional layout (``init`` defaults to the identity, ``criteria`` to
    ``ICPConvergenceCriteria()``); the points are handed to the GPU as float32, like every cloud of this package."""
    from . import icp as _icp
    if not isinstance(source, PointCloud) or not isinstance(target, PointCloud):
        raise TypeError("source / target must be eyoc_amd.o3d.geometry.PointCloud")
    if estimation_method is None:
        estimation_method = TransformationEstimationPointToPoint(False)
    if not isinstance(estimation_method, TransformationEstimationPointToPoint):
        raise NotImplementedError("only point-to-point ICP is implemented (lib/data_loaders.py:501-502)")
    if estimation_method.with_scaling:
        raise NotImplementedError("TransformationEstimationPointToPoint(with_scaling=True) is not implemented")
    criteria = ICPConvergenceCriteria() if criteria is None else criteria
    if not isinstance(criteria, ICPConvergenceCriteria):
        raise TypeError("criteria must be an ICPConvergenceCriteria")
    return _icp.registration_icp(np.asarray(source.points, np.float32), np.asarray(target.points, np.float32),
                                 float(max_correspondence_distance), np.eye(4) if init is None else init, estimation_method, criteria)


geometry = types.SimpleNamespace(PointCloud=PointCloud, KDTreeSearchParamHybrid=KDTreeSearchParamHybrid)
utility = types.SimpleNamespace(Vector3dVector=_vector3d)
pipelines = types.SimpleNamespace(registration=types.SimpleNamespace(
    Feature=Feature, TransformationEstimationPointToPoint=TransformationEstimationPointToPoint,
    CorrespondenceCheckerBasedOnEdgeLength=CorrespondenceCheckerBasedOnEdgeLength,
    CorrespondenceCheckerBasedOnDistance=CorrespondenceCheckerBasedOnDistance,
    RANSACConvergenceCriteria=RANSACConvergenceCriteria, RegistrationResult=RegistrationResult,
    registration_ransac_based_on_feature_matching=registration_ransac_based_on_feature_matching,
    TransformationEstimationPointToPlane=TransformationEstimationPointToPlane, ICPConvergenceCriteria=ICPConvergenceCriteria,
    registration_icp=registration_icp, compute_fpfh_feature=compute_fpfh_feature))
registration = pipelines.registration      # the pre-0.10 module path scripts/SC2_PCR/benchmark_utils.py:52-54 uses
