"""eyoc_amd - MI355X-native implementation of EYOC's registration hot path.

Public names follow the reference (liuQuan98/EYOC): ``SparseTensor``, ``load_model`` /
``ResUNetBN2C``, ``find_nn_gpu`` / ``pdist`` / ``find_corr``, ``est_quad_linear_robust`` /
``pose_estimation``, ``rigid_transform_3d``, ``Matcher``; plus the two aliases named by the project
brief, ``find_correspondences`` and ``estimate_transform``.  All compute happens in
``eyoc_amd/lib/libeyoc_hip.so`` (hand-written HIP for gfx950) through the C ABI of
``include/eyoc_hip.h``; there is no CPU fallback.
"""
from ._lib import EyocError, LIB_PATH  # noqa: F401
from .sparse_tensor import SparseTensor, CoordinateManager  # noqa: F401
from .model import (load_model, ResUNet2, ResUNetBN2, ResUNetBN2B, ResUNetBN2C, ResUNetBN2D,  # noqa: F401
                    ResUNetBN2E, ResUNetFatBN, MODELS, ResUNetIN2, ResUNetIN2B, ResUNetIN2C, ResUNetIN2D, ResUNetIN2E,
                    IN_MODELS)
from .eval import find_nn_gpu, pdist, find_corr, find_correspondences, random_sample, knn1_segmented  # noqa: F401
from .eval import knn1_mutual_segmented, mutual_correspondences  # noqa: F401
from .transform_estimation import (est_quad_linear_robust, estimate_transform, pose_estimation,  # noqa: F401
                                   rigid_transform_3d, transform, integrate_trans, est_quad_linear_robust_batched)
from .registration import (Matcher, registration_ransac_based_on_feature_matching,  # noqa: F401
                           ransac_from_correspondences, ransac_batched_from_correspondences, RegistrationResult)
from .metrics import registration_errors, apply_transform, evaluate_nn_dist  # noqa: F401
from .voxelize import sparse_quantize, sparse_quantize_batch, voxelize, extract_features  # noqa: F401
from .labels import (knn2_segmented, lowe_topk, spherical_filter, similarity_filter, load_dist_sim_map,  # noqa: F401
                     match_and_filter_corr, correspondences_under_pose, lowe_topk_segmented, pair_filter_batched, posed_nn_grid,
                     match_and_filter_corr_batched, correspondences_under_pose_batched, corr_through_registration, label_step)
from .validate import (valid_metrics_batched, decode_valid_records, ValidMeters, ValidStep, valid_step, valid_epoch)  # noqa: F401,E402
from .autograd import sparse_conv, contrastive_hardest_negative_loss  # noqa: F401,E402
from .loss import hardest_contrastive_loss, triplet_loss, hardest_triplet_loss  # noqa: F401,E402
from .loss import contrastive_loss, generate_rand_negative_pairs  # noqa: F401,E402
from .draws import DeviceDraws  # noqa: F401,E402
from .matches import (matching_indices_batched, get_matching_indices, compute_overlap_ratio, overlap_ratio_batched)  # noqa: F401,E402
from .trainbatch import TrainBatch, draw_augmentation  # noqa: F401,E402
from .icp import (estimate_normals, estimate_normals_batched, icp_plane_batched, registration_icp_point_to_plane)  # noqa: F401,E402
from .fpfh import (compute_fpfh_batched, compute_fpfh_feature, fpfh_descriptors, register_fpfh_batched)  # noqa: F401,E402
from .downsample import voxel_down_sample, voxel_down_sample_batched  # noqa: F401,E402
