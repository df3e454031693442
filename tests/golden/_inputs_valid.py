"""Deterministic inputs of the validation-metrics fixture (``g12_valid.npz``), shared by ``make_golden_valid.py`` (which runs the
reference on them) and the tests (which run the restatement / the HIP path on them).  Built on ``_inputs``: PCG64 uniform doubles and
element-wise IEEE operations only, so the arrays are bit-reproducible and the fixture stores the case table and OUTPUTS alone."""
import numpy as np

import _inputs as gi

EXTENT = np.array((60.0, 60.0, 6.0))
HIT_THRESH = 0.1         # config.py: hit_ratio_thresh
MARGIN = 2e-5            # no stored case has a correspondence whose fp64 hit distance is this close to HIT_THRESH (ten fp32 ulps at 32 m)

# (seed, n, inlier_frac, T params): every segment size class of the kernels (below a wave, one wave, below / above one 1024-row sweep,
# several sweeps); the seeds are those whose hit distances keep MARGIN (the generator asserts it)
VALID_CASES = [
    (45, 3, 1.0, (0.01, -0.02, 0.10, 1.0, -0.5, 0.1)),
    (44, 64, 0.9, (0.02, 0.01, -0.15, -2.0, 0.4, 0.0)),
    (42, 777, 0.7, (-0.01, 0.03, 0.20, 1.5, 0.3, -0.05)),
    (46, 1025, 0.5, (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
    (47, 1500, 0.35, (0.03, 0.00, 0.15, -1.2, 0.4, 0.0)),
    (49, 5000, 0.6, (0.02, -0.03, 0.30, 2.0, -0.5, 0.1)),
]
# the second T_gt of every case: the true pose composed with a 2 degree rotation and a 0.3 m shift (rre ~ 0.035 rad, well conditioned)
OFFSET = gi.rigid(0.0, 0.0, np.deg2rad(2.0), 0.3, 0.0, 0.0)


def full_cloud(seed, n):
    """The pair's full source cloud: ``4 n + 100`` uniform points of the scene box."""
    return ((gi._u(seed + 7, 4 * n + 100, 3) - 0.5) * EXTENT).astype(np.float32)


def valid_case(seed, n, frac, tp, offset):
    """-> ``p0, p1`` (``corr_case`` with noise 0.04), the full cloud ``x0`` and ``T_gt f32 [4, 4]``: the true pose, or (``offset``) the
    true pose composed with ``OFFSET``."""
    T = gi.rigid(*tp)
    p0, p1, _ = gi.corr_case(seed, n, T, frac, noise=0.04)
    T_gt = (T @ OFFSET if offset else T).astype(np.float32)
    return p0, p1, full_cloud(seed, n), T_gt
