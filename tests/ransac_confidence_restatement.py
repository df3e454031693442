"""The convergence criterion of ``eyoc_ransac_converging_batched_ws`` (include/eyoc_hip.h) restated in fp64 numpy, and the cases the
host test (tests/test_ransac_confidence_host.py, on top of oracle/ransac.py) and the GPU test (tests/test_gpu_ransac_confidence.py,
on top of the existing one-pass call) share.  No test in here.

Device and numpy ``log`` may differ in their last bits, so a decision taken where the checkpoint ``E`` and the required number of
iterations ``k`` agree to 1e-9 could go either way: ``borderline`` says so, and the tests assert that NO decision they look at is
borderline - a condition on their inputs, not a tolerance on the outcome."""
from __future__ import annotations

import numpy as np

C_DEFAULT = 0.999


def as_device(c: float) -> float:
    """The confidence the device computes with: the C ABI carries it as fp32, the kernel widens that value to fp64."""
    return float(np.float32(c))


def checkpoints(first_check: int, H: int) -> list:
    """``E_0 = min(first_check, H)``, ``E_{j+1} = min(2 E_j, H)``, up to and including ``H``."""
    assert first_check >= 1 and H >= 1
    E = [min(int(first_check), int(H))]
    while E[-1] < H:
        E.append(min(2 * E[-1], int(H)))
    return E


def required_iterations(inliers: int, n: int, c: float) -> float:
    """``k = log(1 - c) / log(1 - f^4)`` with ``f = inliers / n`` in fp64, ``f^4`` as ``(f f)(f f)``.  ``inf`` with no inlier (the pair
    is never finished), 0 where ``f^4 >= 1`` (it is finished at once).  ``c`` is taken as it is: pass ``as_device(c)`` for the number
    the kernel computes (k moves by 2e-6 of itself between 0.999 and fp32(0.999))."""
    if inliers <= 0:
        return float("inf")
    c64 = np.float64(c)
    f = np.float64(inliers) / np.float64(n)
    q = (f * f) * (f * f)
    if q >= 1.0:
        return 0.0
    return float(np.log(np.float64(1.0) - c64) / np.log(np.float64(1.0) - q))


def borderline(E: int, k: float) -> bool:
    return bool(np.isfinite(k) and abs(E - k) <= 1e-9 * k)


def stop_checkpoint(inliers_at, n: int, c: float, first_check: int, H: int):
    """``inliers_at(E)``: the inlier count of the best record over all h < E (0: nothing survived).  -> ``(the checkpoint at which the
    pair stops, or H; [(E, inliers, k, finished)] for every checkpoint looked at)``.  ``c >= 1`` never stops early."""
    seen = []
    for E in checkpoints(first_check, H):
        inl = int(inliers_at(E))
        k = required_iterations(inl, n, c) if c < 1.0 else float("inf")
        done = inl > 0 and float(E) >= k
        seen.append((E, inl, k, done))
        if done or E == H:
            return E, seen
    raise AssertionError("unreachable: the last checkpoint is H")


# ---- the shared cases: gi.corr_case(1000 + n, n, T0, frac, noise=0.03), threshold 0.3, seed 7, c = 0.999
THRESHOLD, SEED = 0.3, 7
T0_ARGS = (0.02, -0.01, 0.12, 4.0, -1.0, 0.3)          # T0 of tests/test_gpu_ransac_generate.py
# name -> (n, frac, H, first_check, final inliers, k, stops at)
HOST_CASES = {
    "frac0.5": (600, 0.5, 1 << 17, 1024, 315, 87.4, 1024),
    "frac0.3": (600, 0.3, 1 << 17, 1024, 191, 669.2, 1024),
    "frac0.15": (600, 0.15, 1 << 17, 1024, 105, 7361.7, 8192),
    "frac0.08": (600, 0.08, 1 << 17, 1024, 60, 69074.1, 1 << 17),
    "all_inliers": (5, 1.0, 1 << 12, 64, 5, 0.0, 64),
}


def case_points(name):
    import _inputs as gi
    n, frac = HOST_CASES[name][:2]
    p0, p1, _ = gi.corr_case(1000 + n, n, gi.rigid(*T0_ARGS), frac, noise=0.03)
    return p0, p1
