"""Generate ``g12_valid.npz``: the reference's validation metrics (lib/trainer.py:360-378 of ``_valid_epoch``) on seeded inputs.

Run in the build container only (``python tests/golden/make_golden_valid.py``); it imports the reference read-only through
``_refimport.install()`` and runs, unmodified, ``util.transform_estimation.est_quad_linear_robust``, ``lib.metrics.corr_dist`` and
``lib.trainer.ContrastiveLossTrainer.evaluate_hit_ratio`` (unbound, on ``object.__new__``: the method reads no attribute).  Nothing of
the reference is copied: the fixture holds the case table and the reference's numeric outputs; the inputs are regenerated from seeds
(``_inputs_valid.valid_case``).

Every case runs twice: with ``T_gt`` the true pose, and with the true pose composed with a 2 degree rotation and a 0.3 m shift.
Stored per (case, variant): ``T_est`` (per case), ``loss``, ``hit_ratio``, ``rte``, ``rre`` (and the cosine inside it) as the reference computes them,
``loss_gap = |reference fp32 corr_dist - fp64 restatement|`` and ``margin``: the smallest distance of a correspondence's fp64 hit distance
from the threshold, asserted to be at least ``MARGIN`` (a seed that fails is replaced).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refimport  # noqa: E402
_refimport.install()

import _inputs_valid as gv  # noqa: E402
from valid_restatement import hit_distances, valid_record  # noqa: E402
from util.transform_estimation import est_quad_linear_robust  # noqa: E402
from lib.metrics import corr_dist  # noqa: E402
from lib.trainer import ContrastiveLossTrainer  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(1)      # one summation order for the reference's fp32 means = a reproducible fixture


def g12(cases=gv.VALID_CASES, path=os.path.join(HERE, "g12_valid.npz")):
    me = object.__new__(ContrastiveLossTrainer)
    out = {"cases": np.array(json.dumps(cases)), "hit_thresh": np.array(gv.HIT_THRESH)}
    cols = {k: np.zeros((len(cases), 2)) for k in ("loss", "hit_ratio", "rte", "rre", "cos_rre", "loss_gap", "margin")}
    for c, (seed, n, frac, tp) in enumerate(cases):
        T_est = None
        for v in (0, 1):
            p0, p1, x0, T_gt_np = gv.valid_case(seed, n, frac, tp, bool(v))
            xyz0_corr, xyz1_corr, xyz0, T_gt = torch.from_numpy(p0), torch.from_numpy(p1), torch.from_numpy(x0), torch.from_numpy(T_gt_np)
            if T_est is None:
                T_est = est_quad_linear_robust(xyz0_corr, xyz1_corr)                 # lib/trainer.py:360
                out[f"T_est{c}"] = T_est.numpy().astype(np.float32)
            loss = corr_dist(T_est, T_gt, xyz0, None, weight=None)                   # :362 (xyz1 is not read)
            # :365-368, re-typed: the expressions are statements inside the loop body, not a callable
            rte = np.linalg.norm(T_est[:3, 3] - T_gt[:3, 3])
            cos_rre = (np.trace(T_est[:3, :3].t() @ T_gt[:3, :3]) - 1) / 2          # the argument of :367-368's arccos, kept as well
            with np.errstate(invalid="ignore"):
                rre = np.arccos(cos_rre)
            hit_ratio = ContrastiveLossTrainer.evaluate_hit_ratio(me, xyz0_corr, xyz1_corr, T_gt, thresh=gv.HIT_THRESH)   # :372-376
            rs = valid_record(p0, p1, None, x0, out[f"T_est{c}"], T_gt_np, gv.HIT_THRESH)
            margin = float(np.abs(hit_distances(p0, p1, None, T_gt_np) - gv.HIT_THRESH).min())
            assert margin >= gv.MARGIN, f"seed {seed} (n {n}, variant {v}): a hit distance lies {margin:.2e} from the threshold - replace the seed"
            assert rs["hits"] == round(float(hit_ratio) * n), (seed, v, rs["hits"], hit_ratio)
            cols["loss"][c, v], cols["hit_ratio"][c, v], cols["rte"][c, v], cols["rre"][c, v] = float(loss), float(hit_ratio), float(rte), float(rre)
            cols["cos_rre"][c, v] = float(cos_rre)
            cols["loss_gap"][c, v], cols["margin"][c, v] = abs(float(loss) - rs["loss"]), margin
            print(f"case {c} seed {seed} n {n} variant {v}: loss {float(loss):.6f} hit_ratio {float(hit_ratio):.4f} rte {float(rte):.5f} "
                  f"rre {float(rre):.6f} | loss_gap {cols['loss_gap'][c, v]:.2e} margin {margin:.2e} cos(restated) - 1 = {rs['cos_rre'] - 1:.3e}")
    out.update(cols)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    g12()
    print("wrote g12")
