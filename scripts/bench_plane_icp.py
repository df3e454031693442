"""Point-to-plane ICP against point-to-point ICP (eyoc_amd.icp, csrc/icp.hip sections 2, 5 and 6) on the same sample sets.

  python scripts/bench_plane_icp.py [--pairs 64] [--iters 10] [--warmup 2] [--reg-steps 4] [--out result.json]

(a) ``--pairs`` pairs x 5000 sampled points, gate 2 x voxel_size, 30 iterations, every pair started from its ground truth turned by 1
    degree and shifted by ~0.2 m: the normals of the target sample sets (radius 5 x voxel_size, 30 neighbours), ``icp_plane_batched`` with
    those normals and ``icp_batched``.  The three calls are timed in turn inside one loop (device events, warmed), so that clocks and
    cache state drift over all of them alike; iterations, convergence and the errors against ``T_gt`` come from the same calls.
(b) the harness: one ``RegistrationPipeline.register`` step with the ICP stage off, ``icp_method="point"`` and ``"plane"``, alternating,
    synchronised wall clock with the read-back; RTE / RRE of the registered pairs for each.

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_icp import make_pairs, perturb  # noqa: E402


def errors(Ts, pairs):
    """-> mean / median / max of RTE (m) and RRE (deg) of ``Ts f64 [P, 4, 4]`` against the pairs' ground truth"""
    from eyoc_amd.metrics import registration_errors
    rte, rre = [], []
    for T, p in zip(Ts, pairs):
        a, b, _ = registration_errors(np.asarray(T, np.float32), np.asarray(p["T_gt"], np.float32), 2.0, 5.0)
        rte.append(float(a)); rre.append(float(np.rad2deg(b)))
    return {"rte_mean": float(np.mean(rte)), "rte_median": float(np.median(rte)), "rte_max": float(np.max(rte)),
            "rre_deg_mean": float(np.mean(rre)), "rre_deg_median": float(np.median(rre)), "rre_deg_max": float(np.max(rre))}


def summarise(res, pairs):
    from eyoc_amd import icp
    rs = [icp.decode_icp_result(r) for r in res.cpu()]
    its = [r.iterations for r in rs]
    return {"iterations_mean": float(np.mean(its)), "iterations_min": int(np.min(its)), "iterations_max": int(np.max(its)),
            "converged": int(sum(bool(r.status & icp.CONVERGED) for r in rs)), "singular": int(sum(bool(r.status & icp.SINGULAR) for r in rs)),
            "fitness_mean": float(np.mean([r.fitness for r in rs])), "rmse_mean": float(np.mean([r.inlier_rmse for r in rs])),
            **errors([r.transformation for r in rs], pairs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reg-steps", type=int, default=4)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    P = args.pairs
    seeds = list(range(P))
    pairs = make_pairs(seeds, args.workers)

    import torch
    import eyoc_amd
    from eyoc_amd import icp
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    if not torch.cuda.is_available():
        raise SystemExit("bench_plane_icp.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = RegistrationConfig()
    batch = DeviceBatch(pairs, seeds, dev, cfg.n_points, descriptor=dict(inlier_ratio=0.3))
    init_h = np.stack([perturb(p["T_gt"], np.random.default_rng(s), 1.0, 0.2) for p, s in zip(pairs, seeds)])
    init = torch.from_numpy(init_h).to(dev)
    x0, x1 = batch.xyz0.reshape(-1, 3), batch.xyz1.reshape(-1, 3)
    gate, radius, max_nn = 2 * cfg.voxel_size, 5 * cfg.voxel_size, cfg.icp_normal_max_nn
    normals, count, status = icp.estimate_normals_batched(x1, batch.seg, radius, max_nn, return_count=True)
    fns = {"normals": lambda: icp.estimate_normals_batched(x1, batch.seg, radius, max_nn)[0],
           "plane": lambda: icp.icp_plane_batched(x0, x1, normals, batch.seg, batch.seg, gate, init, 30),
           "point": lambda: icp.icp_batched(x0, x1, batch.seg, batch.seg, gate, init, 30)}
    out = {}
    for _ in range(args.warmup):
        for k, fn in fns.items():
            out[k] = fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.iters):          # one loop over all three: what drifts, drifts for all of them
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out[k] = fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    timing = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for k, v in ms.items()}
    count_h = count.cpu().numpy()
    result = {"pairs": P, "points": cfg.n_points, "gate": gate, "normal_radius": radius, "max_nn": max_nn, "max_iteration": 30,
              "start": errors(init_h, pairs),
              "normals": {**timing["normals"], "rows_without_normal": float((count_h < 3).mean()), "rows_cut": float((count_h == max_nn).mean()),
                          "clouds_with_status": int((status != 0).sum())},
              "plane": {**timing["plane"], **summarise(out["plane"], pairs)},
              "point": {**timing["point"], **summarise(out["point"], pairs)}}

    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in syn.make_weights().items()})
    model = model.to(dev).eval()
    pipes = {"off": RegistrationPipeline(model, RegistrationConfig()),
             "point": RegistrationPipeline(model, RegistrationConfig(icp_refine=True)),
             "plane": RegistrationPipeline(model, RegistrationConfig(icp_refine=True, icp_method="plane"))}
    for _ in range(2):
        for pipe in pipes.values():
            pipe.register(batch, seed=0, return_device=True).cpu()
    torch.cuda.synchronize()
    wall = {k: [] for k in pipes}
    for _ in range(args.reg_steps):
        for k, pipe in pipes.items():
            t0 = time.perf_counter()
            pipe.register(batch, seed=0, return_device=True).cpu()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    model.check_range()
    reg = {}
    for k, pipe in pipes.items():
        rows = pipe.evaluate(batch, pipe.register(batch, seed=0))
        reg[k] = {"step_ms": float(np.median(wall[k])), "rte_mean": float(np.mean([r["rte"] for r in rows])),
                  "rte_median": float(np.median([r["rte"] for r in rows])), "rre_deg_mean": float(np.mean([r["rre_deg"] for r in rows])),
                  "rre_deg_median": float(np.median([r["rre_deg"] for r in rows])), "success": int(sum(r["success"] for r in rows))}
        if pipe.last_icp is not None:
            reg[k]["icp_iterations_mean"] = float(np.mean([r.iterations for r in pipe.last_icp]))
            reg[k]["icp_status"] = sorted({int(r.status) for r in pipe.last_icp})
    result["register"] = reg

    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
