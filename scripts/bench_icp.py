"""ICP refinement (eyoc_amd.icp, csrc/icp.hip): what the stage costs.

  python scripts/bench_icp.py [--pairs 64] [--iters 10] [--warmup 2] [--reg-steps 6] [--only harness|gt] [--out result.json]

(a) the harness stage: ``--pairs`` pairs x 5000 sampled points, gate 2 x voxel_size, 30 iterations - ``icp_batched`` alone (device
    events around warmed calls), and inside ``RegistrationPipeline.register`` (one step with the stage off and on, alternating,
    synchronised wall clock, read-back included);
(b) the ground-truth case of lib/data_loaders.py:485-515: the raw sweeps of ``make_pair(keep_raw=True)`` voxelised at 5 cm (~100 k
    points per cloud), gate 0.2, 200 iterations, 1 pair and 8 pairs in one call.
The launch count of a call is a host-side fact of the library: 2 per evaluation (``eval_solve_launches``) + the grid build (3 kernels,
1 fill, 2 radix sorts), whatever the number of pairs (up to 64 per launch set); the kernel split comes from a profiler run of this script:

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o icp -- python scripts/bench_icp.py --only gt --iters 2 --workers 1
  python scripts/kstats.py <dir>

(``--workers 1`` under the profiler: the scene generator's forked pool workers inherit the profiler's signal handler and do not exit
when the pool terminates them.)

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


def _pair(seed):
    from eyoc_amd import synthetic as syn
    return syn.make_pair(seed, keep_raw=True)


def make_pairs(seeds, workers):
    """Before this process touches the GPU: the workers are forked."""
    import multiprocessing as mp
    if workers <= 1:
        return [_pair(s) for s in seeds]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_pair, seeds)


def perturb(T, rng, rot_deg, trans):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = np.deg2rad(rot_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    D[:3, 3] = rng.normal(size=3) * trans / np.sqrt(3)
    return D @ np.asarray(T, np.float64)


def event_ms(fn, iters, warmup):
    """Median / min device time of ``fn`` between two events on the current stream, after ``warmup`` calls."""
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}, out


def summarise(res):
    from eyoc_amd import icp
    rs = [icp.decode_icp_result(r) for r in res.cpu()]
    return {"iterations": [r.iterations for r in rs], "converged": int(sum(bool(r.status & icp.CONVERGED) for r in rs)),
            "fitness_mean": float(np.mean([r.fitness for r in rs])), "rmse_mean": float(np.mean([r.inlier_rmse for r in rs]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reg-steps", type=int, default=6)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--only", choices=("harness", "gt"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n_gt = 8
    seeds = list(range(max(args.pairs if args.only != "gt" else 0, n_gt if args.only != "harness" else 0)))
    pairs = make_pairs(seeds, args.workers)

    import torch
    import eyoc_amd
    from eyoc_amd import icp
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    if not torch.cuda.is_available():
        raise SystemExit("bench_icp.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    result = {}

    if args.only != "gt":
        P = args.pairs
        cfg = RegistrationConfig()
        batch = DeviceBatch(pairs[:P], seeds[:P], dev, cfg.n_points, descriptor=dict(inlier_ratio=0.3))
        init = torch.from_numpy(np.stack([perturb(p["T_gt"], np.random.default_rng(s), 1.0, 0.2) for p, s in zip(pairs[:P], seeds[:P])])).to(dev)
        x0, x1 = batch.xyz0.reshape(-1, 3), batch.xyz1.reshape(-1, 3)
        gate = 2 * cfg.voxel_size
        ms, res = event_ms(lambda: icp.icp_batched(x0, x1, batch.seg, batch.seg, gate, init, 30), args.iters, args.warmup)
        ms1, _ = event_ms(lambda: icp.icp_batched(x0[:cfg.n_points], x1[:cfg.n_points], [0, cfg.n_points], [0, cfg.n_points], gate, init[:1], 30),
                          args.iters, args.warmup)
        result["harness_stage"] = {"pairs": P, "points": cfg.n_points, "gate": gate, "max_iteration": 30, "eval_solve_launches": 2 * 31, **ms,
                                   "one_pair": ms1, **summarise(res)}
        model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
        model.load_state_dict({k: torch.from_numpy(np.asarray(w)) for k, w in syn.make_weights().items()})
        model = model.to(dev).eval()
        off, on = RegistrationPipeline(model, RegistrationConfig()), RegistrationPipeline(model, RegistrationConfig(icp_refine=True))
        step = lambda pipe: (lambda: pipe.register(batch, seed=0, return_device=True).cpu())      # noqa: E731
        fns = {"off": step(off), "on": step(on)}
        for _ in range(2):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        wall = {k: [] for k in fns}
        for _ in range(args.reg_steps):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        model.check_range()
        rows_off = off.evaluate(batch, off.register(batch, seed=0))
        rows_on = on.evaluate(batch, on.register(batch, seed=0))
        result["register_step_ms"] = {k: float(np.median(v)) for k, v in wall.items()}
        result["register"] = {"rte_mean_off": float(np.mean([r["rte"] for r in rows_off])), "rte_mean_on": float(np.mean([r["rte"] for r in rows_on])),
                              "rre_deg_mean_off": float(np.mean([r["rre_deg"] for r in rows_off])),
                              "rre_deg_mean_on": float(np.mean([r["rre_deg"] for r in rows_on])),
                              "success_off": int(sum(r["success"] for r in rows_off)), "success_on": int(sum(r["success"] for r in rows_on)),
                              "icp_iterations": [r.iterations for r in on.last_icp]}

    if args.only != "harness":
        clouds = []
        for p in pairs[:n_gt]:
            x0 = p["raw0"][syn.voxelize(p["raw0"], 0.05)[0]][:, :3]
            x1 = p["raw1"][syn.voxelize(p["raw1"], 0.05)[0]][:, :3]
            clouds.append((torch.from_numpy(np.ascontiguousarray(x0, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(x1, np.float32)).to(dev)))
        init = torch.from_numpy(np.stack([perturb(p["T_gt"], np.random.default_rng(s), 1.0, 0.2) for p, s in zip(pairs[:n_gt], seeds)])).to(dev)
        gt = {}
        for P in (1, n_gt):
            S, T = torch.cat([c[0] for c in clouds[:P]]), torch.cat([c[1] for c in clouds[:P]])
            seg_s = np.concatenate([[0], np.cumsum([len(c[0]) for c in clouds[:P]])])
            seg_t = np.concatenate([[0], np.cumsum([len(c[1]) for c in clouds[:P]])])
            ms, res = event_ms(lambda: icp.icp_batched(S, T, seg_s, seg_t, 0.2, init[:P], 200), max(args.iters // 2, 2), 1)
            gt[f"pairs_{P}"] = {"source_points": int(seg_s[-1]), "target_points": int(seg_t[-1]), "eval_solve_launches": 2 * 201, **ms, **summarise(res)}
        result["ground_truth_case"] = {"voxel": 0.05, "gate": 0.2, "max_iteration": 200, **gt}

    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
