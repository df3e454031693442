"""Ground-truth matching indices (eyoc_amd.matches, csrc/icp.hip section 4): what the route costs.

  python scripts/bench_matches.py [--pairs 64] [--iters 10] [--warmup 2] [--host-pairs 8] [--out result.json]

At the bench's geometry - ``--pairs`` pairs of ``synthetic.make_pair`` (0.3 m voxels, about 30 k per cloud), radius 0.45 m - once with
the identity (the base stage) and once with the ground-truth pose (validation):
  batched     one ``matching_indices_batched`` call for all pairs, collated, its one read-back included (synchronised wall clock, and
              device events around the same call)
  single      one ``get_matching_indices`` call per pair, all pairs (synchronised wall clock)
  count/fill  the two passes of the batched call on their own (device events; the fill without the allocation of its output)
  host        ``scipy.spatial.cKDTree.query_ball_point`` per pair on ``--host-pairs`` pairs, scaled to ``--pairs`` (one thread, what
              scripts/train_synthetic.py does today); the clouds are already on the host, no transfer is counted
The clouds are on the device before the clock starts.  Prints one JSON line."""
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
    p = syn.make_pair(seed)
    return {k: p[k] for k in ("xyz0", "xyz1", "T_gt")}


def make_pairs(seeds, workers):
    """Before this process touches the GPU: the workers are forked."""
    import multiprocessing as mp
    if workers <= 1:
        return [_pair(s) for s in seeds]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_pair, seeds)


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def event_ms(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return _stats(ms)


def wall_ms(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms)


def host_route(x0, x1, T, r):
    """All neighbours inside r of every posed source point, as (i, j), nearest first: the KD-tree on the host."""
    from scipy.spatial import cKDTree
    p = x0.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    q = x1.astype(np.float64)
    out = []
    for i, cand in enumerate(cKDTree(q).query_ball_point(p, r)):
        if cand:
            j = np.asarray(cand)
            d = ((q[j] - p[i]) ** 2).sum(1)
            o = np.lexsort((j, d))
            out.append(np.stack([np.full(len(o), i), j[o]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-pairs", type=int, default=8)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--radius", type=float, default=0.45)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pairs = make_pairs(list(range(args.pairs)), args.workers)

    import torch
    from eyoc_amd import matches
    if not torch.cuda.is_available():
        raise SystemExit("bench_matches.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    P, r = args.pairs, args.radius
    c0 = [torch.from_numpy(np.ascontiguousarray(p["xyz0"], np.float32)).to(dev) for p in pairs]
    c1 = [torch.from_numpy(np.ascontiguousarray(p["xyz1"], np.float32)).to(dev) for p in pairs]
    S, T = torch.cat(c0), torch.cat(c1)
    seg0 = [0] + [int(v) for v in np.cumsum([len(c) for c in c0])]
    seg1 = [0] + [int(v) for v in np.cumsum([len(c) for c in c1])]
    gt = np.stack([np.asarray(p["T_gt"], np.float64) for p in pairs])
    result = {"pairs": P, "radius": r, "source_points": seg0[-1], "target_points": seg1[-1],
              "workspace_mb": matches._lib.load().eyoc_radius_matches_workspace_bytes(P, seg0[-1], seg1[-1]) / 2 ** 20}

    for name, poses in (("identity", None), ("gt_pose", gt)):
        Td = None if poses is None else torch.from_numpy(poses).to(dev)
        corr, seg_m, status = matches.matching_indices_batched(S, T, Td, r, seg0=seg0, seg1=seg1)
        total = int(corr.shape[0])
        per_row = torch.diff(matches._Search("bench", S, T, Td, r, None, seg0, seg1).offsets)
        out = {"matches": total, "matches_per_source_mean": total / seg0[-1], "matches_per_source_max": int(per_row.max().item()),
               "status_nonzero": int((status != 0).sum().item())}
        out["batched_wall"] = wall_ms(lambda: matches.matching_indices_batched(S, T, Td, r, seg0=seg0, seg1=seg1), args.iters, args.warmup)
        out["batched_events"] = event_ms(lambda: matches.matching_indices_batched(S, T, Td, r, seg0=seg0, seg1=seg1), args.iters, args.warmup)

        def singles():
            for b in range(P):
                matches.get_matching_indices(c0[b], c1[b], None if poses is None else poses[b], r)
        out["single_wall"] = wall_ms(singles, max(args.iters // 3, 2), 1)
        out["count_events"] = event_ms(lambda: matches._Search("bench", S, T, Td, r, None, seg0, seg1), args.iters, args.warmup)
        q = matches._Search("bench", S, T, Td, r, None, seg0, seg1)
        out["fill_events"] = event_ms(lambda: q.fill(total), args.iters, args.warmup)
        out["count_K1_events"] = event_ms(lambda: matches._Search("bench", S, T, Td, r, 1, seg0, seg1), args.iters, args.warmup)
        # the host route, on the first pairs; its result is the device's (sets compared, the orders agree up to ties in fp64 rounding)
        hp = min(args.host_pairs, P)
        t0 = time.perf_counter()
        host = [host_route(pairs[b]["xyz0"], pairs[b]["xyz1"], np.eye(4) if poses is None else poses[b], r) for b in range(hp)]
        host_ms = (time.perf_counter() - t0) * 1e3
        local, seg_l, _ = matches.matching_indices_batched(c0[:hp], c1[:hp], None if poses is None else poses[:hp], r, collated=False)
        local, seg_l = local.cpu().numpy(), seg_l.cpu().numpy()
        same = sum(set(map(tuple, host[b])) == set(map(tuple, local[seg_l[b]:seg_l[b + 1]])) for b in range(hp))
        out["host_ckdtree"] = {"pairs_timed": hp, "wall_ms": host_ms, "scaled_to_all_pairs_ms": host_ms * P / hp, "pairs_with_the_same_set": int(same)}
        result[name] = out

    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
