"""Mutual nearest-neighbour matching (eyoc_amd.eval.mutual_correspondences): what a user could do before it against both routes of
``eyoc_knn1_mutual``, and the registration step with ``mutual_filter`` on against off, in one process.

  python scripts/bench_mutual.py [--pairs 64,1] [--n 5000] [--iters 30] [--warmup 3] [--step-pairs 64] [--step-iters 5] [--out result.json]

Query part.  ``P`` pairs of ``n`` unit descriptors [n, 32], SquareL2, index query: the targets are random, 30 % of the sources are noisy
copies of distinct targets (the bench's planted inlier ratio), the rest random.

  two_calls  two ``knn1_segmented`` calls, the reciprocity test in torch, one boolean-mask ``nonzero`` per pair (a read-back each)
  route0     ``eyoc_knn1_mutual`` as two one-way queries + ``eyoc_mutual_compact`` + the read-back of the segment offsets
  route1     the same with the fused sweep (``knn1_mutual_kernel``)
  auto       the same with the library's own choice between the two

The four run on the same inputs, alternating, each call ended by a device synchronise; the figure is the median wall-clock time of
``--iters`` calls after ``--warmup``.  Their kept rows and neighbours are compared once (equal or the script fails).

Step part (``--step-pairs 0`` skips it).  ``RegistrationPipeline.register`` on one batch of synthetic pairs in the benchmark's descriptor
mode (inlier ratio 0.3), ``mutual_filter`` off and on, alternating: ms per step, pairs registered, mean RTE / RRE of the registered pairs,
and the mean share of correspondences the filter kept.  Prints one JSON line."""
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
    return syn.make_pair(seed)


def make_pairs(seeds, workers):
    """Before this process touches the GPU: the workers are forked."""
    import multiprocessing as mp
    if workers <= 1 or len(seeds) <= 1:
        return [_pair(s) for s in seeds]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_pair, seeds)


def descriptors(P, n, dev, ratio=0.3, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    F1 = torch.nn.functional.normalize(torch.randn(P, n, 32, generator=g), dim=2)
    F0 = torch.nn.functional.normalize(torch.randn(P, n, 32, generator=g), dim=2)
    k = int(ratio * n)
    for p in range(P):
        src, tgt = torch.randperm(n, generator=g)[:k], torch.randperm(n, generator=g)[:k]
        F0[p, src] = torch.nn.functional.normalize(F1[p, tgt] + 0.05 * torch.randn(k, 32, generator=g), dim=1)
    return F0.reshape(-1, 32).contiguous().to(dev), F1.reshape(-1, 32).contiguous().to(dev)


def query_part(P, n, iters, warmup, dev):
    import torch
    from eyoc_amd import _lib
    from eyoc_amd.eval import knn1_segmented, mutual_correspondences
    F0, F1 = descriptors(P, n, dev)
    seg = np.arange(P + 1) * n
    first = torch.arange(P, device=dev).repeat_interleave(n) * n
    arange = torch.arange(P * n, device=dev)
    sync = torch.cuda.synchronize

    def two_calls():
        ab = knn1_segmented(F0, F1, seg, seg, "SquareL2", return_distance=False)
        ba = knn1_segmented(F1, F0, seg, seg, "SquareL2", return_distance=False)
        mutual = ba[ab + first] + first == arange
        rows = [torch.nonzero(mutual[p * n:(p + 1) * n]).reshape(-1) for p in range(P)]
        return rows, [ab[p * n:(p + 1) * n][r] for p, r in enumerate(rows)]

    def route(mode):
        def run():
            _lib.knob("eyoc_knn_mutual_select", mode)
            return mutual_correspondences(F0, F1, seg, seg, "SquareL2")
        return run

    fns = {"two_calls": two_calls, "route0": route(0), "route1": route(1), "auto": route(-1)}
    prev = _lib.knob("eyoc_knn_mutual_select", -2) - 2
    try:
        out = {}
        for _ in range(warmup):
            for k, fn in fns.items():
                out[k] = fn()
                sync()
        rows, corr = (torch.cat(v) for v in out["two_calls"])
        for k in ("route0", "route1", "auto"):
            r, c, s = out[k]
            assert torch.equal(r, rows) and torch.equal(c, corr) and int(s[-1]) == len(rows), k
        ms = {k: [] for k in fns}
        for _ in range(iters):
            for k, fn in fns.items():
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                ms[k].append((time.perf_counter() - t0) * 1e3)
    finally:
        _lib.knob("eyoc_knn_mutual_select", prev)
    return {"ms_median": {k: float(np.median(v)) for k, v in ms.items()}, "ms_min": {k: float(np.min(v)) for k, v in ms.items()},
            "ms_spread": {k: float(np.percentile(v, 90) - np.percentile(v, 10)) for k, v in ms.items()},
            "mutual_share": float(len(rows) / (P * n))}


def step_part(pairs, iters, warmup, hyp, dev):
    import torch
    import eyoc_amd
    from eyoc_amd import synthetic as syn
    from eyoc_amd.harness import DeviceBatch, RegistrationConfig, RegistrationPipeline
    sd = syn.make_weights()
    model = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(dev).eval()
    P = len(pairs)
    batch = DeviceBatch(pairs, list(range(P)), dev, descriptor=dict(inlier_ratio=0.3))
    pipes = {k: RegistrationPipeline(model, RegistrationConfig(ransac_max_iteration=hyp, mutual_filter=k == "on")) for k in ("off", "on")}
    sync = torch.cuda.synchronize
    res = {}
    for _ in range(warmup):
        for k, pipe in pipes.items():
            res[k] = pipe.register(batch)
            sync()
    ms = {k: [] for k in pipes}
    for _ in range(iters):
        for k, pipe in pipes.items():
            sync()
            t0 = time.perf_counter()
            pipe.register(batch)
            sync()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"pairs": P, "ransac_iters": hyp}
    for k, pipe in pipes.items():
        ev = pipe.evaluate(batch, res[k])
        ok = [e for e in ev if e["success"]]
        out[k] = {"ms_median": float(np.median(ms[k])), "ms_min": float(np.min(ms[k])), "registered": len(ok),
                  "rte_mean": float(np.mean([e["rte"] for e in ok])) if ok else None,
                  "rre_deg_mean": float(np.mean([e["rre_deg"] for e in ok])) if ok else None,
                  "fitness_mean": float(np.mean([r.fitness for r in res[k]]))}
    # the share of correspondences the filter kept, and how many of the kept / of all are true (ground-truth residual below the threshold)
    from eyoc_amd.eval import mutual_correspondences
    pipes["on"].register(batch)
    out["on"]["inlier_ratio_all"] = float(np.nanmean(pipes["on"].correspondence_inlier_ratio(batch)))
    F = pipes["off"]._features(batch, None, sampled=True)[0]
    import types
    F0, F1 = pipes["off"]._sampled_halves(types.SimpleNamespace(batch=batch, F=F))
    _, _, seg = mutual_correspondences(F0, F1, batch.seg, batch.seg, min_keep=4)
    out["on"]["kept_share_mean"] = float(np.mean(np.diff(seg) / batch.n_points))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="64,1")
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-pairs", type=int, default=64)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--ransac-iters", type=int, default=4000000)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pairs = make_pairs(list(range(args.step_pairs)), args.workers) if args.step_pairs > 0 else []

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mutual.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    result = {"n": args.n, "iters": args.iters}
    for P in [int(p) for p in args.pairs.split(",") if p]:
        result[f"P{P}"] = query_part(P, args.n, args.iters, args.warmup, dev)
    if pairs:
        result["step"] = step_part(pairs, args.step_iters, max(args.warmup - 1, 1), args.ransac_iters, dev)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
