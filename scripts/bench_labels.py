"""Label generation of one training iteration (eyoc_amd.labels): the per-pair route against ``label_step``, in one process.

  python scripts/bench_labels.py [--batches 4,16] [--iters 10] [--warmup 2] [--workers 8] [--out result.json]

Synthetic pairs of ~30 k voxels (``synthetic.make_pair``) with descriptors planted on the voxels the two clouds share under the
ground-truth pose (noisy copies; the rest random), so that the matches, the registration and the 2 m gate all have real work.

  per_pair   exactly the composition INTEGRATION.md 2b shows: ``match_and_filter_corr`` -> gather -> ``Matcher.SC2_PCR_batch`` ->
             ``correspondences_under_pose(..., T.cpu().numpy())`` once per pair
  batched    ``label_step`` (``match_and_filter_corr_batched`` -> ``corr_through_registration``)

Both routes run on the same inputs with generators seeded alike, alternating, each call ended by a device synchronise; the figure is
the median wall-clock time of ``--iters`` calls after ``--warmup``.  A second pass synchronises after every stage for the split
(its stages therefore sum to more than the whole).  The two routes' outputs are compared once (byte-equal or the script fails).
On a tree without ``label_step`` only the per-pair route is measured.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATCHER = dict(inlier_threshold=0.6, d_thre=0.1, ratio=0.2, nms_radius=0.6, max_points=8000, k1=30, k2=20, num_iterations=20)


def _pair(seed):
    from eyoc_amd import synthetic as syn
    return syn.make_pair(seed)


def make_pairs(seeds, workers):
    """Before this process touches the GPU: the workers are forked."""
    import multiprocessing as mp
    if workers <= 1:
        return [_pair(s) for s in seeds]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_pair, seeds)


def plant_features(pair, seed, dev):
    """Unit descriptors [n, 32]: a voxel of cloud 1 whose nearest posed voxel of cloud 0 lies within 0.3 m carries a noisy copy of that
    voxel's descriptor, every other one is random."""
    import torch
    import eyoc_amd
    from eyoc_amd import labels
    g = torch.Generator().manual_seed(seed)
    x0, x1 = torch.from_numpy(pair["xyz0"]).to(dev), torch.from_numpy(pair["xyz1"]).to(dev)
    F0 = torch.nn.functional.normalize(torch.randn(len(x0), 32, generator=g), dim=1).to(dev)
    F1 = torch.nn.functional.normalize(torch.randn(len(x1), 32, generator=g), dim=1).to(dev)
    Tinv = np.linalg.inv(np.asarray(pair["T_gt"], np.float64)).astype(np.float32)
    pad = lambda P: torch.cat([P, torch.zeros((P.shape[0], 1), device=P.device)], 1).contiguous()      # noqa: E731
    idx, d1, _ = eyoc_amd.knn2_segmented(pad(labels.apply_pose(Tinv, x1)), pad(x0), [0, len(x1)], [0, len(x0)])
    near = d1 < 0.09
    noisy = torch.nn.functional.normalize(F0[idx] + 0.05 * torch.randn(len(x1), 32, generator=g).to(dev), dim=1)
    F1 = torch.where(near[:, None], noisy, F1)
    return x0, F0.contiguous(), x1, F1.contiguous(), float(near.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    pairs = make_pairs(list(range(max(batches))), args.workers)

    import torch
    import eyoc_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_labels.py needs an MI355X: the hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    has_batched = hasattr(eyoc_amd, "label_step")
    matcher = eyoc_amd.Matcher(**MATCHER)
    data = [plant_features(p, s, dev) for s, p in enumerate(pairs)]
    sync = torch.cuda.synchronize
    result = {"voxels_mean": float(np.mean([len(d[0]) + len(d[2]) for d in data]) / 2), "shared_fraction": float(np.mean([d[4] for d in data])),
              "num_corres": 5000, "n_sample": 5000, "iters": args.iters, "has_batched": has_batched}

    for B in batches:
        C0, F0, C1, F1 = ([d[i] for d in data[:B]] for i in range(4))
        stages = {"per_pair": {}, "batched": {}}

        def tick(route, name, t0, split):
            if split:
                sync()
                stages[route].setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
            return time.perf_counter()

        def per_pair(split=False):
            g = torch.Generator().manual_seed(1)
            t = time.perf_counter()
            matches, unc = eyoc_amd.match_and_filter_corr(C0, F0, C1, F1, radius=20, feature_filter="Lowe", spatial_filter="Spherical")
            t = tick("per_pair", "match_and_filter", t, split)
            src = [C0[i][u[:, 0]] for i, u in enumerate(unc)]
            tgt = [C1[i][u[:, 1]] for i, u in enumerate(unc)]
            poses = matcher.SC2_PCR_batch(src, tgt)
            t = tick("per_pair", "registration", t, split)
            corr = [eyoc_amd.correspondences_under_pose(C0[i], C1[i], T.cpu().numpy(), generator=g) for i, (T, _) in enumerate(poses)]
            tick("per_pair", "under_pose", t, split)
            return poses, corr

        def batched(split=False):
            g = torch.Generator().manual_seed(1)
            if not split:
                return eyoc_amd.label_step(C0, F0, C1, F1, matcher, radius=20, feature_filter="Lowe", spatial_filter="Spherical", generator=g)
            from eyoc_amd import labels
            t = time.perf_counter()
            matches, unc = eyoc_amd.match_and_filter_corr_batched(C0, F0, C1, F1, radius=20, feature_filter="Lowe", spatial_filter="Spherical")
            t = tick("batched", "match_and_filter", t, True)
            # corr_through_registration in its two halves
            P0, seg0 = labels._pack_clouds(C0)
            P1, seg1 = labels._pack_clouds(C1, dev)
            us = [u[:matcher.max_points] for u in unc]
            src = torch.cat([C0[i][u[:, 0]] for i, u in enumerate(us)])
            tgt = torch.cat([C1[i][u[:, 1]] for i, u in enumerate(us)])
            T, fit, _ = matcher.SC2_PCR_packed(src, tgt, labels._offsets([len(u) for u in us]))
            t = tick("batched", "registration", t, True)
            out = labels._under_pose_packed(P0, P1, seg0, seg1, T, 5000, 2.0, None, g)
            tick("batched", "under_pose", t, True)
            return out

        fns = {"per_pair": per_pair}
        if has_batched:
            fns["batched"] = batched
        out = {}
        for _ in range(args.warmup):
            for k, fn in fns.items():
                out[k] = fn()
                sync()
        if has_batched:             # the two routes agree byte for byte
            poses, corr = out["per_pair"]
            pos_pairs, unc_corr, T, fits = out["batched"]
            for b in range(B):
                assert torch.equal(T[b], poses[b][0]) and torch.equal(fits[b], poses[b][1]) and torch.equal(unc_corr[b], corr[b]), b
        ms = {k: [] for k in fns}
        for _ in range(args.iters):
            for k, fn in fns.items():
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for _ in range(max(args.iters // 2, 2)):
            for fn in fns.values():
                fn(True)
        poses, corr = out["per_pair"]
        result[f"B{B}"] = {
            "ms_median": {k: float(np.median(v)) for k, v in ms.items()}, "ms_min": {k: float(np.min(v)) for k, v in ms.items()},
            "ms_spread": {k: float(np.percentile(v, 90) - np.percentile(v, 10)) for k, v in ms.items()},
            "stage_ms_median": {r: {k: float(np.median(v)) for k, v in s.items()} for r, s in stages.items() if s},
            "labels_per_pair_mean": float(np.mean([len(c) for c in corr])),
            "registered": int(sum(eyoc_amd.registration_errors(T.cpu().numpy(), pairs[b]["T_gt"])[2] for b, (T, _) in enumerate(poses))),
        }

    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
